"""The training iteration's log (train.py:188-200, 402-433): the reference's eager statements, with their host copies and
.item()s, against gftorf_amd.tof.TrainLog.record, timed against each other in one process.

    eager         the statements as train.py writes them: depth_from_tof_torch twice with .item()s of depth_range and the
                  offset, five images copied to the host, the scattering-phase maps and their means in numpy, the two means
                  over get_features_phasor[:, 0, 1] (one through [visibility_filter]), the two depth errors, five .item()s
    record        log.record(...) eagerly: two launches, nothing read on the host
    record_graph  the same call replayed from a graph (the eager statements cannot be captured: they read the host)

at 320x240 with P = 100 k Gaussians and at 640x480 with P = 1 M, 60 % visible rows.  Device events around windows of many
iterations after a warm-up, the routes alternating window by window; the median window is reported.  (The eager route blocks
on the host every iteration, so its window is host + device time; the other two are enqueue-bound and device-bound.)  One run
per shape under a time limit of its own:

    timeout 300 python profiles/bench_tof_log.py --shape small --out profiles/tof_log_bench_small.json
    timeout 300 python profiles/bench_tof_log.py --shape large --out profiles/tof_log_bench_large.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROUNDS = 7
SHAPES = {"small": (100_000, 240, 320), "large": (1_000_000, 480, 640)}
SH_C0 = 0.28209479177387814


def alternate(routes, seconds):
    """routes: name -> callable that enqueues ONE iteration.  Returns name -> dict(ms, min_ms, max_ms, iters, windows)."""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    iters = {}
    for name, fn in routes.items():
        for _ in range(20):
            fn()
        a, b = ev(), ev()
        a.record()
        for _ in range(50):
            fn()
        b.record()
        torch.cuda.synchronize()
        per = max(a.elapsed_time(b) / 50, 1e-3)
        iters[name] = max(20, int(seconds * 1e3 / ROUNDS / per) + 1)
    times = {name: [] for name in routes}
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            a, b = ev(), ev()
            a.record()
            for _ in range(iters[name]):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / iters[name])
    return {name: dict(ms=statistics.median(t), min_ms=min(t), max_ms=max(t), iters=iters[name], windows=ROUNDS)
            for name, t in times.items()}


def eager_tof_depth(planes, depth_range, offset):
    """The eager launches of the reference's ToF depth (scene/torf_utils.py:59-64) in the same order: abs, lt, full_like,
    where, atan2, an in-place sub, lt, add, where, mul, div."""
    re, im = planes[0], planes[1]
    near_zero = torch.abs(re) < 1e-6
    safe_re = torch.where(near_zero, torch.full_like(re, 1e-6), re)
    angle = torch.atan2(im, safe_re)
    angle.sub_(offset)
    negative = angle < 0
    angle = torch.where(negative, angle + 2 * torch.pi, angle)
    return angle * depth_range / (4 * torch.pi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="small")
    ap.add_argument("--visible", type=float, default=0.6)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--coefficients", choices=("features_phasor", "amp_f_dc"), default="features_phasor",
                    help="what record reads the amplitude coefficients from: element [:, 0, 1] of the [P, 16, 2] tensor in place "
                         "(128 bytes apart) or the model's own [P, 1, 1] tensor (4 bytes apart)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tof_log.py needs a HIP device: there is nothing to time without one")
    from gftorf_amd import tof
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    P, H, W = SHAPES[args.shape]
    phasor = torch.randn(7, H, W, device=dev)
    phasor[2].uniform_(0.02, 1.0)
    gt_phasor = torch.randn(3, H, W, device=dev)
    gt_phasor[2].uniform_(0.02, 1.0)
    depth = torch.empty(1, H, W, device=dev).uniform_(0.3, 5.0)
    gt_depth = depth + 0.2 * torch.randn_like(depth)
    dd = torch.rand(1, H, W, device=dev)
    features_phasor = torch.randn(P, 16, 2, device=dev)
    coefficients = {"features_phasor": features_phasor} if args.coefficients == "features_phasor" else \
        {"amp_f_dc": features_phasor[:, :1, 1:].contiguous()}
    radii = torch.where(torch.rand(P, device=dev) < args.visible, torch.randint(1, 40, (P,), device=dev), 0).to(torch.int32)
    depth_range, phase_offset = torch.tensor([10.0], device=dev), torch.tensor([0.1], device=dev)
    scalars = [torch.rand((), device=dev) for _ in range(5)]           # loss, Ll1, Ll1_p, the two flow terms
    sink = {}

    def eager():
        visibility_filter = radii > 0
        phase_depth = eager_tof_depth(phasor[:3], depth_range.item(), phase_offset.detach().cpu().numpy().item())
        gt_phase_depth = eager_tof_depth(gt_phasor[:3], depth_range.item(), phase_offset.detach().cpu().numpy().item())
        amp = (phasor[:3].cpu().detach().numpy().transpose(1, 2, 0) * 1.0)[:, :, 2]
        gt_amp = gt_phasor.cpu().detach().numpy().transpose(1, 2, 0)[:, :, 2]
        gsp = gt_amp * (gt_phase_depth.cpu().detach().numpy() ** 2)
        sp = amp * (depth.cpu().detach().numpy()[0] ** 2)
        sp_tof = amp * (phase_depth.cpu().detach().numpy() ** 2)
        sink["rows"] = [s.item() for s in scalars] + [
            dd.mean().item(), (features_phasor[:, 0, 1] * SH_C0 + 0.5).mean().item(),
            (features_phasor[:, 0, 1][visibility_filter] * SH_C0 + 0.5).mean().item(), sp.mean(), sp_tof.mean(), gsp.mean(),
            np.abs(gsp - sp).mean(), np.abs(gsp - sp_tof).mean(), float(torch.abs(depth - gt_depth).mean()),
            float(torch.abs(phase_depth - gt_phase_depth).mean()), np.abs(amp - gt_amp).mean()]

    log = tof.TrainLog(slots=256)

    def record():
        log.record(phasor, depth, gt_phasor, depth_range, phase_offset, gt_depth=gt_depth, depth_distortion=dd,
                   visible=radii, extras=scalars, **coefficients)

    # the two routes compute the same thing
    eager()
    record()
    rows, _ = log.drain(wait=True)
    names = ("dd", "gs_sp", "gs_sp_visible", "sp", "sp_tof", "gsp", "sp_err", "sp_tof_err", "depth_err", "tof_depth_err", "amp_err")
    agree = {n: dict(eager=float(sink["rows"][5 + k]), record=float(rows[n][-1])) for k, n in enumerate(names)}
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            record()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            record()
    torch.cuda.current_stream().wait_stream(side)
    result = dict(device=torch.cuda.get_device_name(0), shape=args.shape, P=P, H=H, W=W, visible_rows=int((radii > 0).sum()),
                  coefficients=args.coefficients, seconds=args.seconds, windows=ROUNDS, agreement=agree,
                  **alternate(dict(eager=eager, record=record, record_graph=graph.replay), args.seconds))
    text = json.dumps(result, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
