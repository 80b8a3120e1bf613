"""A view's evaluation metrics (train.py:535-566): the reference's eager statements, with their two .item() reads, against
gftorf_amd.metrics.EvalReport.add_view, timed against each other in one process, per view.

    eager           the statements as train.py writes them: l1_loss and psnr of the colour image, l1_loss, l2_loss and psnr of
                    three ToF channels, depth_from_tof_torch with .item()s of depth_range and the offset, l1_loss / l2_loss of
                    the depth, l2_loss of the ToF depth, and the eight `+= x.mean().double()`
    add_view        report.add_view(...) eagerly: two launches, nothing read on the host
    add_view_graph  the same call replayed from a graph (the eager statements cannot be captured: they read the host)

at 320x240 and at 640x480, colour and ToF images of the same size.  Windows of views after a warm-up, the routes alternating
window by window, a few hundred views per route in all; per window the wall time (host clock from the first call to the end of a
synchronize) and the GPU time (device events around the same calls), both divided by the window's views; the medians over the
windows are reported.  (The eager route blocks on the host in every view, so its two times are nearly the same; add_view is
bound by its enqueue, the replayed graph by the device.)

    timeout 300 python profiles/bench_metrics.py --out profiles/metrics_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROUNDS = 7
SHAPES = {"320x240": (240, 320), "640x480": (480, 640)}


def alternate(routes, views):
    """routes: name -> callable that enqueues ONE view.  Returns name -> dict(wall_us, gpu_us, ..., views, windows)."""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for fn in routes.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    wall, gpu = {name: [] for name in routes}, {name: [] for name in routes}
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            a, b = ev(), ev()
            t0 = time.perf_counter()
            a.record()
            for _ in range(views):
                fn()
            b.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e6 / views)
            gpu[name].append(a.elapsed_time(b) * 1e3 / views)
    return {name: dict(wall_us=statistics.median(wall[name]), wall_min_us=min(wall[name]), wall_max_us=max(wall[name]),
                       gpu_us=statistics.median(gpu[name]), gpu_min_us=min(gpu[name]), gpu_max_us=max(gpu[name]),
                       views=views * ROUNDS, windows=ROUNDS) for name in routes}


def eager_tof_depth(planes, depth_range, offset):
    """The eager launches of the reference's ToF depth (scene/torf_utils.py:59-64) in the same order."""
    re, im = planes[0], planes[1]
    near_zero = torch.abs(re) < 1e-6
    safe_re = torch.where(near_zero, torch.full_like(re, 1e-6), re)
    angle = torch.atan2(im, safe_re)
    angle.sub_(offset)
    negative = angle < 0
    angle = torch.where(negative, angle + 2 * torch.pi, angle)
    return angle * depth_range / (4 * torch.pi)


def eager_l1(a, b):
    return torch.abs(a - b).mean()


def eager_l2(a, b):
    return ((a - b) ** 2).mean()


def eager_psnr(a, b):
    per_channel = ((a - b) ** 2).view(a.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(per_channel))


def bench_shape(H, W, views):
    from gftorf_amd import metrics
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    image = torch.rand(3, H, W, device=dev)
    gt_image = (image + 0.05 * torch.randn_like(image)).clamp(0, 1)
    phasor = torch.randn(7, H, W, device=dev)
    gt_phasor = phasor[:3] + 0.05 * torch.randn(3, H, W, device=dev)
    depth = torch.empty(1, H, W, device=dev).uniform_(0.3, 5.0)
    gt_depth = depth + 0.2 * torch.randn_like(depth)
    depth_range, phase_offset = torch.tensor([10.0], device=dev), torch.tensor([0.1], device=dev)
    sums = {}

    def eager():
        if not sums:
            sums.update(dict.fromkeys(metrics.VALUES, 0.0))
        sums["l1"] += eager_l1(image, gt_image).mean().double()
        sums["psnr"] += eager_psnr(image, gt_image).mean().double()
        tof_gt, tof_rendered = gt_phasor[:3], phasor[:3]
        sums["l1_p"] += eager_l1(tof_rendered, tof_gt).mean().double()
        sums["l2_p"] += eager_l2(tof_rendered, tof_gt).mean().double()
        sums["psnr_p"] += eager_psnr(tof_rendered, tof_gt).mean().double()
        depth_tof = eager_tof_depth(phasor, depth_range.item(), phase_offset.detach().cpu().numpy().item()).unsqueeze(0)
        sums["l1_d"] += eager_l1(depth, gt_depth).mean().double()
        sums["l2_d"] += eager_l2(depth, gt_depth).mean().double()
        sums["l2_d_tof"] += eager_l2(depth_tof, gt_depth).mean().double()

    report = metrics.EvalReport(device=dev)

    def add_view():
        report.add_view(image=image, gt_image=gt_image, tof=phasor[:3], gt_tof=gt_phasor, depth=depth, gt_depth=gt_depth, phasor=phasor,
                        depth_range=depth_range, phase_offset=phase_offset)

    # the two routes compute the same thing
    eager()
    add_view()
    res = report.result()
    agree = {n: dict(eager=float(sums[n]), add_view=res[n]) for n in metrics.VALUES}
    sums.clear()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            add_view()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            add_view()
    torch.cuda.current_stream().wait_stream(side)
    return dict(H=H, W=W, agreement=agree, **alternate(dict(eager=eager, add_view=add_view, add_view_graph=graph.replay), views))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=50, help="views per window; %d windows per route" % ROUNDS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_metrics.py needs a HIP device: there is nothing to time without one")
    result = dict(device=torch.cuda.get_device_name(0), views_per_window=args.views, windows=ROUNDS,
                  shapes={name: bench_shape(H, W, args.views) for name, (H, W) in SHAPES.items()})
    text = json.dumps(result, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
