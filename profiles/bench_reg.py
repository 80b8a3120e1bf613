"""The four regularisers of the loss (train.py:237-240, 266-277): forward plus backward of the reference's eager statements
against gftorf_amd.reg.regularizers, timed against each other in one process.

    eager       the statements as train.py writes them: get_opacity[get_motion_mask], get_scaling[visibility_filter], the means
    fused       reg.regularizers(..., raw=True) on the model's raw tensors
    fused_graph the same call and its backward replayed from a graph (the eager statements cannot be captured: their
                boolean-mask selections read the row count on the host)

at P = 100 k Gaussians with a 320x240 distortion image and P = 1 M at 640x480, 30 % dynamic and 60 % visible rows.  Every
route ends in the gradients of d_xyz, _opacity, _scaling and the distortion image.  Device events around windows of many
iterations after a warm-up, the routes alternating window by window; the median window is reported.  One run per shape under
a time limit of its own:

    timeout 300 python profiles/bench_reg.py --shape small --out profiles/reg_bench_small.json
    timeout 300 python profiles/bench_reg.py --shape large --out profiles/reg_bench_large.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

ROUNDS = 7
SHAPES = {"small": (100_000, 240, 320), "large": (1_000_000, 480, 640)}
LAMBDAS = dict(mlp=0.01, oe=0.01, scale=1.0, dd=0.1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="small")
    ap.add_argument("--dynamic", type=float, default=0.3)
    ap.add_argument("--visible", type=float, default=0.6)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_reg.py needs a HIP device: there is nothing to time without one")
    from gftorf_amd import reg
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    P, H, W = SHAPES[args.shape]
    mask = torch.rand(P, device=dev) < args.dynamic
    radii = torch.where(torch.rand(P, device=dev) < args.visible, torch.randint(1, 40, (P,), device=dev), 0).to(torch.int32)
    n_dyn = int(mask.sum())
    leaves = dict(d_xyz=0.05 * torch.randn(n_dyn, 3, device=dev), opacity=torch.randn(P, 1, device=dev),
                  scaling=torch.log(torch.empty(P, 3, device=dev).uniform_(0.004, 0.3)), dd=torch.rand(1, H, W, device=dev))
    for t in leaves.values():
        t.requires_grad_()
    lam = LAMBDAS

    def clear():
        for t in leaves.values():
            t.grad = None

    def eager():
        clear()
        visibility_filter = radii > 0
        get_opacity, get_scaling = torch.sigmoid(leaves["opacity"]), torch.exp(leaves["scaling"])
        loss = lam["mlp"] * torch.abs(leaves["d_xyz"]).mean()
        loss = loss + lam["dd"] * leaves["dd"].mean()
        dynamic_opacities = get_opacity[mask]
        loss = loss + lam["oe"] * (-dynamic_opacities * torch.log(dynamic_opacities + 1e-10)
                                   - (1 - dynamic_opacities) * torch.log(1 - dynamic_opacities + 1e-10)).mean()
        vis_scales = get_scaling[visibility_filter]
        loss = loss + lam["scale"] * ((vis_scales.mean(dim=-1) ** 2).mean())
        loss.backward()
        return loss.detach()          # (a live autograd graph on the leaves would break the capture below: INTEGRATION K)

    def fused():
        clear()
        loss = reg.regularizers(d_xyz=leaves["d_xyz"], w_mlp=lam["mlp"], opacity=leaves["opacity"], motion_mask=mask, w_oe=lam["oe"],
                                scaling=leaves["scaling"], visible=radii, w_scale=lam["scale"], depth_distortion=leaves["dd"],
                                w_dd=lam["dd"], raw=True)
        loss.backward()
        return loss.detach()          # (a live autograd graph on the leaves would break the capture below: INTEGRATION K)

    # the two routes compute the same thing
    le = eager()
    ge = {k: t.grad.clone() for k, t in leaves.items()}
    lf = fused()
    agree = dict(loss_eager=float(le), loss_fused=float(lf),
                 grad_max_abs_diff={k: float((t.grad - ge[k]).abs().max()) for k, t in leaves.items()},
                 grad_max_abs={k: float(ge[k].abs().max()) for k in ge})
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fused()
        clear()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            fused()
    torch.cuda.current_stream().wait_stream(side)
    result = dict(device=torch.cuda.get_device_name(0), shape=args.shape, P=P, H=H, W=W, dynamic_rows=n_dyn,
                  visible_rows=int((radii > 0).sum()), seconds=args.seconds, windows=ROUNDS, agreement=agree,
                  **alternate(dict(eager=eager, fused=fused, fused_graph=graph.replay), args.seconds))
    text = json.dumps(result, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
