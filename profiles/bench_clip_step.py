"""Gradient-norm clip + Adam step (train.py:468-472): the three routes, timed against each other in one process.

    torch_clip_step   torch.nn.utils.clip_grad_norm_(params, 1.0); FusedAdam.step()      (the only route before this feature)
    gft_clip_step     gftorf_amd.clip_grad_norm_(params, 1.0);     FusedAdam.step()
    fused_step        FusedAdam.step(max_grad_norm=1.0)

on (a) the reference network's 24 gradient tensors as a real DeformNetwork backward at --points points leaves them and (b) the
ten per-Gaussian tensors at --rows rows; each eagerly and replayed from a graph (capturable optimizer).  The first two routes
scale `.grad` in place, which would leave later iterations with nothing to clip, so EVERY route starts its iteration by
restoring the gradients from a saved copy (one copy kernel for the network's flat buffer, one _foreach_copy_ otherwise);
`restore_only` times that alone, and `net_ms` is a route's time less it.  Also: a captured step(visibility=...) at
--visible of --big-rows rows against the captured dense step.

Device events around windows of many iterations, the routes alternating window by window; a window is sized from a probe so
that every route is timed for --seconds in all.  Prints one JSON document (and writes it to --out).

    python profiles/bench_clip_step.py --out profiles/r07_clip_step.json
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

PER_GAUSSIAN = dict(xyz=(3,), f_dc_color=(1, 3), f_rest_color=(15, 3), phase_f_dc=(1, 1), phase_f_rest=(15, 1), amp_f_dc=(1, 1),
                    amp_f_rest=(15, 1), opacity=(1,), scaling=(3,), rotation=(4,))
LRS = dict(xyz=1.6e-4, f_dc_color=2.5e-3, f_rest_color=1.25e-4, phase_f_dc=1.6e-4, phase_f_rest=8e-6, amp_f_dc=1.6e-4, amp_f_rest=8e-6,
           opacity=0.05, scaling=1e-3, rotation=1e-3)


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


def capture(fn):
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def clip_routes(params, make_opt, seconds):
    """The three routes + restore_only over `params` (tensors with .grad), eager and captured."""
    import gftorf_amd
    grads = [p.grad for p in params if p.grad is not None]
    base = grads[0].untyped_storage().data_ptr()
    if all(g.untyped_storage().data_ptr() == base for g in grads):       # the network's backward: one flat buffer
        lo = min(g.storage_offset() for g in grads)
        hi = max(g.storage_offset() + g.numel() for g in grads)
        flat = torch.as_strided(grads[0], (hi - lo,), (1,), lo)
        saved = flat.clone()
        restore = lambda: flat.copy_(saved)
    else:
        saved = [g.clone() for g in grads]
        restore = lambda: torch._foreach_copy_(grads, saved)
    out = {}
    for mode in ("eager", "graph"):
        opts = {name: make_opt(mode == "graph") for name in ("torch_clip_step", "gft_clip_step", "fused_step")}

        def torch_clip_step(o=opts["torch_clip_step"]):
            restore()
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            o.step()

        def gft_clip_step(o=opts["gft_clip_step"]):
            restore()
            gftorf_amd.clip_grad_norm_(params, 1.0)
            o.step()

        def fused_step(o=opts["fused_step"]):
            restore()
            o.step(max_grad_norm=1.0)
        routes = dict(restore_only=restore, torch_clip_step=torch_clip_step, gft_clip_step=gft_clip_step, fused_step=fused_step)
        for fn in routes.values():
            fn()                                       # optimizer state and buffers exist before anything is captured
        torch.cuda.synchronize()
        if mode == "graph":
            graphs = {name: capture(fn) for name, fn in routes.items()}
            routes = {name: g.replay for name, g in graphs.items()}
        res = alternate(routes, seconds)
        for name, r in res.items():
            r["net_ms"] = r["ms"] - res["restore_only"]["ms"]
        out[mode] = res
    out["grad_norm"] = float(opts["fused_step"].last_grad_norm)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--big-rows", type=int, default=1_000_000)
    ap.add_argument("--visible", type=float, default=0.14)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_clip_step.py needs a HIP device: there is nothing to time without one")
    import gftorf_amd
    from gftorf_amd import FusedAdam
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    result = dict(device=torch.cuda.get_device_name(0), points=args.points, rows=args.rows, big_rows=args.big_rows,
                  visible=args.visible, seconds=args.seconds, windows=ROUNDS, max_norm=1.0)

    # ---- (a) the network's gradients after a real backward
    net = gftorf_amd.reference_network().to(dev)
    x, t = torch.randn(args.points, 3, device=dev), torch.rand(args.points, 1, device=dev)
    d_xyz, _, d_sh, _ = net(x, t, zeros_as_scalars=True)
    (d_xyz.sum() + d_sh.sum()).backward()
    params = list(net.parameters())
    n_grad = sum(p.grad.numel() for p in params if p.grad is not None)
    make = lambda cap: FusedAdam([{"params": params, "lr": 1e-5, "name": "deform"}], lr=0.0, eps=1e-15, capturable=cap)
    result["network"] = dict(tensors=sum(p.grad is not None for p in params), elements=n_grad, **clip_routes(params, make, args.seconds))
    del net, x, t, d_xyz, d_sh

    # ---- (b) the ten per-Gaussian tensors
    def gaussians(rows):
        par = {k: torch.nn.Parameter(torch.randn((rows,) + s, device=dev)) for k, s in PER_GAUSSIAN.items()}
        for p in par.values():
            p.grad = torch.randn_like(p)
        return par
    par = gaussians(args.rows)
    params = list(par.values())
    make = lambda cap: FusedAdam([{"params": [par[k]], "lr": LRS[k], "name": k} for k in par], lr=0.0, eps=1e-15, capturable=cap)
    result["gaussians"] = dict(tensors=len(params), elements=sum(p.numel() for p in params), **clip_routes(params, make, args.seconds))
    del par, params

    # ---- (c) the captured row-masked step against the captured dense one
    par = gaussians(args.big_rows)
    mask = torch.rand(args.big_rows, device=dev) < args.visible
    opts = [FusedAdam([{"params": [par[k]], "lr": LRS[k], "name": k} for k in par], lr=0.0, eps=1e-15, capturable=True) for _ in range(2)]
    opts[0].step(), opts[1].step(visibility=mask)
    graphs = dict(dense_step=capture(lambda: opts[0].step()), visible_step=capture(lambda: opts[1].step(visibility=mask)))
    result["captured_visibility"] = dict(rows=args.big_rows, visible_rows=int(mask.sum()),
                                         **alternate({k: g.replay for k, g in graphs.items()}, args.seconds))
    text = json.dumps(result, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
