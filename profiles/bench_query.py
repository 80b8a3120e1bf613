"""The deformation queries of an F-ToRF iteration (train.py:169-176, 248, 255): forward plus backward of the batched call
gftorf_amd.query against the unfused route it replaces, timed against each other in one process.

    unfused        K DeformNetwork calls on a pre-gathered x (gftorf_amd/frames.py:48-49), each with its time as a device
                   scalar expanded over the points, torch's lerp / differences (train.py:176, 249, 256), autograd's sums of
                   the K parameter gradients
    fused          DeformQuery.plan: one input kernel, one network call over K * n rows, one combine node
    *_graph        the same iteration replayed from a graph (times and coefficients in device memory)

Two shapes: `flow` (n = 30 k dynamic Gaussians, K = 3, the flow matrix) and `lerp` (n = 300 k, K = 2, frame curr + 1).  The
upstream gradients are non-zero on 10 % of the rows (the Gaussians a pixel blended), as in training.  Every route ends in the
network's parameter gradients.  Device events around windows of many iterations after a warm-up, the routes alternating
window by window; the median window is reported, with the launches of one eager iteration (torch.profiler's device events).
One run per shape under a time limit of its own:

    timeout 300 python profiles/bench_query.py --shape flow --out profiles/query_bench.json
    timeout 300 python profiles/bench_query.py --shape lerp --out profiles/query_bench.json
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
FLOW = [[1.0, 0.0, 0.0], [-1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]]
# n, dynamic share, times, matrix
SHAPES = {"flow": (30_000, 0.3, [4 / 11, 8 / 11, 0.0], FLOW), "lerp": (300_000, 0.3, [4 / 11, 8 / 11], [[0.75, 0.25]])}


def alternate(routes, seconds):
    """routes: name -> callable that enqueues ONE iteration.  Returns name -> dict(ms, min_ms, max_ms, iters, windows)."""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    iters = {}
    for name, fn in routes.items():
        for _ in range(10):
            fn()
        a, b = ev(), ev()
        a.record()
        for _ in range(10):
            fn()
        b.record()
        torch.cuda.synchronize()
        per = max(a.elapsed_time(b) / 10, 1e-3)
        iters[name] = max(5, int(seconds * 1e3 / ROUNDS / per) + 1)
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


def launches(fn):
    """Device-side events (kernels, copies, fills) of one iteration, or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
        count = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return count / 3.0 if count else None
    except Exception as e:          # the timing does not depend on it
        print("launch count unavailable: %s" % e, file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="flow")
    ap.add_argument("--rows-with-gradient", type=float, default=0.1)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_query.py needs a HIP device: there is nothing to time without one")
    from gftorf_amd import DeformQuery, reference_network, synth
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n_want, share, times, matrix = SHAPES[args.shape]
    K, M = len(times), len(matrix)
    P = int(n_want / share)
    extent = 3.7
    xyz = (torch.rand(P, 3, device=dev) * 2 - 0.5) * extent
    mask = torch.zeros(P, dtype=torch.bool, device=dev)
    mask[torch.randperm(P, device=dev)[:n_want]] = True
    q = DeformQuery(mask)
    n = q.n
    nets = {}
    for route in ("unfused", "fused"):                 # a network each: the share of rows the last backward used is per network
        net = reference_network()
        net.load_state_dict({k: torch.tensor(v) for k, v in synth.random_deform_params(7).items()})
        nets[route] = net.to(dev)
    gs = []
    for _ in range(M):
        keep = torch.rand(n, device=dev) < args.rows_with_gradient
        gs.append(torch.randn(n, 3, device=dev) * keep[:, None])
    times_dev = torch.tensor(times, dtype=torch.float32, device=dev)
    matrix_dev = torch.tensor(matrix, dtype=torch.float32, device=dev)
    x_norm = (xyz / extent)[mask].contiguous()         # the pre-gathered stand-in of frames.py:48-49

    def unfused():
        net = nets["unfused"]
        net.zero_grad(set_to_none=True)
        d = [net(x_norm, times_dev[k:k + 1].view(1, 1).expand(n, -1), zeros_as_scalars=True)[0] for k in range(K)]
        if M == 1:              # train.py:176 on frame curr + 1
            outs = [0.25 * (1 * d[1] + 3 * d[0])]
        else:                   # train.py:173, 249, 256
            outs = [d[0], d[1] - d[0], d[2] - d[0]]
        torch.autograd.backward(outs, gs)
        return [o.detach() for o in outs]

    def fused():
        net = nets["fused"]
        net.zero_grad(set_to_none=True)
        outs, _ = q.plan(net, xyz, extent, times_dev, matrix_dev)
        torch.autograd.backward(list(outs), gs)
        return [o.detach() for o in outs]

    # the two routes compute the same thing
    ou, of = unfused(), fused()
    named = lambda net: {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    gu, gf = named(nets["unfused"]), named(nets["fused"])
    agree = dict(outputs_bit_equal=all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(ou, of)),
                 grad_max_rel_diff=max(float((gf[k] - gu[k]).abs().max() / gu[k].abs().max().clamp_min(1e-30)) for k in gf),
                 params_with_grad=dict(unfused=len(gu), fused=len(gf)))
    routes = dict(unfused=unfused, fused=fused)
    counts = {name: launches(fn) for name, fn in routes.items()}
    graphs = {}
    for name, fn in list(routes.items()):
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
            nets[name].zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=side):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        graphs[name] = graph
        routes[name + "_graph"] = graph.replay
    timed = alternate(routes, args.seconds)
    for name, c in counts.items():
        timed[name]["launches"] = c
    result = dict(device=torch.cuda.get_device_name(0), shape=args.shape, P=P, n=n, K=K, M=M, rows=K * n, times=times, matrix=matrix,
                  rows_with_gradient=args.rows_with_gradient, seconds=args.seconds, windows=ROUNDS, agreement=agree, **timed)
    result["speedup_eager"] = timed["unfused"]["ms"] / timed["fused"]["ms"]
    result["speedup_graph"] = timed["unfused_graph"]["ms"] / timed["fused_graph"]["ms"]
    print(json.dumps(result, indent=1, sort_keys=True))
    if args.out:                    # one file for both shapes: {shape: result}
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        both = json.load(open(args.out)) if os.path.exists(args.out) else {}
        both[args.shape] = result
        with open(args.out, "w") as f:
            f.write(json.dumps(both, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
