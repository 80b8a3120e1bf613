"""gftorf_amd.rigid against the reference's statements (utils/loss_utils.py:35-72) run by torch on the device, in one process.

  knn      find_knn(xyz, 20) at 20 k, 100 k and 1 M points of an SfM-like cloud (dense blobs and a sparse background), and at
           20 k points the reference-shaped route, topk of torch.cdist(xyz, xyz) -- a 1.6 GB matrix, the largest size it can
           reasonably run at -- with how many of its rows are the exact table
  losses   forward + backward of rigidity_loss + isometry_loss at 100 k x 20:
             eager        the reference's statements
             fused        rigid.rigid_terms
             fused_graph  the same, replayed from a graph
           every route ends in the gradients of curr_xyz and prev_xyz.  The reference's statements are NOT replayed from a
           graph: a captured copy of them faulted on the MI355X at this size (illegal memory access in the replays).  Their
           backward is index_put with accumulate, which sorts the 2 M indices with the vendor library's radix sort; that sort
           clears its counters with hipMemsetAsync, and a memset node replays garbage on this platform from the second replay
           on (README, platform findings) -- the reading that fits, not confirmed beyond that.  gftorf_amd.rigid issues no
           memset, sorts nothing per iteration and is captured here and in tests/test_rigid.py.

Device events around windows of many iterations after a warm-up, the routes alternating window by window; the median window
is reported.  No kernel times under a profiler are taken: the figures are whole calls as a training loop would issue them.

    timeout 600 python profiles/bench_rigid.py --out profiles/rigid_bench.json
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
K = 20


def alternate(routes, seconds, warm=5, probe=10):
    """routes: name -> callable that enqueues ONE iteration.  Returns name -> dict(ms, min_ms, max_ms, iters, windows)."""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    iters = {}
    for name, fn in routes.items():
        for _ in range(warm):
            fn()
        a, b = ev(), ev()
        a.record()
        for _ in range(probe):
            fn()
        b.record()
        torch.cuda.synchronize()
        per = max(a.elapsed_time(b) / probe, 1e-3)
        iters[name] = max(3, int(seconds * 1e3 / ROUNDS / per) + 1)
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


def cloud(P, dev, seed=0):
    """dense blobs + sparse background, centred at the origin (where cdist is at its best)"""
    rng = np.random.default_rng(seed)
    c = rng.normal(0, 3, (8, 3))
    pts = c[rng.integers(0, 8, P)] + rng.normal(0, 0.05, (P, 3))
    pts[: P // 10] = rng.uniform(-10, 10, (P // 10, 3))
    return torch.tensor((pts - pts.mean(axis=0)).astype(np.float32), device=dev)


def reference_find_knn(xyz, k):
    dist = torch.cdist(xyz, xyz, p=2)
    return torch.topk(dist, k + 1, dim=-1, largest=False)[1][:, 1:]


def statements(prev, curr, idx, w, d0):
    k = idx.shape[1]
    curr_knn_pos, prev_knn_pos = curr[idx], prev[idx]
    curr_rep, prev_rep = curr.unsqueeze(1).expand(-1, k, -1), prev.unsqueeze(1).expand(-1, k, -1)
    rig = (w * torch.sqrt((((prev_rep - prev_knn_pos) - (curr_rep - curr_knn_pos)) ** 2).sum(dim=-1) + 1e-16)).mean()
    iso = (w * (torch.sqrt(d0 + 1e-16) - torch.sqrt(((curr_rep - curr_knn_pos) ** 2).sum(dim=-1) + 1e-16))).abs().mean()
    return rig, iso


def capture(fn, clear):
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
        clear()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rigid.py needs a HIP device: there is nothing to time without one")
    from gftorf_amd import rigid
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), K=K, seconds=args.seconds, windows=ROUNDS,
                  profiler="none: whole calls timed with device events, no kernel times under a profiler were taken")

    def save():
        text = json.dumps(result, indent=1, sort_keys=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return text

    knn = {}
    small = cloud(20_000, dev)
    exact, found = rigid.find_knn(small, K), reference_find_knn(small, K)
    knn["P20000"] = alternate(dict(find_knn=lambda: rigid.find_knn(small, K), cdist_topk=lambda: reference_find_knn(small, K)), args.seconds)
    knn["P20000"]["cdist_topk_rows_exact"] = int((found == exact).all(dim=1).sum())
    knn["P20000"]["cdist_topk_rows_with_self"] = int((found == torch.arange(20_000, device=dev)[:, None]).any(dim=1).sum())
    del found
    for P in (100_000, 1_000_000):
        xyz = cloud(P, dev)
        knn["P%d" % P] = alternate(dict(find_knn=lambda: rigid.find_knn(xyz, K)), args.seconds)
    result["knn"] = knn
    save()                                                     # (the neighbour figures stand on their own)

    P = 100_000
    prev = cloud(P, dev).requires_grad_()
    curr = (prev.detach() + 0.01 * torch.randn(P, 3, device=dev)).requires_grad_()
    nb = rigid.Neighbours.build(prev.detach(), K)
    idx = nb.idx.long()
    d0 = nb.dist2
    w = torch.exp(-d0 / d0.median())
    lam = (4.0, 2.0)

    def clear():
        prev.grad = curr.grad = None

    def eager():
        clear()
        rig, iso = statements(prev, curr, idx, w, d0)
        loss = lam[0] * rig + lam[1] * iso
        loss.backward()
        return loss.detach()

    def fused():
        clear()
        loss = rigid.rigid_terms(prev, curr, nb, w, d0, *lam)[0]
        loss.backward()
        return loss.detach()

    le = eager()
    ge = (curr.grad.clone(), prev.grad.clone())
    lf = fused()
    result["losses"] = dict(P=P, max_in_degree=int(nb.in_degree.max()), agreement=dict(
        loss_eager=float(le), loss_fused=float(lf), g_curr_max_abs_diff=float((curr.grad - ge[0]).abs().max()),
        g_prev_max_abs_diff=float((prev.grad - ge[1]).abs().max()), g_curr_max_abs=float(ge[0].abs().max()),
        g_prev_max_abs=float(ge[1].abs().max())))
    g_fused = capture(fused, clear)
    result["losses"].update(alternate(dict(eager=eager, fused=fused, fused_graph=g_fused.replay), args.seconds, warm=20, probe=50))
    print(save())


if __name__ == "__main__":
    main()
