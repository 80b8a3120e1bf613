"""The F-ToRF scene-flow term at the ftorf size (320x240), forward + backward, both directions: the reference's composition
in stock torch (train.py:243-259 with scene/torf_utils.py's operations: meshgrid, elementwise maths, cat, torch.inverse,
matmuls, the squared-error means) against gftorf_amd.flow.flow_loss, eager and captured in a graph (replays).  Device
events around each iteration after warm-up; prints the median, 10th and 90th percentile in microseconds as one JSON line
(and writes it to --out).

    python profiles/flow_loss_bench.py [--iters 300] [--warmup 30] [--fused-only] [--out FILE]

Run the fused leg alone under `rocprofv3 --kernel-trace --stats` for the kernel times."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np        # noqa: E402
import torch              # noqa: E402

from gftorf_amd import flow, synth      # noqa: E402


def camera(dev, H, W, seed):
    rng = np.random.default_rng(seed)
    f = 0.9 * W
    K = torch.tensor([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=torch.float32, device=dev)
    K_tof = torch.tensor([[0.95 * f, 0, W / 2 + 1.5], [0, 0.95 * f, H / 2 - 1.0], [0, 0, 1]], dtype=torch.float32, device=dev)
    a = rng.uniform(-0.1, 0.1, 3)
    w2c = synth.look_at_w2c(*a, t=rng.uniform(-0.2, 0.2, 3))
    w2c_tof = synth.look_at_w2c(*(a + 0.02), t=w2c[:3, 3] + np.array([0.05, 0.0, 0.0]))
    t = lambda m: torch.tensor(np.ascontiguousarray(m.T), device=dev)
    gen = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(fx=float(K[0, 0]), fy=float(K[1, 1]), cx=float(K[0, 2]), cy=float(K[1, 2]), K=K, K_tof=K_tof,
                                 world_view_transform=t(w2c), world_view_transform_tof=t(w2c_tof),
                                 forward_flow=(2 * torch.randn((2, H, W), generator=gen)).to(dev),
                                 backward_flow=(2 * torch.randn((2, H, W), generator=gen)).to(dev))


# the reference's operations, restated (scene/torf_utils.py:80-124)
def eager_points3d(distance_map, cam):
    H, W = distance_map.shape[1:]
    u, v = torch.meshgrid(torch.arange(W, device=distance_map.device), torch.arange(H, device=distance_map.device), indexing="xy")
    z = distance_map / torch.sqrt(((u - cam.cx) / cam.fx) ** 2 + ((v - cam.cy) / cam.fy) ** 2 + 1)
    x = (u - cam.cx) * z / cam.fx
    y = (v - cam.cy) * z / cam.fy
    p = torch.cat([x, y, z], dim=0).view(3, -1)
    p = torch.cat([p, torch.ones((1, H * W), device=p.device)], dim=0)
    return (torch.inverse(cam.world_view_transform) @ p)[:3, :].reshape(3, H, W)


def eager_project(p3, cam, flow3d=None):
    H, W = p3.shape[1:]
    p = p3.view(3, -1) if flow3d is None else p3.view(3, -1) + flow3d.view(3, -1)
    p = torch.cat([p, torch.ones((1, H * W), device=p.device)], dim=0)
    q = cam.K_tof @ (cam.world_view_transform_tof.transpose(1, 0) @ p)[:3, :]
    return (q[:2, :] / (q[2:, :] + 1e-7)).reshape(2, H, W)


def eager_iteration(depth, cam, ff, fb):
    p3 = eager_points3d(depth.detach(), cam)
    p2 = eager_project(p3, cam)
    lf = torch.square((eager_project(p3, cam, ff) - p2) - cam.forward_flow).mean()
    lb = torch.square((eager_project(p3, cam, fb) - p2) - cam.backward_flow).mean()
    (0.01 * (lf + lb)).backward()


def fused_iteration(depth, cam, ff, fb):
    lf, lb = flow.flow_loss(depth, cam, ff, fb)
    (0.01 * (lf + lb)).backward()


def captured(fn, args):
    """fn(*args) captured in a graph after a warm-up on a side stream; returns the graph's replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn(*args)
    return graph.replay


def time_it(fn, args, iters, warmup):
    for _ in range(warmup):
        fn(*args)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(*args)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    ts = np.array(ts)
    return {"median_us": round(float(np.median(ts)), 2), "p10_us": round(float(np.percentile(ts, 10)), 2),
            "p90_us": round(float(np.percentile(ts, 90)), 2), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_loss_bench.py needs a HIP device")
    dev = torch.device("cuda:0")
    H, W = 240, 320
    cam = camera(dev, H, W, 3)
    gen = torch.Generator().manual_seed(4)
    depth = (0.5 + 7.5 * torch.rand((1, H, W), generator=gen)).to(dev)
    ff = (0.1 * torch.randn((3, H, W), generator=gen)).to(dev).requires_grad_()
    fb = (0.1 * torch.randn((3, H, W), generator=gen)).to(dev).requires_grad_()
    res = {"size": [H, W], "device": torch.cuda.get_device_name(dev)}
    res["fused"] = time_it(fused_iteration, (depth, cam, ff, fb), a.iters, a.warmup)
    res["fused_graph_replay"] = time_it(captured(fused_iteration, (depth, cam, ff, fb)), (), a.iters, a.warmup)
    if not a.fused_only:
        res["eager"] = time_it(eager_iteration, (depth, cam, ff, fb), a.iters, a.warmup)
        ff.grad = fb.grad = None
        eager_iteration(depth, cam, ff, fb)
        ge = (ff.grad.clone(), fb.grad.clone())
        ff.grad = fb.grad = None
        fused_iteration(depth, cam, ff, fb)
        res["max_rel_grad_diff"] = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip((ff.grad, fb.grad), ge))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
