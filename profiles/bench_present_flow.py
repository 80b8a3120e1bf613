"""The optical-flow debug images of one direction (train.py:382-386) at 320x240, the debug block's frame: the reference-shaped
host route against gftorf_amd.present.flow_images, timed against each other in one process.

    host_numpy         the reference's route: the two blocking `.cpu()` copies of the rendered and the target flow, then
                       flow_to_image three times, restated here in numpy as numpy >= 2 evaluates it (float64 behind the
                       division), with the in-place edits of the arguments the later calls see
    flow_images        present.flow_images eagerly into a kept buffer: two launches, nothing read on the host (wall = the
                       enqueue plus the window's one synchronize; gpu = device events)
    flow_images_graph  the same call captured once and replayed: the device time of the two kernels

Windows of calls after a warm-up, the routes alternating window by window; per window the wall time (host clock from the first
call to the end of a synchronize) and the GPU time (device events around the same calls), both divided by the window's calls;
the medians over the windows are reported.  `enqueue_us` is the host time of flow_images alone, without any synchronize: what
the call holds the host for.  PNG encoding is the same work on either route and is not timed.

    timeout 300 python profiles/bench_present_flow.py --out profiles/present_flow_bench.json
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROUNDS = 7
H, W = 240, 320


def alternate(routes, calls):
    """routes: name -> callable that handles ONE direction.  Returns name -> dict(wall_us, gpu_us, ..., calls, windows)."""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for fn in routes.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    wall, gpu = {name: [] for name in routes}, {name: [] for name in routes}
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            a, b = ev(), ev()
            t0 = time.perf_counter()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e6 / calls)
            gpu[name].append(a.elapsed_time(b) * 1e3 / calls)
    return {name: dict(wall_us=statistics.median(wall[name]), wall_min_us=min(wall[name]), wall_max_us=max(wall[name]),
                       gpu_us=statistics.median(gpu[name]), gpu_min_us=min(gpu[name]), gpu_max_us=max(gpu[name]),
                       calls=calls * ROUNDS, windows=ROUNDS) for name in routes}


def colour(u, v, wheel):
    """compute_color of float64 u, v [H, W]"""
    nan = np.isnan(u) | np.isnan(v)
    u[nan] = 0
    v[nan] = 0
    rad = np.sqrt(u ** 2 + v ** 2)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * (len(wheel) - 1) + 1
    k0 = np.floor(fk).astype(int)
    k1 = k0 + 1
    k1[k1 == len(wheel) + 1] = 1
    f = fk - k0
    img = np.zeros(u.shape + (3,))
    for i in range(3):
        tmp = wheel[:, i]
        col = (1 - f) * (tmp[k0 - 1] / 255) + f * (tmp[k1 - 1] / 255)
        idx = rad <= 1
        col[idx] = 1 - rad[idx] * (1 - col[idx])
        col[~idx] *= 0.75
        img[:, :, i] = np.uint8(np.floor(255 * col * (1 - nan)))
    return img


def to_image(flow, gt, wheel):
    """flow_to_image(flow, gt) for [H, W, 2] float32 arrays, which it edits in place as the reference does"""
    u, v = flow[:, :, 0], flow[:, :, 1]
    unknown = (abs(u) > 200) | (abs(v) > 200)
    u[unknown] = 0
    v[unknown] = 0
    gu, gv = gt[..., 0], gt[..., 1]
    lost = (abs(gu) > 200) | (abs(gv) > 200)
    gu[lost] = 0
    gv[lost] = 0
    nan = np.isnan(gu) | np.isnan(gv)
    gu[nan] = 0
    gv[nan] = 0
    maxrad = np.max(np.sqrt(gu ** 2 + gv ** 2))
    maxrad *= 1.1
    den = maxrad + np.finfo(float).eps
    img = colour(u / den, v / den, wheel)
    img[np.repeat(unknown[:, :, None], 3, axis=2)] = 0
    return np.uint8(img)


def host_route(flow, gt_flow, wheel):
    """train.py:382-386 with its copies"""
    r = flow.cpu().detach().numpy().transpose(1, 2, 0)
    t = gt_flow.cpu().detach().numpy().transpose(1, 2, 0)
    return dict(flow=to_image(r, t, wheel), gt=to_image(t, t, wheel), error=to_image(t - r, t, wheel))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_present_flow.py needs a HIP device: nothing is measured without one")
    from gftorf_amd import present
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    gt_np = (3.0 * rng.normal(size=(2, H, W))).astype(np.float32)
    flow_np = np.concatenate([gt_np + (0.3 * rng.normal(size=(2, H, W))).astype(np.float32), np.zeros((1, H, W), np.float32)])
    gt_np[:, 5, 7], flow_np[:2, 9, 11] = np.nan, 250.0
    flow, gt_flow = torch.tensor(flow_np, device=dev), torch.tensor(gt_np, device=dev)         # render_flow's 3 planes; the target
    wheel = present.flow_wheel().astype(np.float64)
    out = torch.empty((3, H, W, 3), device=dev, dtype=torch.uint8)
    partials = torch.empty((present.flow_blocks(H * W) + 1,), device=dev, dtype=torch.float32)
    eager = lambda: present.flow_images(flow, gt_flow, out=out, _partials=partials)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eager()

    # the routes agree before they are timed (up to arctan2's last bits: a byte may differ by one at a rare pixel)
    host = host_route(flow[:2], gt_flow, wheel)
    got = {k: x.cpu().numpy() for k, x in eager().items()}
    differing = {k: float((got[k] != host[k]).any(-1).mean()) for k in host}
    assert all(np.abs(got[k].astype(int) - host[k].astype(int)).max() <= 1 and differing[k] < 1e-3 for k in host), differing
    res = alternate(dict(host_numpy=lambda: host_route(flow[:2], gt_flow, wheel), flow_images=eager, flow_images_graph=graph.replay),
                    args.calls)
    torch.cuda.synchronize()
    spans = []
    for _ in range(200):
        t0 = time.perf_counter()
        eager()
        spans.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    res["flow_images"]["enqueue_us"] = statistics.median(spans)
    res["host_numpy"]["bytes_to_host"] = 4 * H * W * 4
    res["flow_images"]["bytes_to_host"] = res["flow_images_graph"]["bytes_to_host"] = 0
    result = dict(device=torch.cuda.get_device_name(0), size="%dx%d" % (W, H), numpy=np.__version__, pixels_differing=differing, routes=res)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
