"""What the reproducible mode (gftorf_amd.reproducible) costs, each workload timed three ways in one
process:

    default       float atomics (the switch off)
    serial        the switch on, the stored rows added by the one-workgroup comparator (GFT_DET_REDUCE=serial)
    grid          the switch on, the rows added by the grid-wide sum (csrc/k_detsum.hip; the mode's default)

    rasterizer_backward   the rasterizer's backward alone on the metric frame (1 M Gaussians, 640 x 480): one forward, then
                          backwards through it (retain_graph), device events around a window of them
    c3_flow_iteration     one C3-shaped iteration (bench_loop.build_loop: 100 k Gaussians, 320 x 240, the network on) followed by
                          the two scene-flow renders of an F-ToRF flow iteration on the same model (flow.render_flows) and
                          their backward

Windows of calls after a warm-up, the three ways alternating window by window; per window the wall time (host clock from the
first call to the end of a synchronize) and the GPU time (device events around the same calls), both divided by the window's
calls; the medians over the windows are reported.  No figure is judged here but one: `grid_not_slower_than_serial` says
whether, on the metric frame, the grid-wide sum was at most as slow as the serial one in this session -- the condition under
which it stays the mode's default.

    timeout 900 python profiles/bench_reproducible.py --out profiles/reproducible_bench.json
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

ROUNDS = 5
WAYS = ("default", "serial", "grid")


def set_way(way):
    from gftorf_amd import reproducible as R
    R.set_reproducible(way != "default")
    R._det_reduce = "serial" if way == "serial" else "grid"


def alternate(fn, calls, warmup=2):
    """fn: one call of the workload.  Returns way -> dict(wall_us, gpu_us, ...), the ways alternating window by window."""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for way in WAYS:
        set_way(way)
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    wall, gpu = {w: [] for w in WAYS}, {w: [] for w in WAYS}
    for _ in range(ROUNDS):
        for way in WAYS:
            set_way(way)
            a, b = ev(), ev()
            t0 = time.perf_counter()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            wall[way].append((time.perf_counter() - t0) * 1e6 / calls)
            gpu[way].append(a.elapsed_time(b) * 1e3 / calls)
    set_way("default")
    return {w: dict(wall_us=statistics.median(wall[w]), wall_min_us=min(wall[w]), wall_max_us=max(wall[w]),
                    gpu_us=statistics.median(gpu[w]), gpu_min_us=min(gpu[w]), gpu_max_us=max(gpu[w]),
                    calls=calls * ROUNDS, windows=ROUNDS) for w in WAYS}


def rasterizer_backward(dev, calls):
    from gftorf_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib, api, synth
    api.keep_last_buffers = True               # (for the frame's binning capacity: what the mode's buffers are sized by)
    scene = synth.make_scene("metric")
    cfg, cam, g = scene["cfg"], scene["cam"], scene["gaussians"]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    leaf = {k: t(v).requires_grad_() for k, v in g.items() if v is not None}
    means2D = torch.zeros((cfg["P"], 3), device=dev, requires_grad=True)
    settings = GaussianRasterizationSettings(
        image_height=cfg["H"], image_width=cfg["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=t(scene["bg"]),
        scale_modifier=1.0, viewmatrix=t(cam["viewmatrix"]), projmatrix=t(cam["projmatrix"]), sh_degree=cfg["D"],
        campos=t(cam["campos"]), prefiltered=False, debug=False, near_n=cam["znear"], far_n=cam["zfar"],
        depth_range=scene["depth_range"], use_view_dependent_phase=True)
    out = GaussianRasterizer(raster_settings=settings)(
        means3D=leaf["means3D"], means2D=means2D, opacities=leaf["opacities"], shs=leaf["shs"], shs_p=leaf["shs_p"],
        scales=leaf["scales"], rotations=leaf["rotations"], phase_offset=scene["phase_offset"], dc_offset=scene["dc_offset"])
    names = ("color", "phasor", "depth", "normal", "acc", "entropy", "depth_distortion")
    loss = sum((out[names.index(k)] * t(scene["grads"][k])).sum() for k in ("color", "phasor", "depth", "acc", "depth_distortion"))
    tensors = list(leaf.values()) + [means2D]

    def backward():
        for x in tensors:
            x.grad = None
        loss.backward(retain_graph=True)

    res = alternate(backward, calls)
    cap = int(api.last_call_buffers.get("cap", 0))
    api.keep_last_buffers = False
    api.last_call_buffers.clear()
    lib = _lib.load()
    mem = dict(binning_instances=cap,
               rasterizer_rows_bytes=int(lib.gft_det_partials_bytes(cap, cfg["W"], cfg["H"])) if cap else None,
               index_bytes=int(lib.gft_detsum_index_bytes(cfg["P"], cap)) if cap else None)
    return dict(workload="metric frame: P=%d %dx%d, backward alone" % (cfg["P"], cfg["W"], cfg["H"]), ways=res, memory=mem)


def c3_flow_iteration(dev, calls):
    import bench_loop
    from gftorf_amd import GaussianRasterizationSettings, flow
    cfg = bench_loop.C3
    iteration, info = bench_loop.build_loop(dev, cfg)
    par, cams = info["par"], info["frame"]["cams"]
    P, W, H = cfg["P"], cfg["W"], cfg["H"]
    cam = cams[0][1]
    settings = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=torch.zeros((7, H, W), device=dev),
        scale_modifier=1.0, viewmatrix=cam["_view"], projmatrix=cam["_proj"], sh_degree=3, campos=cam["_campos"], prefiltered=False,
        debug=False, near_n=cam["znear"], far_n=cam["zfar"], depth_range=cfg["depth_range"], use_view_dependent_phase=True)
    gen = torch.Generator().manual_seed(7)
    fa, fb = ((0.02 * torch.randn((P, 3), generator=gen)).to(dev).requires_grad_() for _ in range(2))
    ga, gb = (torch.randn((3, H, W), generator=gen).to(dev) for _ in range(2))
    state = dict(it=cfg["warm_up"])

    def step():
        state["it"] += 1
        iteration(state["it"])
        with torch.no_grad():
            geo = (par["xyz"].detach(), torch.sigmoid(par["opacity"]), torch.exp(par["scaling"]),
                   torch.nn.functional.normalize(par["rotation"]))
        fa.grad = fb.grad = None
        ia, ib = flow.render_flows(settings, *geo, fa, fb)
        ((ia * ga).sum() + (ib * gb).sum()).backward()

    res = alternate(step, calls, warmup=3)
    return dict(workload="C3-shaped iteration (P=%d %dx%d, network on) + the two flow renders and their backward" % (P, W, H), ways=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", default=None, choices=("rasterizer_backward", "c3_flow_iteration"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reproducible.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), rounds=ROUNDS)
    if args.only in (None, "rasterizer_backward"):
        result["rasterizer_backward"] = r = rasterizer_backward(dev, args.calls)
        result["grid_not_slower_than_serial"] = r["ways"]["grid"]["gpu_us"] <= r["ways"]["serial"]["gpu_us"]
        torch.cuda.empty_cache()
    if args.only in (None, "c3_flow_iteration"):
        result["c3_flow_iteration"] = c3_flow_iteration(dev, args.calls)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
