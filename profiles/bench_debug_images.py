"""The debug images of one training iteration (the ToF branch of train.py:295-378) at 320x240 and 640x480: the reference-shaped
host route against gftorf_amd.present.debug_images with the sheet's pinned copy, timed against each other in one process.

    host_numpy          the reference's route: the block's twenty blocking `.cpu()` copies of float32 planes and its numpy
                        statements (normalize_im, normalize_im_gt, to8b, cm.magma), restated here; the three scattering-phase
                        arrays and their two errors are formed before the window, as train.py:194-200 leaves them
    debug_images        present.debug_images eagerly into a kept sheet, then the sheet's copy to pinned memory: two launches
                        and one copy, nothing read on the host before the window's synchronize
    debug_images_graph  the two launches captured once and replayed, then the same copy

Windows of calls after a warm-up, the routes alternating window by window; per window the wall time (host clock from the first
call to the end of a synchronize) and the GPU time (device events around the same calls), both divided by the window's calls;
the medians over the windows are reported.  `enqueue_us` is the host time of debug_images and the copy's enqueue alone, without
any synchronize: what the call holds the host for.  PNG encoding is the same work on either route and is not timed.  No figure
is judged here; the script prints what it measured.

    timeout 300 python profiles/bench_debug_images.py --out profiles/debug_images_bench.json
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
SIZES = ((240, 320), (480, 640))
DEPTH_RANGE, PHASE_OFFSET, MULT = 7.5, 0.3, 2.0
PERMUTATION, QUAD_INDEX = (1, 0, 3, 2), 1


def alternate(routes, calls):
    """routes: name -> callable that handles ONE iteration.  Returns name -> dict(wall_us, gpu_us, ..., calls, windows)."""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for fn in routes.values():
        for _ in range(3):
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


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def normalize(im, lo, hi):
    im = (im - lo) / (hi - lo)
    im[np.isnan(im)] = 0.
    return np.clip(im, 0, 1)


def selfnorm(im):
    return normalize(im, np.min(im), np.max(im))


def draw(rng, H, W):
    """one iteration's tensors as numpy float32, a rendered view near its ground truth, and the three training views"""
    f32 = np.float32
    views = []
    for _ in range(3):
        theta = rng.uniform(0.05, 2 * np.pi - 0.05, (H, W)) + PHASE_OFFSET
        length = rng.uniform(0.05, 1.0, (H, W))
        views.append(np.stack([length * np.cos(theta), length * np.sin(theta), rng.uniform(0.02, 0.3, (H, W))]).astype(f32))
    gt = views[0]
    gt_quad = rng.uniform(-1, 1, (4, H, W)).astype(f32)
    phasor = np.empty((7, H, W), f32)
    phasor[:2] = gt[:2] * (1 + 0.05 * rng.normal(size=(2, H, W))) / MULT
    phasor[2] = gt[2] / MULT * (1 + 0.1 * rng.normal(size=(H, W)))
    phasor[3:] = gt_quad[list(PERMUTATION)] + 0.1 * rng.normal(size=(4, H, W))
    gt_image = rng.uniform(0, 1, (3, H, W)).astype(f32)
    return dict(phasor=phasor, gt_phasor=gt, dd=rng.uniform(0, 0.2, (1, H, W)).astype(f32), gt_image=gt_image,
                image=(gt_image + 0.1 * rng.normal(size=(3, H, W))).astype(f32), gt_quad=gt_quad), views


def sequence_ranges(views):
    """train.py:57-64 on the host, once before training: (lo, hi) of gt_reals, gt_imags, gt_amps, gt_scattering_phases"""
    def red_blue(p):
        return np.stack([np.where(p <= 0, 0, p), np.zeros_like(p), -np.where(p >= 0, 0, p)], -1).astype(np.float32)

    def tof_depth(v):
        phase = np.arctan2(v[1], v[0]) - np.float32(PHASE_OFFSET)
        phase = np.where(phase < 0, phase + np.float32(2 * np.pi), phase)
        return phase * np.float32(DEPTH_RANGE) / np.float32(4 * np.pi)
    lists = ([red_blue(v[0]) for v in views], [red_blue(v[1]) for v in views], [v[2] for v in views], [v[2] * tof_depth(v) ** 2 for v in views])
    return np.array([f(seq) for seq in lists for f in (np.min, np.max)], np.float32)


def host_route(t, pre, ranges, zplanes, magma):
    """the block with its copies: `t` the device tensors, `pre` what train.py:194-200 formed earlier in the iteration"""
    cpu = lambda x: x.cpu().detach().numpy()
    znear, zfar = zplanes
    out = {}
    depth = cpu(t["depth"])[0]
    out["depth"] = to8b(magma(1 - (depth - znear) / (zfar - znear)))
    amp = cpu(t["phasor"][:3]).transpose(1, 2, 0)[:, :, 2] * np.float32(MULT)
    gt_amp = cpu(t["gt_phasor"]).transpose(1, 2, 0)[:, :, 2]
    amp_error = selfnorm(np.abs(gt_amp - amp))
    for k, (name, im, err) in enumerate((("amp", amp, amp_error), ("scattering_phase", pre["sp"], pre["sp_error"]),
                                         ("scattering_phase_tof_depth", pre["sp_tof"], pre["sp_tof_error"]))):
        out[name] = to8b(normalize(im, ranges[2 * k], ranges[2 * k + 1]))
        out[name + "_error"] = to8b(err)
    out["scattering_phase_gt"] = to8b(normalize(pre["gt_sp"], ranges[6], ranges[7]))
    out["depth_error"] = to8b(selfnorm(np.abs(cpu(t["gt_phase_depth"]) - depth)))
    out["phase_depth"] = to8b(magma(1 - (cpu(t["phase_depth"]) - znear) / (zfar - znear)))
    out["phase_depth_gt"] = to8b(magma(1 - (cpu(t["gt_phase_depth"]) - znear) / (zfar - znear)))
    out["phase_depth_error"] = to8b(selfnorm(np.abs(cpu(t["gt_phase_depth"]) - cpu(t["phase_depth"]))))
    image, gt_image = cpu(t["image"]).transpose(1, 2, 0), cpu(t["gt_image"]).transpose(1, 2, 0)
    out["color"], out["color_gt"], out["color_error"] = to8b(image), to8b(gt_image), to8b(np.abs(gt_image - image))
    out["dd"] = to8b(selfnorm(cpu(t["dd"])[0]))
    quad, quad_gt, quad_error = [], [], []
    for i in range(4):
        q = cpu(t["phasor"][3:][i])
        quad.append(to8b(np.abs(q)))
        if PERMUTATION[i] == QUAD_INDEX:
            quad_error.append(to8b(selfnorm(np.abs(q - cpu(t["gt_quad"][list(PERMUTATION)][i])))))
        else:
            quad_error.append(to8b(np.zeros_like(q)))
        quad_gt.append(to8b(np.abs(cpu(t["gt_quad"][list(PERMUTATION)][i]))))
    out["quad"], out["quad_gt"], out["quad_error"] = np.stack(quad), np.stack(quad_gt), np.stack(quad_error)
    return out


def measure(H, W, calls, magma, magma_name):
    from gftorf_amd import _lib, present, tof
    dev = torch.device("cuda:0")
    v, views = draw(np.random.default_rng(H), H, W)
    t = {k: torch.tensor(a, device=dev) for k, a in v.items()}
    t["phase_depth"] = tof.depth_from_tof(t["phasor"][:3], DEPTH_RANGE, PHASE_OFFSET)
    t["gt_phase_depth"] = tof.depth_from_tof(t["gt_phasor"], DEPTH_RANGE, PHASE_OFFSET)
    t["depth"] = (t["gt_phase_depth"] * (1 + 0.03 * torch.randn(H, W, device=dev)))[None].contiguous()
    ranges = sequence_ranges(views)
    zplanes = present.zplanes(DEPTH_RANGE)
    zp32 = tuple(np.float32(z) for z in zplanes)
    amp = v["phasor"][2] * np.float32(MULT)
    d, pd, gpd = (t[k].cpu().numpy().reshape(H, W) for k in ("depth", "phase_depth", "gt_phase_depth"))
    gt_sp = v["gt_phasor"][2] * gpd ** 2
    pre = dict(sp=amp * d ** 2, sp_tof=amp * pd ** 2, gt_sp=gt_sp)
    pre.update(sp_error=np.abs(gt_sp - pre["sp"]), sp_tof_error=np.abs(gt_sp - pre["sp_tof"]))

    total = present.debug_sheet_layout(H, W, 511)[0]
    sheet = torch.empty((total,), device=dev, dtype=torch.uint8)
    pinned = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
    partials = torch.empty((present.debug_blocks(H * W), _lib.DEBUGVIZ_PARTIAL_WORDS), device=dev, dtype=torch.float32)
    kw = dict(t, permutation=PERMUTATION, quad_index=QUAD_INDEX, ranges=torch.tensor(ranges, device=dev), zplanes=zplanes, tof_multiplier=MULT)
    launch = lambda: present.debug_images(out=sheet, _partials=partials, **kw)

    def eager():
        images = launch()
        pinned.copy_(sheet, non_blocking=True)
        return images

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()

    def replay():
        graph.replay()
        pinned.copy_(sheet, non_blocking=True)

    # the routes agree before they are timed
    host = host_route(t, pre, ranges, zp32, magma)
    got = {k: x.cpu().numpy() for k, x in eager().items()}
    differing = {k: float((got[k] != host[k]).mean()) for k in host}
    assert set(got) == set(host) and all(x < 1e-3 for x in differing.values()), differing
    res = alternate(dict(host_numpy=lambda: host_route(t, pre, ranges, zp32, magma), debug_images=eager, debug_images_graph=replay), calls)
    torch.cuda.synchronize()
    spans = []
    for _ in range(200):
        t0 = time.perf_counter()
        eager()
        spans.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    res["debug_images"]["enqueue_us"] = statistics.median(spans)
    res["host_numpy"]["bytes_to_host"] = 20 * 4 * H * W
    res["host_numpy"]["copies"] = 20
    res["debug_images"]["bytes_to_host"] = res["debug_images_graph"]["bytes_to_host"] = total
    return dict(size="%dx%d" % (W, H), sheet_bytes=total, sheet_bytes_per_pixel=total / (H * W), bytes_differing=differing, magma=magma_name,
                routes=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_debug_images.py needs a HIP device: nothing is measured without one")
    from gftorf_amd import present
    try:
        from matplotlib import cm
        magma, magma_name = cm.magma, "matplotlib cm.magma"
    except ImportError:                 # the map as a table lookup: cheaper than matplotlib's call, so the host route reads low
        table = present.magma_table().astype(np.float64) / 255

        def magma(x):
            row = np.where(np.isnan(x), 256, np.clip(np.trunc(np.nan_to_num(x) * 256), 0, 255)).astype(np.int64)
            return table[row]
        magma_name = "table lookup (no matplotlib)"
    result = dict(device=torch.cuda.get_device_name(0), numpy=np.__version__, sizes=[measure(H, W, args.calls, magma, magma_name) for H, W in SIZES])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
