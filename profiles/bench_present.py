"""A rendered view's display images (render.py:129-184): the reference's statements on host copies against
gftorf_amd.present, timed against each other in one process, per 640x480 view with every group (colour, a 7-plane phasor,
depth, acc, dd).

    host_numpy    the reference's route: the blocking `.cpu()` copies of the rasterizer's float32 outputs, then the statements
                  in numpy float32 (phasor2real_img_amp, normalize_im_gt, depth_from_tof, depth / acc, the magma colour map,
                  normalize_im, to8b), restated here; the colour map is matplotlib's cm.magma when matplotlib is there, else a
                  lookup in the kernel's table (the result says which)
    view_images   present.view_images eagerly into a kept sheet: two launches, nothing read on the host (wall = the enqueue
                  plus the window's one synchronize; gpu = device events)
    view_images_graph  the same call captured once and replayed: the device time of the two kernels
    view_sheets   ViewSheets end to end: submit (the two launches, the sheet's asynchronous copy to pinned memory, an event)
                  and ready(wait=True) per view, i.e. until the uint8 images are numpy arrays on the host

Windows of views after a warm-up, the routes alternating window by window; per window the wall time (host clock from the first
call to the end of a synchronize) and the GPU time (device events around the same calls), both divided by the window's views;
the medians over the windows are reported, with the bytes per view each route brings to the host.  PNG encoding is the same
work on either route and is not timed.

    timeout 300 python profiles/bench_present.py --out profiles/present_bench.json
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
H, W = 480, 640


def alternate(routes, views):
    """routes: name -> callable that handles ONE view.  Returns name -> dict(wall_us, gpu_us, ..., views, windows)."""
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
            for _ in range(views):
                fn()
            b.record()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e6 / views)
            gpu[name].append(a.elapsed_time(b) * 1e3 / views)
    return {name: dict(wall_us=statistics.median(wall[name]), wall_min_us=min(wall[name]), wall_max_us=max(wall[name]),
                       gpu_us=statistics.median(gpu[name]), gpu_min_us=min(gpu[name]), gpu_max_us=max(gpu[name]),
                       views=views * ROUNDS, windows=ROUNDS) for name in routes}


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def normalize(im, lo, hi):
    im = (im - lo) / (hi - lo)
    im[np.isnan(im)] = 0.
    return np.clip(im, 0, 1)


def red_blue(plane):
    out = np.tile(plane[:, :, None], (1, 1, 3))
    out[:, :, 0][out[:, :, 0] <= 0] = 0.0
    out[:, :, 2][out[:, :, 2] >= 0] = 0.0
    out[:, :, 2] = -out[:, :, 2]
    out[:, :, 1] = 0.0
    return out


def host_route(t, ranges, znear, zfar, depth_range, phase_offset, mult, magma):
    """render.py:129-184 with its copies, one per use as the reference makes them"""
    cpu = lambda x: x.cpu().detach().numpy()
    out = {}
    ph = cpu(t["phasor"]).transpose(1, 2, 0) * mult
    for k, (name, im) in enumerate((("real", red_blue(ph[:, :, 0])), ("imag", red_blue(ph[:, :, 1])), ("amp", ph[:, :, 2]))):
        out[name] = to8b(normalize(im, ranges[2 * k], ranges[2 * k + 1]))
    tof = cpu(t["phasor"]).transpose(1, 2, 0)                                                  # the saved .npy
    out["quad"] = [to8b(np.abs(cpu(t["phasor"][3:][k]))) for k in range(4)]
    hwc = cpu(t["phasor"]).transpose(1, 2, 0)
    phase = np.arctan2(hwc[..., 1:2], hwc[..., 0:1])
    phase -= phase_offset
    phase[phase < 0] = phase[phase < 0] + 2 * np.pi
    depth_tof = (phase * depth_range / (4 * np.pi))[:, :, 0]
    out["depth_tof"] = magma(1 - (depth_tof - znear) / (zfar - znear))
    depth = cpu(t["depth"])[0]
    out["depth"] = magma(1 - (depth - znear) / (zfar - znear))
    depth_norm = cpu(t["depth"])[0] / cpu(t["acc"])[0]
    out["depth_norm"] = magma(1 - (depth_norm - znear) / (zfar - znear))
    depth_norm_tof_cam = cpu(t["depth"])[0] / cpu(t["acc"])[0]                                 # the ToF-camera pass's copies
    out["color"] = to8b(cpu(t["image"]).transpose(1, 2, 0))
    dd = cpu(t["dd"])[0]
    out["dd"] = to8b(normalize(dd, np.min(dd), np.max(dd)))
    return out, tof, depth_norm_tof_cam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--views", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_present.py needs a HIP device: nothing is measured without one")
    from gftorf_amd import present
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    depth_range, phase_offset, mult = np.float32(7.5), 0.3, 2.0
    znear, zfar = 0.05 * depth_range * 0.9, 0.55 * depth_range * 1.1
    up = lambda a: torch.tensor(a.astype(np.float32), device=dev)
    t = dict(image=up(rng.uniform(0, 1, (3, H, W))), phasor=up(rng.uniform(-1, 1, (7, H, W))), depth=up(rng.uniform(0.3, 4, (1, H, W))),
             acc=up(rng.uniform(0.2, 1, (1, H, W))), dd=up(rng.uniform(0, 3, (1, H, W))))
    ranges = np.array([0, 1.6, 0, 1.6, 0.1, 1.8], np.float32)
    table = present.magma_table()
    try:
        from matplotlib import cm
        magma, magma_name = (lambda x: to8b(cm.magma(x))), "matplotlib cm.magma"
    except ImportError:
        def magma(x):
            s = x * np.float32(256)
            return table[np.where(np.isnan(x), 256, np.where(x < 0, 0, np.where(s >= 256, 255, np.trunc(s)))).astype(np.int64)]
        magma_name = "table lookup"
    kw = dict(image=t["image"], phasor=t["phasor"], depth=t["depth"], acc=t["acc"], dd=t["dd"], ranges=[float(x) for x in ranges],
              zplanes=(float(znear), float(zfar)), depth_range=float(depth_range), phase_offset=phase_offset, tof_multiplier=mult)
    total, _ = present.sheet_layout(H, W, 63)
    sheet = torch.empty(total, device=dev, dtype=torch.uint8)
    sheets = present.ViewSheets(slots=2)

    def via_sheets():
        sheets.submit(0, **kw)
        for _ in sheets.ready(wait=True):
            pass

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        present.view_images(out=sheet, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        present.view_images(out=sheet, **kw)

    # the routes agree before they are timed (depth_tof up to arctan2's last bits: a few pixels may sit on a bin edge)
    host = host_route(t, ranges, znear, zfar, depth_range, phase_offset, mult, magma)[0]
    got = {k: x.cpu().numpy() for k, x in present.view_images(**kw).items()}
    for k in ("color", "real", "imag", "amp", "depth", "depth_norm", "dd"):
        assert np.array_equal(got[k], host[k]), k
    assert np.array_equal(got["quad"], np.stack(host["quad"])) and (got["depth_tof"] != host["depth_tof"]).any(-1).mean() < 1e-3
    res = alternate(dict(host_numpy=lambda: host_route(t, ranges, znear, zfar, depth_range, phase_offset, mult, magma),
                         view_images=lambda: present.view_images(out=sheet, **kw), view_images_graph=graph.replay,
                         view_sheets=via_sheets), args.views)
    floats = 4 * H * W * (7 * 3 + 4 + 3 + 2 + 3 + 1)           # the copies: the phasor x3, 4 single planes of it, depth x3, acc x2, colour, dd
    res["host_numpy"]["bytes_to_host"] = floats
    res["view_images"]["bytes_to_host"] = res["view_images_graph"]["bytes_to_host"] = 0
    res["view_sheets"]["bytes_to_host"] = total
    out = dict(device=torch.cuda.get_device_name(0), size="%dx%d" % (W, H), colour_map=magma_name, routes=res)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
