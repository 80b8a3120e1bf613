"""The PNG files of one debug sheet (240 x 320, 19 images = 28 files) and one view sheet (480 x 640): gftorf_amd.png on the device
against the host route they replace, ``present.ViewSheets.ready()`` followed by Pillow's PNG encoder (what imageio calls).

    device    png.encode over the sheet's images, timed by device events: eagerly and as a replayed graph, best of --repeats
    sheets    PngSheets.submit_* .. ready(wait=True), host clock, end to end with the copy to pinned memory
    host      ViewSheets.submit* .. ready(wait=True), then Image.save(compress_level = 1 and 9) of every image, on one thread
              and on 16 (Pillow releases the GIL while zlib runs), host clock, best of --repeats
    bytes     the files' sizes by each route, and the raw bytes

The inputs are a synthetic room: smooth fields with edges, the ground truth with sigma = 2 / 255 sensor noise, the render
without.  Every device file is decoded with Pillow and compared with the sheet before anything is timed.

    python profiles/bench_png.py --out profiles/png_bench.json
"""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

LAUNCHES_PER_CALL = 3       # gft_png_encode at level 1: k_png_filter, k_png_segment, k_png_assemble (two at level 0)


def room(H, W, seed):
    """float32 inputs of present.view_images and present.debug_images for one H x W view"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = x / W, y / H
    wall = 2.0 + 1.5 * u + 0.3 * np.sin(6 * v)
    box = (np.abs(u - 0.55) < 0.18) & (np.abs(v - 0.6) < 0.25)
    depth = np.where(box, 1.4 + 0.2 * u, wall)
    shade = 0.35 + 0.5 * np.clip(1.2 - 0.3 * depth, 0, 1)
    albedo = np.stack([0.6 + 0.3 * np.sin(9 * u), 0.5 + 0.3 * np.cos(7 * v), np.where(box, 0.8, 0.4) + 0 * u])
    image = np.clip(albedo * shade, 0, 1)
    gt_image = np.clip(image + rng.normal(0, 2 / 255, image.shape), 0, 1)
    dr = 7.5
    phase = 2 * np.pi * (2 * depth) / dr % (2 * np.pi)
    amp = 0.3 * shade / depth ** 2
    gt = np.stack([amp * np.cos(phase), amp * np.sin(phase), amp]) * (1 + rng.normal(0, 0.01, (3, H, W)))
    quad = np.stack([amp * np.cos(phase + k * np.pi / 2) for k in range(4)])
    phasor = np.concatenate([gt * (1 + 0.02 * np.sin(11 * u)), quad])
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(image=f(image), gt_image=f(gt_image), depth=f(depth[None]), acc=f(np.clip(0.9 + 0.1 * np.cos(5 * u), 0, 1)[None]),
                dd=f((0.05 * np.abs(np.sin(13 * u * v)))[None]), phasor=f(phasor), gt_phasor=f(gt), gt_quad=f(quad * (1 + rng.normal(0, 0.01, quad.shape))),
                phase_depth=f(depth * (1 + 0.01 * np.sin(17 * u))), gt_phase_depth=f(depth), depth_range=dr)


def pillow_bytes(a, level):
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(a).save(out, format="PNG", compress_level=level)
    return out.getvalue()


def planes(arrays):
    """the images of a ViewSheets dict as Pillow takes them: the quads as four gray images, no float images"""
    out = {}
    for k, a in arrays.items():
        if a.dtype != np.uint8:
            continue
        if a.ndim == 3 and a.shape[0] == 4 and a.shape[2] not in (3, 4):
            out.update({"%s%d" % (k, q): a[q] for q in range(4)})
        else:
            out[k] = a
    return out


def best(fn, repeats):
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return min(times)


def best_events(fn, repeats):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return min(times)


def measure(kind, H, W, repeats, dev):
    from PIL import Image
    from gftorf_amd import png, present
    r = room(H, W, seed=H)
    t = {k: torch.tensor(a, device=dev) for k, a in r.items() if isinstance(a, np.ndarray)}
    zp = present.zplanes(r["depth_range"])
    if kind == "debug":
        kw = dict(phasor=t["phasor"], gt_phasor=t["gt_phasor"], depth=t["depth"], phase_depth=t["phase_depth"], gt_phase_depth=t["gt_phase_depth"],
                  dd=t["dd"], image=t["image"], gt_image=t["gt_image"], gt_quad=t["gt_quad"], quad_index=1,
                  ranges=[-0.2, 0.2, -0.2, 0.2, 0.0, 0.2, 0.0, 0.5], zplanes=zp)
        sheet = present.debug_images(**kw)
        submit_plain, submit_png = "submit_debug", "submit_debug"
    else:
        kw = dict(image=t["image"], phasor=t["phasor"], depth=t["depth"], acc=t["acc"], dd=t["dd"], ranges=[-0.2, 0.2, -0.2, 0.2, 0.0, 0.2],
                  zplanes=zp, depth_range=r["depth_range"])
        sheet = present.view_images(**kw)
        submit_plain, submit_png = "submit", "submit_view"
    coded = {k: v for k, v in sheet.items() if v.dtype == torch.uint8}
    host_images = planes({k: v.cpu().numpy() for k, v in coded.items()})
    res = {"H": H, "W": W, "files": len(host_images), "raw_bytes": int(sum(a.size for a in host_images.values())),
           "launches_per_call": LAUNCHES_PER_CALL}

    # the device files are the sheet's pixels
    files = png.encode(coded).to_host()
    assert list(files) == list(host_images)
    for k, a in host_images.items():
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[k]))), a), k
    res["device_bytes"] = int(sum(len(b) for b in files.values()))
    res["device_level0_bytes"] = int(sum(len(b) for b in png.encode(coded, level=0).to_host().values()))
    res["device_bytes_per_file"] = {k: len(b) for k, b in files.items()}

    shapes = [(a.shape[0], a.shape[1], a.shape[2] if a.ndim == 3 else 1) for a in host_images.values()]
    out = torch.empty((png.layout(shapes)[0],), device=dev, dtype=torch.uint8)
    scratch = torch.empty((png.scratch_bytes(shapes),), device=dev, dtype=torch.uint8)
    eager = lambda level: (lambda: png.encode(coded, level=level, out=out, scratch=scratch))
    for level in (1, 0):
        for _ in range(3):
            eager(level)()
        res["device_eager_level%d_s" % level] = best_events(eager(level), repeats)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eager(level)()
        for _ in range(3):
            graph.replay()
        res["device_graph_level%d_s" % level] = best_events(graph.replay, repeats)
        del graph

    sheets = png.PngSheets(slots=2)

    def through_sheets():
        getattr(sheets, submit_png)(0, **kw)
        for _, got in sheets.ready(wait=True):
            pass
    through_sheets()
    res["png_sheets_end_to_end_s"] = best(through_sheets, repeats)

    plain = present.ViewSheets(slots=2)
    pool = ThreadPoolExecutor(max_workers=16)

    def through_pillow(level, threads):
        getattr(plain, submit_plain)(0, **kw)
        for _, arrays in plain.ready(wait=True):
            todo = list(planes(arrays).values())
            if threads == 1:
                return [pillow_bytes(a, level) for a in todo]
            return list(pool.map(lambda a: pillow_bytes(a, level), todo))
    for level in (1, 9):
        res["pillow_level%d_bytes" % level] = int(sum(len(b) for b in through_pillow(level, 1)))
        for threads in (1, 16):
            res["host_pillow_level%d_%dthread_s" % (level, threads)] = best(lambda: through_pillow(level, threads), max(3, repeats // 4))
    pool.shutdown()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    import PIL
    out = {"device": torch.cuda.get_device_name(0), "pillow": PIL.__version__, "repeats": args.repeats, "host_threads_available": os.cpu_count()}
    for kind, H, W in (("debug", 240, 320), ("view", 480, 640)):
        out["%s_%dx%d" % (kind, W, H)] = measure(kind, H, W, args.repeats, dev)
        print(json.dumps({kind: out["%s_%dx%d" % (kind, W, H)]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
