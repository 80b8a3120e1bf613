"""The model's PLY files (scene/gaussian_model.py:340-367, 378-454; Scene.save, scene/__init__.py:127-130): the reference's
route, restated here without plyfile, against gftorf_amd.ply, at P = 100 000 and 1 000 000 Gaussians of SH degree 3.

    save      reference: the blocking `.cpu()` copies, np.concatenate, `elements[:] = list(map(tuple, attributes))` and
              elements.tofile, once per file; here: ply.save_pair (one launch, two files), end to end
    load      reference: the file as a structured array, the per-column copies into float64 arrays and the 11
              torch.tensor(...) uploads; here: ply.read_gaussians, end to end
    pack      the pack launch alone (ply.submit), by device events

Each pair is timed in alternating windows (reference, here, reference, ...) and the median window is kept.  The files of both
routes are compared byte for byte and the loaded tensors bit for bit.

    python profiles/bench_ply.py --out profiles/ply_bench.json
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_REST, SCALES, SEG = 15, 3, 3
SIZES = {100_000: 5, 1_000_000: 3}          # P: windows per route


class Model:
    max_sh_degree = 3
    active_sh_degree = 0


def model(P, dev):
    torch.manual_seed(P)
    m = Model()
    for attr, shape in (("_xyz", (P, 3)), ("_features_dc_color", (P, 1, 3)), ("_features_rest_color", (P, N_REST, 3)),
                        ("_opacity", (P, 1)), ("_scaling", (P, SCALES)), ("_rotation", (P, 4)), ("_features_dc_phase", (P, 1, 1)),
                        ("_features_rest_phase", (P, N_REST, 1)), ("_features_dc_amp", (P, 1, 1)), ("_features_rest_amp", (P, N_REST, 1)),
                        ("_features_seg_color", (P, SEG))):
        setattr(m, attr, torch.randn(shape, device=dev))
    return m


def reference_save(m, path, names, sibr_only):
    """save_ply:340-367, the file written as plyfile writes one element of float properties"""
    os.makedirs(os.path.dirname(path), exist_ok=True)
    flat = lambda t: t.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    xyz = m._xyz.detach().cpu().numpy()
    normals = np.zeros_like(xyz)
    parts = [xyz, normals, flat(m._features_dc_color), flat(m._features_rest_color), m._opacity.detach().cpu().numpy(),
             m._scaling.detach().cpu().numpy(), m._rotation.detach().cpu().numpy()]
    if not sibr_only:
        parts += [flat(m._features_dc_phase), flat(m._features_rest_phase), flat(m._features_dc_amp), flat(m._features_rest_amp),
                  m._features_seg_color.detach().contiguous().cpu().numpy()]
    elements = np.empty(xyz.shape[0], dtype=[(n, "f4") for n in names])
    attributes = np.concatenate(parts, axis=1)
    elements[:] = list(map(tuple, attributes))
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(elements) +
                 "".join("property float %s\n" % n for n in names) + "end_header\n").encode("ascii"))
        elements.tofile(f)


def reference_load(path, max_sh_degree, dev):
    """load_ply:378-454 over the structured array plyfile would hand out"""
    from gftorf_amd import ply
    with open(path, "rb") as f:
        P, names, offset = ply.parse_header(f.read(1 << 16))
    el = np.fromfile(path, dtype=[(n, "<f4") for n in names], count=P, offset=offset)
    xyz = np.stack((np.asarray(el["x"]), np.asarray(el["y"]), np.asarray(el["z"])), axis=1)
    opacities = np.asarray(el["opacity"])[..., np.newaxis]

    def family(prefix):
        found = sorted((n for n in names if n.startswith(prefix)), key=lambda x: int(x.split("_")[-1]))
        out = np.zeros((xyz.shape[0], len(found)))
        for idx, name in enumerate(found):
            out[:, idx] = np.asarray(el[name])
        return out

    def dc(prefix, c):
        out = np.zeros((xyz.shape[0], c, 1))
        for i in range(c):
            out[:, i, 0] = np.asarray(el["%s_%d" % (prefix, i)])
        return out

    n = (max_sh_degree + 1) ** 2 - 1
    up = lambda a: torch.tensor(a, dtype=torch.float, device=dev)
    feat = lambda a: up(a).transpose(1, 2).contiguous().requires_grad_(True)
    return {"xyz": up(xyz).requires_grad_(True), "features_dc_color": feat(dc("f_dc", 3)),
            "features_rest_color": feat(family("f_rest_").reshape((P, 3, n))), "features_dc_phase": feat(dc("phase_f_dc", 1)),
            "features_rest_phase": feat(family("phase_f_rest_").reshape((P, 1, n))), "features_dc_amp": feat(dc("amp_f_dc", 1)),
            "features_rest_amp": feat(family("amp_f_rest_").reshape((P, 1, n))), "opacity": up(opacities).requires_grad_(True),
            "scaling": up(family("scale_")).requires_grad_(True), "rotation": up(family("rot")).requires_grad_(True),
            "features_seg_color": up(family("f_seg_color_")).contiguous().requires_grad_(True)}


def windows(fns, rounds):
    """seconds of every window, the routes alternating"""
    out = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append(time.perf_counter() - t0)
    return [statistics.median(w) for w in out]


def measure(P, rounds, folder, dev):
    from gftorf_amd import ply
    m = model(P, dev)
    names = {full: ply.columns(m, full) for full in (False, True)}
    ref = [os.path.join(folder, "ref", "point_cloud.ply"), os.path.join(folder, "ref", "point_cloud_full.ply")]
    own = [os.path.join(folder, "own", "point_cloud.ply"), os.path.join(folder, "own", "point_cloud_full.ply")]

    def ref_save():
        reference_save(m, ref[0], names[False], True)
        reference_save(m, ref[1], names[True], False)

    ply.save_pair(m, *own)                                      # warm-up: the pinned buffers
    res = {"K_sibr": len(names[False]), "K_full": len(names[True])}
    res["save_reference_s"], res["save_pair_s"] = windows([ref_save, lambda: ply.save_pair(m, *own)], rounds)
    print(json.dumps({"P": P, "save": res}), flush=True)
    res["same_files"] = all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(ref, own))
    res["file_bytes"] = [os.path.getsize(p) for p in own]
    load = lambda: reference_load(ref[1], 3, dev)
    read = lambda: ply.read_gaussians(own[1], dev, max_sh_degree=3)
    a, b = load(), read()
    res["same_tensors"] = all(torch.equal(a[k].detach().view(torch.int32), b[k].view(torch.int32)) and a[k].shape == b[k].shape for k in b)
    del a, b
    res["load_reference_s"], res["read_gaussians_s"] = windows([load, read], rounds)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    pack = []
    for _ in range(9):
        ev[0].record()
        job = ply.submit(m, path_sibr=own[0], path_full=own[1])
        ev[1].record()
        torch.cuda.synchronize()
        pack.append(ev[0].elapsed_time(ev[1]) * 1e3)
        del job
    res["pack_events_us"] = statistics.median(pack)
    res["pack_bytes"] = 4 * P * ((res["K_full"] - 3) + res["K_full"] + res["K_sibr"])
    res["pack_GBps"] = res["pack_bytes"] / res["pack_events_us"] / 1e3
    shutil.rmtree(os.path.join(folder, "ref"))
    shutil.rmtree(os.path.join(folder, "own"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary folder)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ply.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    folder = tempfile.mkdtemp(prefix="bench_ply_", dir=args.dir)
    out = {"device": torch.cuda.get_device_name(0), "windows": {str(P): r for P, r in SIZES.items()}}
    try:
        for P, rounds in SIZES.items():
            out[str(P)] = measure(P, rounds, folder, dev)
            print(json.dumps({str(P): out[str(P)]}), flush=True)
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
