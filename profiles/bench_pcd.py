"""The input point cloud (scene/dataset_readers.py:110-150, 530-586, 1067-1118; scene/gaussian_model.py:180-236) on
gftorf_amd.pcd, on 320 x 240 ToF frames, beside this project's own restatement of the same results (tests/pcd_ref.py:
vectorised numpy and eager torch).

The restatement is NOT a model of the reference's cost: the reference fills its file from one Python tuple per point and
unwraps F-ToRF distances in a Python loop per pixel, which the restatement does not do.  Its timings are printed as
`*_restatement_s` for scale only; what this script measures is gftorf_amd.pcd.

    init      pcd.phase_init_torf of one frame, end to end (unproject, the file, the cloud)
    proxy     pcd.proxy_clouds: the two full-resolution clouds per frame of an 8-frame sequence, end to end
    store     pcd.store on one frame's points; the file is compared byte for byte with the restatement's
    create    pcd.create_tensors; the tensors are compared bit for bit with the restatement's
    kernels   the unproject, pack and create calls between device events (they include the host's preparation)

Each pair is timed in alternating windows and the median window is kept.  Nothing is recorded without a HIP device, and no
timing field is ever filled in by hand.

    python profiles/bench_pcd.py --out profiles/pcd_bench.json
"""
import argparse
import json
import math
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, FRAMES, ROUNDS = 240, 320, 8, 3
ZNEAR, FOV_X, FOV_Y = 0.45, 2 * math.atan(0.6), 2 * math.atan(0.45)


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


def events_us(fn, repeats=9):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    took = []
    for _ in range(repeats):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        took.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return statistics.median(took)


def measure(folder, dev):
    import pcd_ref as R
    from gftorf_amd import pcd
    view = np.eye(4, dtype=np.float32)
    view[:3, 3] = (0.1, -0.05, 0.2)
    tofs = [R.make_frame(H, W, 100 + i) for i in range(FRAMES)]
    rendered = [np.random.default_rng(200 + i).uniform(1.0, 3.0, (H, W)).astype(np.float32) for i in range(FRAMES)]
    args = (ZNEAR, FOV_X, FOV_Y, view, R.DEPTH_RANGE, R.PHASE_OFFSET)
    frames = [dict(tof_image=torch.tensor(t, device=dev), znear=ZNEAR, FovX_tof=FOV_X, FovY_tof=FOV_Y, world_view=view,
                   rendered=torch.tensor(r, device=dev)) for t, r in zip(tofs, rendered)]
    ref_path, own_path = os.path.join(folder, "ref.ply"), os.path.join(folder, "own.ply")
    res = {"H": H, "W": W, "frames": FRAMES}

    def write(path, data):
        with open(path, "wb") as f:
            f.write(data)

    def ref_init():
        o = R.unproject(tofs[0], 1, *args, "torf_init")
        n = o["xyz"].shape[0]
        seg = np.repeat(np.array([[1.0, 0.0, 0.0]]), n, axis=0)
        write(ref_path, R.store_bytes(o["xyz"], o["color"] * 255.0, R.zero_phasor(n), o["amplitude"].reshape(-1, 1), seg * 255.0))
        return R.fetch_bytes(open(ref_path, "rb").read())

    own_init = lambda: pcd.phase_init_torf(frames[:1], 1, R.DEPTH_RANGE, R.PHASE_OFFSET, own_path)
    own_init()                                                  # warm-up: the library and the pinned buffers
    res["init_points"] = 2 * H * W
    res["init_restatement_s"], res["phase_init_torf_s"] = windows([ref_init, own_init], ROUNDS)
    # the points differ by the distance's last bits (atan2f), so the files are compared where the inputs are the same: below

    def ref_proxy():
        for i in range(FRAMES):
            o = R.unproject(tofs[i], 1, *args, "proxy", rendered=rendered[i])
            n = o["xyz"].shape[0]
            colors = np.tile([1, 0, 0], (n, 1)).astype(np.float32)
            colors[n // 2:, :] = np.tile([0, 0, 1], (n // 2, 1)).astype(np.float32)
            write(os.path.join(folder, "ref_%d.ply" % i), R.store_bytes(o["xyz"], colors * 255.0, R.zero_phasor(n), R.zero_phasor(n), np.zeros((n, 3))))

    own_proxy = lambda: list(pcd.proxy_clouds(frames, R.DEPTH_RANGE, R.PHASE_OFFSET, [os.path.join(folder, "own_%d.ply" % i) for i in range(FRAMES)]))
    res["proxy_restatement_s"], res["proxy_clouds_s"] = windows([ref_proxy, own_proxy], ROUNDS)

    # storePly alone on the same points: the files must be equal byte for byte
    pts = pcd.unproject(frames[0]["tof_image"], 1, *args, mode="torf_init")
    n = pts["xyz"].shape[0]
    host = {k: v.cpu().numpy() for k, v in pts.items()}
    seg = np.repeat(np.array([[255.0, 0.0, 0.0]]), n, axis=0)
    store_ref = lambda: write(ref_path, R.store_bytes(host["xyz"], host["color"] * 255.0, R.zero_phasor(n), host["amplitude"].reshape(-1, 1), seg))
    dev_args = (pts["xyz"], pts["color"] * 255.0, torch.tensor(R.zero_phasor(n), device=dev), pts["amplitude"], torch.tensor(seg, device=dev))
    store_own = lambda: pcd.store(own_path, *dev_args)
    res["store_restatement_s"], res["store_s"] = windows([store_ref, store_own], ROUNDS)
    res["same_files"] = open(ref_path, "rb").read() == open(own_path, "rb").read()
    res["file_bytes"] = os.path.getsize(own_path)

    cloud = pcd.fetch(own_path, device=dev)
    a, b = R.eager_create(cloud, 3, False, False, 0.1), pcd.create_tensors(cloud, 3)
    res["same_tensors"] = all(torch.equal(a[k], b[k]) for k in a)
    res["create_restatement_s"], res["create_tensors_s"] = windows([lambda: R.eager_create(cloud, 3, False, False, 0.1),
                                                                 lambda: pcd.create_tensors(cloud, 3)], ROUNDS)
    res["unproject_events_us"] = events_us(lambda: pcd.unproject(frames[0]["tof_image"], 1, *args, mode="torf_init"))
    res["pack_events_us"] = events_us(lambda: pcd.submit_store(own_path, *dev_args))
    res["create_events_us"] = events_us(lambda: pcd.create_tensors(cloud, 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary folder)")
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pcd.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    folder = tempfile.mkdtemp(prefix="bench_pcd_", dir=opts.dir)
    out = {"device": torch.cuda.get_device_name(0), "windows": ROUNDS}
    try:
        out["320x240"] = measure(folder, dev)
        print(json.dumps(out), flush=True)
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    if opts.out:
        with open(opts.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
