"""The motion tracks and quad images of the track program (render_ftorf_viz_traj.py:217-347): the reference's loop shape with
its `.cpu()` pattern, restated here on synthetic data, against gftorf_amd.tracks and present.quad_images.  P = n = 300 000
Gaussians, T = 60 frames, a 320 x 240 ToF image, the drawn Gaussians as the program's default quantiles give them.

Without --step the script runs every step as a child process of its own under `timeout`, one after the other, stops at the
first that fails, and writes the merged result; a step alone prints its part as one JSON line.

    baseline  :264-347 as the reference runs it: T projections in torch, the five quantiles, then the Python double loop
              over frames and drawn Gaussians with three `.detach().cpu()` reads per visit; host-blocked seconds per part
    tracks    integrate (device time from events and from one graph replay, enqueue time on the host), select, table, the
              table's one copy, walk on the host copy; and whether walk draws the tracks the baseline loop drew
    flows     network evaluations and time of the sequence's deformation queries: two per view (:223-228) against
              tracks.sequence_flows
    quad      a view's four quad images: four `.cpu()` copies and tof_to_image (matplotlib) against present.quad_images

    python profiles/bench_tracks.py --out profiles/tracks_bench.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

P, T, H, W = 300_000, 60, 240, 320
QUANTILES = dict(big_motion_quantile=0.9, z_distr_quantile=0.5, opacity_quantile=0.5, small_size_quantile=0.1, big_size_quantile=0.9)
STEPS = {"baseline": 600, "tracks": 240, "flows": 300, "quad": 240}          # seconds each step may take


def scene(dev):
    """synthetic inputs on the device: cameras that drift, points in front of them, one flow row per four frames"""
    rng = np.random.default_rng(0)
    K = np.tile(np.array([[260.0, 0, W / 2], [0, 260.0, H / 2], [0, 0, 1]]), (T, 1, 1))
    view = np.tile(np.eye(4), (T, 1, 1))
    view[:, 3, 0] = 0.001 * np.arange(T)                    # the translation row of the transposed matrix
    z = rng.uniform(1.5, 4.0, P)
    pos = np.stack([z * rng.uniform(-0.7, 0.7, P), z * rng.uniform(-0.55, 0.55, P), z], axis=1)
    U = (T + 3) // 4
    flow = rng.normal(0, 0.004, (U, P, 3)) * rng.uniform(0, 1, (1, P, 1)) ** 4      # few Gaussians move much
    up = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    return dict(initial_pos=up(pos), flow=up(flow), flow_index=torch.tensor([t // 4 for t in range(T)], dtype=torch.int32, device=dev),
                K=up(K), world_view=up(view), opacity=up(rng.uniform(0.01, 0.99, (P, 1))),
                scaling=up(np.exp(rng.normal(-4, 0.7, (P, 3)))))


def project(points3d, K, view):
    """scene/torf_utils.py:108-114"""
    n = points3d.shape[0]
    homog = torch.cat([points3d.T, torch.ones((1, n), device=points3d.device)], dim=0)
    h = K @ (view.transpose(1, 0) @ homog)[:3, :]
    return (h[:2, :] / (h[2:, :] + 1e-7)).reshape(2, n).T


def baseline(s):
    """:264-347 in the reference's shape; returns the parts' host-blocked seconds, S and the tracks drawn"""
    sync = torch.cuda.synchronize
    sync()
    t0 = time.perf_counter()
    flows = torch.stack([s["flow"][int(u)] for u in s["flow_index"].tolist()], dim=0)
    all_3d, all_2d = [s["initial_pos"]], [project(s["initial_pos"], s["K"][0], s["world_view"][0])]
    for vid in range(1, T):
        all_3d.append(all_3d[vid - 1] + flows[vid - 1])
        all_2d.append(project(all_3d[-1], s["K"][vid], s["world_view"][vid]))
    sync()
    t1 = time.perf_counter()
    q = QUANTILES
    motion = lambda: torch.mean(torch.sum(flows ** 2, dim=-1), dim=0)
    mask = motion() > torch.quantile(motion(), q["big_motion_quantile"])
    torch.quantile(motion(), 0.95)
    z_thr = torch.quantile(torch.mean(torch.stack(all_3d, dim=0)[:, mask, -1], dim=0), q["z_distr_quantile"])
    mask *= torch.mean(torch.stack(all_3d, dim=0)[:, :, -1], dim=0) < z_thr
    mask *= (s["opacity"] > torch.quantile(s["opacity"][mask], q["opacity_quantile"])).squeeze()
    small = torch.quantile(torch.mean(s["scaling"][mask], dim=-1), q["small_size_quantile"])
    big = torch.quantile(torch.mean(s["scaling"][mask], dim=-1), q["big_size_quantile"])
    mask *= ((small < torch.mean(s["scaling"], dim=-1)) * (torch.mean(s["scaling"], dim=-1) < big)).squeeze()
    pos_2d = torch.stack(all_2d, dim=0)[:, mask, :]
    sync()
    t2 = time.perf_counter()
    S = int(pos_2d.shape[1])
    trajectories, reads = {}, 0
    for vid in range(T):
        used = set()
        for i in range(S):
            init_x, init_y = pos_2d[0, i].detach().cpu()
            old_x, old_y = pos_2d[vid - 1, i].detach().cpu()
            new_x, new_y = pos_2d[vid, i].detach().cpu()
            reads += 3
            init_x, init_y, old_x, old_y, new_x, new_y = (float(v) for v in (init_x, init_y, old_x, old_y, new_x, new_y))
            if not (0 < init_x < W and 0 < init_y < H):
                continue
            if any((int(init_x) + dx, int(init_y) + dy) in used for dx in (-1, 0, 1) for dy in (-1, 0, 1)):
                continue
            if vid == 0:
                trajectories[i] = 1
            else:
                if not (0 < new_x < W - 1 and 0 < new_y < H - 1 and 0 < old_x < W and 0 < old_y < H):
                    continue
                trajectories[i] = trajectories.get(i, 0) + 1
            used.add((int(init_x), int(init_y)))
    t3 = time.perf_counter()
    return dict(positions_s=t1 - t0, select_s=t2 - t1, loop_s=t3 - t2, total_s=t3 - t0, S=S, blocking_reads=reads,
                loop_us_per_read=(t3 - t2) * 1e6 / max(reads, 1)), trajectories


def median_us(fn, rounds=9, inner=1):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / inner)
    return statistics.median(out)


def step_baseline(dev):
    res, _ = baseline(scene(dev))
    return res


def step_tracks(dev):
    from gftorf_amd import tracks
    s = scene(dev)
    args = {k: s[k] for k in ("initial_pos", "flow", "flow_index", "K", "world_view")}
    call = lambda: tracks.integrate(size=(H, W), **args)
    tr = call()
    torch.cuda.synchronize()
    res = dict(integrate_wall_us=median_us(call))
    enq = []
    for _ in range(9):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        enq.append((time.perf_counter() - t0) * 1e6)
        torch.cuda.synchronize()
    res["integrate_enqueue_us"] = statistics.median(enq)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dev_us = []
    for _ in range(9):
        ev[0].record()
        call()
        ev[1].record()
        torch.cuda.synchronize()
        dev_us.append(ev[0].elapsed_time(ev[1]) * 1e3)
    res["integrate_events_us"] = statistics.median(dev_us)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    res["integrate_graph_us"] = median_us(graph.replay, inner=10)
    res["integrate_bytes"] = T * P * 8 + int(s["flow"].numel()) * 4 + T * P + P * 12 * 2 + P * 8
    res["integrate_GBps"] = res["integrate_bytes"] / res["integrate_graph_us"] / 1e3
    pick = lambda: tracks.select(tr, s["opacity"], s["scaling"], **QUANTILES)
    mask, _ = pick()
    res["select_us"] = median_us(pick, rounds=5)
    res["table_us"] = median_us(lambda: tracks.table(tr, mask))
    tab = tracks.table(tr, mask)
    res["S"], res["table_bytes"] = tab.S, int(tab.buffer.numel())
    res["copy_us"] = median_us(tab.to_host)
    host = tab.to_host()
    t0 = time.perf_counter()
    for _, drawn, _ in tracks.walk(host):
        pass
    res["walk_s"] = time.perf_counter() - t0
    res["tracks_drawn"] = len(drawn)
    t0 = time.perf_counter()
    tr2 = call()
    m2, _ = tracks.select(tr2, s["opacity"], s["scaling"], **QUANTILES)
    h2 = tracks.table(tr2, m2).to_host()
    for _ in tracks.walk(h2):
        pass
    res["total_s"] = time.perf_counter() - t0
    if os.environ.get("BENCH_TRACKS_COMPARE", "1") == "1":
        _, ref = baseline(s)
        res["same_tracks_as_baseline"] = bool(sorted(ref) == sorted(drawn) and all(ref[k] == len(drawn[k]) for k in ref))
    return res


def step_flows(dev):
    from gftorf_amd import DeformNetwork, tracks
    torch.manual_seed(0)
    net = DeformNetwork(D=8, W=256, xyz_multires=10, t_multires=10, sh_degree=3).to(dev)
    xyz = (torch.rand(P, 3, device=dev) * 2 - 1)
    frame_ids, denom = list(range(T)), T - 1
    calls = []
    hook = net.register_forward_hook(lambda *a: calls.append(1))

    def per_view():
        with torch.no_grad():
            for f in frame_ids:
                for fid in ((f // 4) * 4, (f // 4 + 1) * 4):
                    t = torch.tensor(np.array([fid / denom])).float().cuda().unsqueeze(0).expand(P, -1)
                    net(xyz, t)

    shared = lambda: tracks.sequence_flows(net, xyz, frame_ids, denom)
    per_view(), shared()
    torch.cuda.synchronize()
    del calls[:]
    a = median_us(per_view, rounds=3)
    n_a = len(calls) // 3
    del calls[:]
    b = median_us(shared, rounds=3)
    n_b = len(calls) // 3
    hook.remove()
    return dict(per_view_evaluations=n_a, per_view_us=a, sequence_flows_evaluations=n_b, sequence_flows_us=b)


def step_quad(dev):
    import matplotlib.pyplot as plt
    from gftorf_amd import present
    rng = np.random.default_rng(1)
    ph = torch.tensor(rng.uniform(-0.7, 0.7, (7, H, W)).astype(np.float32), device=dev)
    perm = torch.tensor([2, 0, 3, 1], device=dev)

    def tof_to_image(tof):
        rgb = plt.get_cmap("seismic")(plt.Normalize(-0.5, 0.5)(np.clip(tof, -0.5, 0.5)))[:, :, :3]
        return (255 * rgb).astype(np.uint8)

    def host():
        return [tof_to_image(ph[3:][perm][i].detach().cpu().numpy()) for i in range(4)]

    out = torch.empty((4, H, W, 3), device=dev, dtype=torch.uint8)
    pinned = torch.empty((4, H, W, 3), dtype=torch.uint8, pin_memory=True)
    call = lambda: present.quad_images(ph, permutation=(2, 0, 3, 1), out=out)

    def to_host():
        call()
        pinned.copy_(out, non_blocking=True)

    assert np.array_equal(np.stack(host()), call().cpu().numpy())
    graph = torch.cuda.CUDAGraph()
    call()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        call()
    return dict(size="%dx%d" % (W, H), host_four_copies_us=median_us(host, rounds=7), quad_images_wall_us=median_us(call, inner=20),
                quad_images_graph_us=median_us(graph.replay, inner=20), quad_images_to_pinned_us=median_us(to_host, inner=20),
                host_bytes=4 * H * W * 4, device_bytes_to_host=4 * H * W * 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=list(STEPS), default=None)
    args = ap.parse_args()
    if args.step:
        if not torch.cuda.is_available():
            raise SystemExit("bench_tracks.py needs a HIP device: nothing is measured without one")
        print(json.dumps({args.step: globals()["step_" + args.step](torch.device("cuda:0"))}), flush=True)
        return
    out = dict(P=P, T=T, size="%dx%d" % (W, H), quantiles=QUANTILES)
    for step, limit in STEPS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("bench_tracks.py: step %s ended with status %d; nothing further is started" % (step, r.returncode))
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps({step: out[step]}), flush=True)
    out["device"] = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_name(0))"], capture_output=True,
                                   text=True).stdout.strip()
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
