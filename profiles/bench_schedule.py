"""RunSchedule.tick() beside the host statements it replaces in front of a replayed iteration, at 320 x 240 and 640 x 480.

    host      the statements of bench_loop.py:264-292 between two replays: the generator's state saved, ``torch.manual_seed(it)``,
              ``s_bg.uniform_(-1, 1)``, the state put back; ``update_learning_rate`` of both optimizers as the reference has it
              (13 groups and one, scene/gaussian_model.py:294-313) and ``refresh_lr()`` of both
    tick      run.tick(): one launch; the table holds the same rates for the same iterations

Both run in this process on the same optimizers' groups.  Per route and shape:

    wall_us    host clock around CALLS calls and one synchronise, per call: what the loop pays between two replays
    graph_us   the device work of a route -- the tick, or the fill alone (a captured ``uniform_`` repeats one seed: it is there for
               its time only) -- CALLS times in one graph, device events around a replay, per call

and once, ``c3_loop``: bench_loop's C3 iteration replayed from its graph as it stands, and the same with a ``tick()`` of the
frame's size queued in front of every replay (bench_loop.py is not changed, so its own host statements stay in both: the
difference is what the tick adds to the loop, not what dropping the statements would save).  The routes alternate and the median
of ROUNDS windows is kept.  Nothing is recorded without a HIP device.

    python profiles/bench_schedule.py --out profiles/schedule_bench.json
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

import torch  # noqa: E402

CALLS, ROUNDS, ITERATIONS = 200, 7, 7000
SHAPES = ((240, 320), (480, 640))
LOOP_WINDOW, LOOP_EAGER = 60, 8                  # 8 + 14 windows stay below iteration 1000, where the SH degree (and the graph) changes
GROUPS = ("xyz", "f_dc_color", "f_rest_color", "phase_f_dc", "phase_f_rest", "amp_f_dc", "amp_f_rest", "opacity", "scaling", "rotation",
          "f_seg_color", "phase_offset", "dc_offset")


def optimizers(dev):
    """Both optimizers of the reference's model with one small parameter per group, stepped once"""
    import bench_loop
    from gftorf_amd import FusedAdam
    new = lambda: torch.zeros(64, device=dev, requires_grad=True)
    opt = FusedAdam([{"params": [new()], "lr": 1e-3, "name": n} for n in GROUPS], lr=0.0, eps=1e-15, capturable=True)
    net = FusedAdam([{"params": [new() for _ in range(20)], "lr": 8e-4, "name": "deform"}], lr=0.0, eps=1e-15, capturable=True)
    for o in (opt, net):
        for g in o.param_groups:
            for p in g["params"]:
                p.grad = torch.ones_like(p)
        o.step()
    xyz = bench_loop.expon_lr(1.6e-4 * 4.5, 1.6e-6 * 4.5, 30000)
    amp = bench_loop.expon_lr(1.6e-4 * 4.5 ** 2, 1.6e-4, 30000)
    phase = bench_loop.expon_lr(0.0, 0.0, 30000)
    deform = bench_loop.expon_lr(8e-4, 1.6e-6, 28000)

    def update(it):                                                  # scene/gaussian_model.py:294-313
        for g in opt.param_groups:
            lr = g["lr"]
            if g["name"] == "xyz" or g["name"].startswith("delta_xyz"):
                lr = xyz(it)
            if g["name"] in ["phase_f_dc"]:
                lr = phase(it)
            if g["name"] in ["phase_f_rest"]:
                lr = phase(it)
            if g["name"] in ["amp_f_dc"]:
                lr = amp(it)
            if g["name"] in ["amp_f_rest"]:
                lr = amp(it)
            if it > 4000:
                if g["name"] in ["phase_offset"]:
                    lr = 1e-6
                if g["name"] in ["dc_offset"]:
                    lr = 1e-6
            g["lr"] = lr

    def update_net(it):                                              # scene/deform_model.py:42-47
        for g in net.param_groups:
            if g["name"] == "deform":
                g["lr"] = deform(it)

    return opt, net, update, update_net


def timed(fn, graph=None, calls=CALLS):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev[0].record()
    if graph is not None:
        graph.replay()
    else:
        for k in range(calls):
            fn(k)
    ev[1].record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls, ev[0].elapsed_time(ev[1]) * 1e3 / calls


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(CALLS):
            fn(k)
    return graph


def measure(H, W, dev):
    from gftorf_amd import schedule
    opt, net, update, update_net = optimizers(dev)
    s_bg = torch.zeros((7, H, W), device=dev)
    run = schedule.RunSchedule(dev, 1, ITERATIONS, bg_shape=(7, H, W))
    t0 = time.perf_counter()
    run.record_lrs(opt, update)
    run.record_lrs(net, lambda it: update_net(it - 2000))
    recorded = time.perf_counter() - t0
    opt.lr_on_device(True)
    net.lr_on_device(True)
    run.commit()
    opt.lr_on_device(False)                                          # (the host route below writes the same slots through pinned memory)
    net.lr_on_device(False)

    def host(k):
        it = 1 + k % ITERATIONS
        rs = torch.random.get_rng_state()
        torch.manual_seed(it)
        s_bg.uniform_(-1.0, 1.0)
        torch.random.set_rng_state(rs)
        update(it)
        update_net(it - 2000)
        opt.refresh_lr()
        net.refresh_lr()

    def tick(k):
        run.tick()

    def fill(k):
        s_bg.uniform_(-1.0, 1.0)

    res = {"H": H, "W": W, "calls": CALLS, "groups": len(GROUPS) + 1, "destinations": run.D,
           "record_lrs_seconds_for_%d_iterations" % ITERATIONS: round(recorded, 3)}
    host(4)
    run.seek(5).tick()
    torch.cuda.synchronize()
    res["same_background"] = bool(torch.equal(run.bg, s_bg))
    graphs = {"tick": captured(tick), "fill": captured(fill)}
    took = {k: [] for k in ("host_wall_us", "tick_wall_us", "tick_graph_us", "fill_graph_us")}
    for fn in (host, tick):
        timed(fn)
    for _ in range(ROUNDS):
        took["host_wall_us"].append(timed(host)[0])
        run.seek(1)
        took["tick_wall_us"].append(timed(tick)[0])
        run.seek(1)
        took["tick_graph_us"].append(timed(None, graphs["tick"])[1])
        took["fill_graph_us"].append(timed(None, graphs["fill"])[1])
    for k, values in took.items():
        res[k] = round(statistics.median(values), 3)
        res[k + "_spread"] = [round(min(values), 3), round(max(values), 3)]
    res["overran"] = run.status()[1]
    return res


def c3_loop(dev):
    """it/s of bench_loop's graph-replayed C3 iteration, and with a tick in front of every replay"""
    import bench_loop
    from gftorf_amd import schedule
    cfg = bench_loop.C3
    iteration, _info = bench_loop.build_loop(dev, cfg, graph=True)
    run = schedule.RunSchedule(dev, 1, 900, bg_shape=(7, cfg["H"], cfg["W"])).commit()
    state = dict(it=0)

    def plain(k):
        state["it"] += 1
        iteration(state["it"])

    def with_tick(k):
        run.tick()
        plain(k)

    for k in range(LOOP_EAGER):                                      # the eager iterations and the capture
        plain(k)
    took = {"plain": [], "with_tick": []}
    for _ in range(3):
        for name, fn in (("plain", plain), ("with_tick", with_tick)):
            took[name].append(timed(fn, calls=LOOP_WINDOW)[0])
    for _ in range(ROUNDS - 3):
        for name, fn in (("with_tick", with_tick), ("plain", plain)):
            took[name].append(timed(fn, calls=LOOP_WINDOW)[0])
    res = {"iterations": state["it"], "window": LOOP_WINDOW}
    for name, values in took.items():
        res[name + "_us_per_iteration"] = round(statistics.median(values), 2)
        res[name + "_us_spread"] = [round(min(values), 2), round(max(values), 2)]
        res[name + "_it_per_s"] = round(1e6 / statistics.median(values), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-loop", action="store_true")
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_schedule.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS}
    for H, W in SHAPES:
        out["%dx%d" % (W, H)] = measure(H, W, dev)
    if not opts.no_loop:
        out["c3_loop"] = c3_loop(dev)
    print(json.dumps(out), flush=True)
    if opts.out:
        with open(opts.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
