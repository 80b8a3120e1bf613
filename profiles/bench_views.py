"""ViewStore.draw() beside the torch statements it replaces, on the F-ToRF group set (colour as bytes, phasor, the four quad
planes, the distance image, two optical flows, and the 96-float record of ViewStore.from_cameras) at 320 x 240 and 640 x 480.

    draw      store.draw(v): one launch
    copies    one `static.copy_(all[v])` per group and one for the record row, the pattern of bench_loop.py:275-276: seven
              launches (the colour image kept as float32 there, as the reference keeps it)

Both run in this process on the same views.  Per route and shape:

    wall_us    host clock around CALLS calls and one synchronise, per call: what an eager loop pays
    events_us  device events around the same CALLS queued calls, per call
    graph_us   CALLS calls captured into one graph, device events around a replay, per call: the device's time without the
               host's gaps -- the nearest this script gets to kernel time; a profiler's trace is a run of its own
    bytes      read + written per call, from the shapes; gb_per_s = bytes / graph_us

The routes alternate and the median of ROUNDS windows is kept.  Nothing is recorded without a HIP device.

    python profiles/bench_views.py --out profiles/views_bench.json
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

VIEWS, CALLS, ROUNDS, RECORD = 8, 200, 7, 96
SHAPES = ((240, 320), (480, 640))


def timed(fn, graph=None):
    """(wall, events) microseconds per call of CALLS queued calls of fn(k), or of one replay of `graph`, which holds CALLS"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev[0].record()
    if graph is not None:
        graph.replay()
    else:
        for k in range(CALLS):
            fn(k)
    ev[1].record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / CALLS, ev[0].elapsed_time(ev[1]) * 1e3 / CALLS


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in range(VIEWS):
            fn(k)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(CALLS):
            fn(k)
    return graph


def measure(H, W, dev):
    from gftorf_amd import views
    rng = np.random.default_rng(H)
    f = lambda *shape: rng.standard_normal((VIEWS,) + shape).astype(np.float32)
    color = rng.integers(0, 256, (VIEWS, H, W, 3)).astype(np.uint8)
    floats = dict(phasor=f(3, H, W), quad=f(4, H, W), distance=f(1, H, W), forward_flow=f(2, H, W), backward_flow=f(2, H, W))
    record = f(RECORD)
    store = views.ViewStore(dev, record=record, color=views.u8(color), **floats)
    # the torch route: every view's tensors on the device, one static tensor each
    everything = dict({k: torch.tensor(v, device=dev) for k, v in floats.items()},
                      color=(torch.from_numpy(color) / 255.0).permute(0, 3, 1, 2).contiguous().to(dev), record=torch.tensor(record, device=dev))
    static = {k: torch.zeros_like(v[0]) for k, v in everything.items()}

    def draw(k):
        store.draw(k % VIEWS)

    def copies(k):
        v = k % VIEWS
        for name, s in static.items():
            s.copy_(everything[name][v])

    res = {"H": H, "W": W, "views": VIEWS, "calls": CALLS, "launches_draw": 1, "launches_copies": len(static)}
    same = True
    for v in (3, 0, VIEWS - 1):                          # the routes agree before anything is timed
        draw(v)
        copies(v)
        same = same and torch.equal(store.record, static["record"]) and all(torch.equal(store.current[k], static[k]) for k in store.current)
    res["same_results"] = bool(same)
    moved = lambda read: read + sum(4 * t.numel() for t in static.values())
    res["bytes_draw"] = moved(store.layout.slab_bytes) + 16
    res["bytes_copies"] = moved(sum(4 * t.numel() for t in static.values()))
    graphs = {"draw": captured(draw), "copies": captured(copies)}
    took = {(r, m): [] for r in ("draw", "copies") for m in ("wall_us", "events_us", "graph_us")}
    for fn in (draw, copies):                            # warm-up of the timed shapes
        timed(fn)
    for _ in range(ROUNDS):
        for route, fn in (("draw", draw), ("copies", copies)):
            wall, events = timed(fn)
            took[route, "wall_us"].append(wall)
            took[route, "events_us"].append(events)
            took[route, "graph_us"].append(timed(None, graphs[route])[1])
    for (route, metric), values in took.items():
        res["%s_%s" % (route, metric)] = round(statistics.median(values), 3)
        res["%s_%s_spread" % (route, metric)] = [round(min(values), 3), round(max(values), 3)]
    for route in ("draw", "copies"):
        res["%s_gb_per_s" % route] = round(res["bytes_" + route] / res[route + "_graph_us"] / 1e3, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_views.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS}
    for H, W in SHAPES:
        out["%dx%d" % (W, H)] = measure(H, W, dev)
    print(json.dumps(out), flush=True)
    if opts.out:
        with open(opts.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
