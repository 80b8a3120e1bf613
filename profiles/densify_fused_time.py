"""One densify_and_prune event: the composite (gftorf_amd.densify.densify_and_prune, four row surgeries in sequence) against
the fused call (densify_and_prune_fused, one plan and one pass over every tensor), timed in one process.

P = 100 000 and P = 1 000 000 Gaussians of oracle.densify_ref.EagerGaussians (thresholds 0.0002 / 0.005, extent 2.0,
max_screen_size 20: about 6 % of the rows are cloned, 45 % split).  Per size and route 5 warm and 20 timed runs, the routes
alternating, every run on a fresh twin of the same model made outside the timed region and under the same torch generator
state; a run's time is the span between two device events around the whole call, host reads included.  Reported per route:
the median, the launches counted from the call sites of one call (every C entry point of the library times the launches it
makes, and every ATen operator that computes something, counted by a dispatch mode) and torch.cuda.max_memory_allocated over
one call (the model itself included).

A third route, ``fused_kernel_children``, is the fused call with ``children="kernel"`` (the split rows' children from one launch
of gft_split_children instead of the reference's torch statements); its yardstick is the ``fused`` route of the same session:
``kernel_median_below_torch_min`` says whether its median lies below that route's fastest run.  gft_split_children alone is
timed by device events around the call on the model's own split rows (5 warm + 20 timed, preallocated outputs).
profiles/densify_fused_time.json is the record of the two-route script and stays as it is; this one writes
profiles/densify_children_time.json.

    timeout 900 python profiles/densify_fused_time.py --out profiles/densify_children_time.json
    python profiles/densify_fused_time.py --table profiles/densify_children_time.json     # the tables of DESIGN.md, no device
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN_SIZE = 0.0002, 0.005, 2.0, 20
WARM, TIMED = 5, 20
# launches behind one call of a C entry point (csrc/k_densify.hip)
ENTRY_LAUNCHES = {"gft_rows_rank": 3, "gft_rows_gather": 1, "gft_densify_classify": 3, "gft_densify_layout": 3, "gft_rows_remap": 1,
                  "gft_split_children": 1}
# ATen operators that launch nothing: views, allocations, metadata
NO_LAUNCH = ("view", "reshape", "squeeze", "unsqueeze", "detach", "alias", "empty", "as_strided", "slice", "select", "expand",
             "_unsafe_view", "t.", "transpose", "permute", "is_", "size", "stride", "numel", "_local_scalar_dense", "lift_fresh",
             "requires_grad_", "set_")


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.ops = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func.__name__
        if not name.startswith(NO_LAUNCH):
            self.ops += 1
        return func(*args, **(kwargs or {}))


class CountEntries:
    """Stands in for the loaded library: counts the launches behind every entry point that is called."""

    def __init__(self, lib):
        self.lib, self.launches, self.reads = lib, 0, 0

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in ENTRY_LAUNCHES:
            return fn

        def counted(*a):
            self.launches += ENTRY_LAUNCHES[name]
            self.reads += name in ("gft_rows_rank", "gft_densify_classify", "gft_densify_layout")
            return fn(*a)
        return counted


def count_launches(route, model):
    from gftorf_amd import _lib
    real = _lib.load()
    proxy = CountEntries(real)
    _lib._lib = proxy
    try:
        with CountOps() as ops:
            route(model)
    finally:
        _lib._lib = real
    return dict(library_launches=proxy.launches, aten_operators=ops.ops, launches=proxy.launches + ops.ops, host_reads=proxy.reads)


def measure(P, dev):
    from gftorf_amd import densify
    from oracle import densify_ref
    base = densify_ref.EagerGaussians(P, dev, seed=5)
    routes = {"composite": lambda m: densify.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN_SIZE),
              "fused": lambda m: densify.densify_and_prune_fused(m, MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN_SIZE),
              "fused_kernel_children": lambda m: densify.densify_and_prune_fused(m, MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN_SIZE,
                                                                                 children="kernel")}
    times = {name: [] for name in routes}
    rows_after = {}
    for run in range(WARM + TIMED):
        for name, route in routes.items():
            m = base.twin()
            torch.manual_seed(run)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            route(m)
            b.record()
            torch.cuda.synchronize()
            if run >= WARM:
                times[name].append(a.elapsed_time(b))
            rows_after[name] = int(m._xyz.shape[0])
            del m
    out = {"P": P, "rows_after": rows_after["fused"]}
    assert rows_after["fused"] == rows_after["composite"] == rows_after["fused_kernel_children"]
    for name, route in routes.items():
        m = base.twin()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        torch.manual_seed(0)
        route(m)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        del m
        m = base.twin()
        torch.manual_seed(0)
        try:
            counts = count_launches(route, m)
        except Exception as e:                      # the times stand without the counts
            counts = dict(library_launches=-1, aten_operators=-1, launches=-1, host_reads=-1, count_error=repr(e))
        del m
        out[name] = dict(median_ms=round(statistics.median(times[name]), 3), min_ms=round(min(times[name]), 3),
                         max_ms=round(max(times[name]), 3), runs=len(times[name]), peak_bytes=peak, model_bytes=before, **counts)
    out["fused_over_composite"] = round(out["fused"]["median_ms"] / out["composite"]["median_ms"], 3)
    out["kernel_children_over_fused"] = round(out["fused_kernel_children"]["median_ms"] / out["fused"]["median_ms"], 3)
    out["kernel_median_below_torch_min"] = out["fused_kernel_children"]["median_ms"] < out["fused"]["min_ms"]
    out["split_children_alone"] = kernel_alone(base, dev)
    return out


def kernel_alone(base, dev, N=2):
    """gft_split_children on the model's own split rows, device events around the call."""
    from gftorf_amd import _lib
    lib = _lib.load()
    grads = base.xyz_gradient_accum / base.denom
    grads[grads.isnan()] = 0.0
    scaling = base.get_scaling.detach().contiguous()
    mask = (grads.reshape(-1) >= MAX_GRAD) & (scaling.max(dim=1).values > base.percent_dense * EXTENT)
    rows = mask.nonzero().reshape(-1).to(torch.int32).contiguous()
    P, S = int(mask.numel()), int(rows.numel())
    z = torch.randn((N * S, 3), device=dev)
    new_xyz = torch.empty((N * S, 3), device=dev)
    xyz, rot = base._xyz.detach().contiguous(), base._rotation.detach().contiguous()
    times = []
    for run in range(WARM + TIMED):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(lib.gft_split_children(_lib.raw_stream(dev), P, S, N, rows.data_ptr(), xyz.data_ptr(), rot.data_ptr(),
                                          scaling.data_ptr(), z.data_ptr(), new_xyz.data_ptr()))
        b.record()
        torch.cuda.synchronize()
        if run >= WARM:
            times.append(a.elapsed_time(b) * 1e3)
    moved = S * (4 + 12 + 16 + 12) + N * S * (12 + 12)
    med = statistics.median(times)
    return dict(S=S, N=N, median_us=round(med, 1), min_us=round(min(times), 1), max_us=round(max(times), 1), bytes=moved,
                gb_per_s=round(moved / med / 1e3, 1))


def table(results):
    lines = ["| P | composite: median, launches, peak | fused: median, launches, peak | fused / composite |",
             "|---|---|---|---|"]
    cell = lambda r: "%.2f ms, %d (%d library + %d ATen), %.2f GB" % (r["median_ms"], r["launches"], r["library_launches"],
                                                                       r["aten_operators"], r["peak_bytes"] / 1e9)
    for r in results["sizes"]:
        lines.append("| %d -> %d | %s | %s | %.2f |" % (r["P"], r["rows_after"], cell(r["composite"]), cell(r["fused"]),
                                                        r["fused_over_composite"]))
    if all("fused_kernel_children" in r for r in results["sizes"]):
        lines += ["", "| P | fused, children=\"torch\": median (min) | children=\"kernel\": median, launches, peak | kernel / torch | "
                      "gft_split_children alone |", "|---|---|---|---|---|"]
        for r in results["sizes"]:
            k = r["split_children_alone"]
            lines.append("| %d -> %d | %.2f ms (%.2f) | %s | %.2f | S = %d: %.1f us, %.0f MB, %.0f GB/s |"
                         % (r["P"], r["rows_after"], r["fused"]["median_ms"], r["fused"]["min_ms"], cell(r["fused_kernel_children"]),
                            r["kernel_children_over_fused"], k["S"], k["median_us"], k["bytes"] / 1e6, k["gb_per_s"]))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_children_time.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--table", help="print DESIGN.md's table from a result file and exit")
    args = ap.parse_args()
    if args.table:
        print(table(json.load(open(args.table))))
        return
    if not torch.cuda.is_available():
        sys.exit("densify_fused_time.py needs a HIP device")
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "thresholds": [MAX_GRAD, MIN_OPACITY, EXTENT, MAX_SCREEN_SIZE],
               "warm": WARM, "timed": TIMED, "sizes": [measure(P, dev) for P in args.sizes]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print(table(results))


if __name__ == "__main__":
    main()
