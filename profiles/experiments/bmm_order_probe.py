"""How often does an order of the three products of a 3x3 by 3x1 batch item give torch.bmm's bits?

densify_and_split rotates the children's samples with ``torch.bmm(rots, samples.unsqueeze(-1))``.  The bits of that K = 3 dot
product belong to whichever BLAS solution the installation picks for the batch count, so gft_split_children states an order
of its own; this probe records how often each candidate order (profiles/experiments/bmm_order_probe.hip: six chains of fused
multiply-adds, three pairings of rounded products) meets torch.bmm on rotation matrices of unnormalised quaternions and
samples of the size the split draws, at batch counts {1, 64, 4097, 100003, 900000}.  Nothing asserts equality.

    hipcc --offload-arch=gfx950 -O3 -shared -fPIC profiles/experiments/bmm_order_probe.hip -o profiles/experiments/bmm_order_probe.so
    timeout 300 python profiles/experiments/bmm_order_probe.py --out profiles/bmm_order_probe.json
    python profiles/experiments/bmm_order_probe.py --table profiles/bmm_order_probe.json      # DESIGN.md's table, no device
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SRC, LIB = os.path.join(HERE, "bmm_order_probe.hip"), os.path.join(HERE, "bmm_order_probe.so")
CANDIDATES = ["fma 0,1,2", "fma 0,2,1", "fma 1,0,2", "fma 1,2,0", "fma 2,0,1", "fma 2,1,0", "(p0+p1)+p2", "(p0+p2)+p1", "(p1+p2)+p0"]
SIZES = [1, 64, 4097, 100003, 900000]


def build():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        from gftorf_amd import build as b
        subprocess.check_call([b.hipcc(), "--offload-arch=" + b.ARCH, "-O3", "-shared", "-fPIC", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    lib.bmm_order_candidates.restype = C.c_int
    lib.bmm_order_candidates.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def measure(lib, B, dev):
    import torch
    from gftorf_amd import _lib, densify
    g = torch.Generator().manual_seed(B)
    r = torch.randn((B, 4), generator=g) * torch.pow(10.0, torch.rand((B, 1), generator=g) * 3 - 2)
    R = densify._rotation_matrices(r.to(dev)).contiguous()
    s = (torch.randn((B, 3), generator=g) * torch.exp(torch.randn((B, 3), generator=g) * 0.7) * 0.02).to(dev).contiguous()
    want = torch.bmm(R, s.unsqueeze(-1)).squeeze(-1).contiguous()
    out = torch.empty((len(CANDIDATES), B, 3), device=dev)
    rc = lib.bmm_order_candidates(_lib.raw_stream(dev), B, R.data_ptr(), s.data_ptr(), out.data_ptr())
    if rc:
        raise RuntimeError("bmm_order_candidates failed: %d" % rc)
    torch.cuda.synchronize()
    equal = (out.view(torch.int32) == want.view(torch.int32)[None]).reshape(len(CANDIDATES), -1).float().mean(dim=1).cpu().tolist()
    return {"batch": B, "elements": 3 * B, "share_equal": {c: round(e, 6) for c, e in zip(CANDIDATES, equal)}}


def best(sizes):
    """The candidate with the highest share over all elements; a tie goes to the ascending chain (the first in the list)."""
    total = sum(r["elements"] for r in sizes)
    mean = [sum(r["share_equal"][c] * r["elements"] for r in sizes) / total for c in CANDIDATES]
    return CANDIDATES[max(range(len(CANDIDATES)), key=lambda i: (round(mean[i], 6), -i))], dict(zip(CANDIDATES, (round(m, 6) for m in mean)))


def table(results):
    lines = ["| order | " + " | ".join("B = %d" % r["batch"] for r in results["sizes"]) + " |", "|---|" + "---|" * len(results["sizes"])]
    for c in CANDIDATES:
        lines.append("| %s | " % c + " | ".join("%.4f" % r["share_equal"][c] for r in results["sizes"]) + " |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bmm_order_probe.json"))
    ap.add_argument("--table", help="print DESIGN.md's table from a result file and exit")
    args = ap.parse_args()
    if args.table:
        print(table(json.load(open(args.table))))
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("bmm_order_probe.py needs a HIP device")
    dev = torch.device("cuda:0")
    lib = build()
    sizes = [measure(lib, B, dev) for B in SIZES]
    winner, mean = best(sizes)
    results = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
               "blas": str(torch.backends.cuda.preferred_blas_library()), "sizes": sizes, "share_equal_all_elements": mean, "best": winner}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    print(table(results))
    print("best:", winner)


if __name__ == "__main__":
    main()
