"""Write gft_present_magma.h: to8b(cm.magma(.)) as a table of 257 x 4 bytes (k_present.hip, include/gftorf_present.h).

Usage: python gftorf_amd/csrc/make_present_magma.py.  Needs matplotlib and numpy; the table is matplotlib's colour map data
after the reference's to8b, `(255 * clip(x, 0, 1)).astype(uint8)`.  Rows 0..255 are the map's entries, row 256 is what a NaN
gives.  Before it writes, the script checks on float32 samples that indexing the table as the kernel does -- row
trunc(x * 256f) clamped to 255, row 0 below 0, row 256 for a NaN -- is what cm.magma itself returns.
"""
import os

import numpy as np
from matplotlib import cm

HERE = os.path.dirname(os.path.abspath(__file__))


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def table():
    rows = to8b(cm.magma(np.arange(256)))
    with np.errstate(invalid="ignore"):
        nan = to8b(cm.magma(np.array([np.nan], np.float32)))
    return np.concatenate([rows, nan]).astype(np.uint8)


def lookup(t, x):
    """the kernel's indexing, for a float32 array"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = x * np.float32(256)
        idx = np.where(np.isnan(x), 256, np.where(x < 0, 0, np.where(s >= 256, 255, np.trunc(s)))).astype(np.int64)
    return t[idx]


def main():
    t = table()
    assert t.shape == (257, 4) and t.dtype == np.uint8 and not t[256].any() and (t[:256, 3] == 255).all()
    rng = np.random.default_rng(0)
    edges = np.arange(-2, 259, dtype=np.float32) / np.float32(256)
    inf = np.float32(np.inf)
    x = np.concatenate([rng.uniform(-0.5, 1.5, 20000).astype(np.float32), edges, np.nextafter(edges, inf), np.nextafter(edges, -inf),
                        np.array([np.nan, np.inf, -np.inf, 1.0, 0.0, -0.0, 3e38, -3e38], np.float32)])
    with np.errstate(invalid="ignore"):
        assert np.array_equal(to8b(cm.magma(x)), lookup(t, x))
    lines = ["// gft_present_magma.h -- to8b(cm.magma(.)): matplotlib's magma map as 256 RGBA rows of bytes, then the NaN row.",
             "// Written by make_present_magma.py from the installed matplotlib; do not edit.",
             "#pragma once",
             "#include <stdint.h>",
             "",
             "#define GFT_MAGMA_ROWS 257",
             "#define GFT_MAGMA_TABLE \\"]
    words = ["0x%08xu" % (int(r[0]) | int(r[1]) << 8 | int(r[2]) << 16 | int(r[3]) << 24) for r in t]
    for k in range(0, len(words), 8):
        lines.append("    " + ", ".join(words[k:k + 8]) + ("," if k + 8 < len(words) else "") + " \\")
    lines[-1] = lines[-1][:-2]
    with open(os.path.join(HERE, "gft_present_magma.h"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote gft_present_magma.h")


if __name__ == "__main__":
    main()
