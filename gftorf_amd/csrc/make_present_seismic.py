"""Write gft_present_seismic.h: trunc(255 * seismic(.)) as a table of 257 x 4 bytes (k_present.hip, include/gftorf_present.h).

Usage: python gftorf_amd/csrc/make_present_seismic.py.  Needs matplotlib and numpy; the table is matplotlib's `seismic` colour
map after the reference's tof_to_image, `(255 * cmap(norm(clip(x, -0.5, 0.5)))[..., :3]).astype(uint8)` with
`norm = Normalize(-0.5, 0.5)`.  Rows 0..255 are the map's entries, row 256 is what a NaN gives.  Before it writes, the script
checks on float32 samples that indexing the table as the kernel does -- c = clip(x, -0.5, 0.5), n = c + 0.5f, row
trunc(n * 256f) with 256 taken as 255, row 256 for a NaN -- is what tof_to_image's statements return.
"""
import os

import numpy as np
import matplotlib.pyplot as plt

HERE = os.path.dirname(os.path.abspath(__file__))


def tof_to_image(x):
    """the statements of scene/torf_utils.py:43-50, for any shape"""
    rgb = plt.get_cmap("seismic")(plt.Normalize(-0.5, 0.5)(np.clip(x, -0.5, 0.5)))[..., :3]
    return (255 * rgb).astype(np.uint8)


def table():
    cmap = plt.get_cmap("seismic")
    rows = (255 * cmap(np.arange(256))).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        nan = (255 * cmap(np.array([np.nan], np.float32))).astype(np.uint8)
    return np.concatenate([rows, nan]).astype(np.uint8)


def lookup(t, x):
    """the kernel's indexing, for a float32 array: the RGB bytes"""
    x = np.asarray(x, np.float32)
    half = np.float32(0.5)
    with np.errstate(invalid="ignore"):
        c = np.where(x < -half, -half, np.where(x > half, half, x)).astype(np.float32)
        s = (c + half) * np.float32(256)
        idx = np.where(np.isnan(x), 256, np.where(s >= 256, 255, np.trunc(s))).astype(np.int64)
    return t[idx][..., :3]


def edges():
    """the 257 bin edges of the float32 index in the input's own scale, each with its two float32 neighbours"""
    e = np.arange(0, 257, dtype=np.float32) / np.float32(256) - np.float32(0.5)
    inf = np.float32(np.inf)
    return np.concatenate([e, np.nextafter(e, inf), np.nextafter(e, -inf)]).astype(np.float32)


def main():
    t = table()
    assert t.shape == (257, 4) and t.dtype == np.uint8 and not t[256].any() and (t[:256, 3] == 255).all()
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-1.0, 1.0, 20000).astype(np.float32), edges(),
                        np.array([np.nan, np.inf, -np.inf, 0.5, -0.5, 0.0, -0.0, 3e38, -3e38], np.float32)])
    with np.errstate(invalid="ignore"):
        assert np.array_equal(tof_to_image(x), lookup(t, x))
    lines = ["// gft_present_seismic.h -- trunc(255 * seismic(.)): matplotlib's seismic map as 256 RGBA rows of bytes, then the NaN row.",
             "// Written by make_present_seismic.py from the installed matplotlib; do not edit.",
             "#pragma once",
             "#include <stdint.h>",
             "",
             "#define GFT_SEISMIC_ROWS 257",
             "#define GFT_SEISMIC_TABLE \\"]
    words = ["0x%08xu" % (int(r[0]) | int(r[1]) << 8 | int(r[2]) << 16 | int(r[3]) << 24) for r in t]
    for k in range(0, len(words), 8):
        lines.append("    " + ", ".join(words[k:k + 8]) + ("," if k + 8 < len(words) else "") + " \\")
    lines[-1] = lines[-1][:-2]
    with open(os.path.join(HERE, "gft_present_seismic.h"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote gft_present_seismic.h")


if __name__ == "__main__":
    main()
