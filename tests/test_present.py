"""gftorf_amd.present: a rendered view's display images (render.py:105-189, :43-54; scene/torf_utils.py:11-29, 53-57;
utils/graphics_utils.py:117-137; matplotlib's cm.magma).  The yardsticks are the reference's own bytes
(tests/golden/present.npz, written by tests/golden/make_golden_present.py from the reference's functions and cm.magma) and
`view_np` below, the same statements restated in numpy float32.

Every statement except arctan2 is a fixed sequence of IEEE float32 operations, so every uint8 image and depth_norm_f must be
bit-equal.  The device's atan2f may differ from numpy's by a few ulp of 2 pi (about 1e-6 rad); disp * 256 = 36.4 * phase, so that
moves a pixel by about 4e-5 of a colour-map bin.  `draw_view` therefore nudges every phasor pixel until (`conditioned`)
  - the float64 disp * 256 is at least 1e-3 from an integer,
  - the wrapped phase lies in [0.05, 2 pi - 0.05],
  - float32 and float64 take the same `+ 2 pi` branch,
and asserts all three for every pixel; no pixel is left out of a comparison.  depth_tof_f is compared with the float64
restatement at three times the reference's own float32 distance from it (`ref_err_depth_tof` of the fixture, relative to
depth_range), the margin tests/test_metrics.py gives the reference's own error.  The other inputs need no conditioning and
deliberately hold values on bin edges and outside [0, 1].
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_present.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "present.npz")
IMAGES = ("color", "real", "imag", "amp", "quad", "depth", "depth_tof", "depth_norm", "dd", "depth_tof_f", "depth_norm_f")
INPUTS = ("image", "phasor", "depth", "acc", "dd")
# name: (H, W, phasor planes, tof_multiplier, phase_offset, depth_range, which inputs)
CASES = {"plain": (12, 16, 3, 1.0, 0.0, 10.0, INPUTS), "quad": (19, 27, 7, 2.0, 0.3, 7.5, INPUTS),
         "tofcam": (5, 7, 0, 1.0, 0.0, 10.0, ("depth", "acc"))}
HAS_COLOR, HAS_PHASOR, HAS_QUAD, HAS_DEPTH, HAS_ACC, HAS_DD = 1, 2, 4, 8, 16, 32
TWO_PI = 2 * np.pi


def f32(x):
    """the float32 the device is handed for a Python number, as a float"""
    return float(np.float32(x))


# ---- the restatement ---------------------------------------------------------------------------------------------------

def zplanes_np(depth_range):
    """render.py:54 with the camera's 0-d float32 depth_range"""
    r = np.array(depth_range, dtype=np.float32)
    return 0.05 * r * 0.9, 0.55 * r * 1.1


def to8b_np(x):
    """torf_utils.py:11-12"""
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def normalize_np(im, lo, hi):
    """torf_utils.py:21-29 with the bounds given: float32 throughout"""
    with np.errstate(invalid="ignore", divide="ignore"):
        im = (im - lo) / (hi - lo)
    im[np.isnan(im)] = 0.
    return np.clip(im, 0, 1)


def red_blue_np(plane):
    """graphics_utils.py:125-137 for one [H, W] plane: [H, W, 3] with the positive part in red, nothing in green and the
    negated negative part in blue (-0.0 where there is none, NaN where the plane is NaN)"""
    zero = np.zeros_like(plane)
    return np.stack([np.where(plane <= 0, zero, plane), zero, -np.where(plane >= 0, zero, plane)], axis=-1)


def depth_from_tof_np(phasor, depth_range, phase_offset, dtype=np.float32):
    """torf_utils.py:53-57 on planes 0 and 1, every step in `dtype`; no clamp of the real part"""
    re, im = phasor[0].astype(dtype), phasor[1].astype(dtype)
    tof_phase = np.arctan2(im, re)
    tof_phase = tof_phase - dtype(phase_offset)
    tof_phase = np.where(tof_phase < 0, tof_phase + dtype(TWO_PI), tof_phase)
    return tof_phase * dtype(depth_range) / dtype(4 * np.pi)


def magma_np(table, x):
    """to8b(cm.magma(x)) of a float32 array through the 257 x 4 table: matplotlib's index is trunc(x * 256) in float32, below
    0 the first entry, from 256 on (x == 1 too) the last, a NaN row 256"""
    assert x.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        s = x * np.float32(256)
        row = np.where(np.isnan(x), 256, np.where(x < 0, 0, np.where(s >= 256, 255, np.trunc(s))))
    return table[row.astype(np.int64)]


def disp_np(d, znear, zfar):
    """render.py:148, 155, 162 in float32"""
    assert d.dtype == np.float32
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1 - (d - np.float32(znear)) / (np.float32(zfar) - np.float32(znear))


def view_np(v, table):
    """render.py:129-184 for one view in numpy float32: `v` holds the float32 inputs present (`image` [3, H, W], `phasor`
    [C, H, W], `depth`, `acc`, `dd` [1, H, W]), `ranges` (6), `znear`, `zfar`, `depth_range`, `phase_offset`, `tof_multiplier`.
    Returns the images of IMAGES that the inputs produce."""
    out = {}
    if "image" in v:
        out["color"] = to8b_np(v["image"].transpose(1, 2, 0))                                   # :174-177
    if "phasor" in v:
        rg = np.asarray(v["ranges"], np.float32)
        scaled = v["phasor"][:3] * np.float32(v["tof_multiplier"])                              # :132
        out["real"] = to8b_np(normalize_np(red_blue_np(scaled[0]), rg[0], rg[1]))               # :137-139
        out["imag"] = to8b_np(normalize_np(red_blue_np(scaled[1]), rg[2], rg[3]))
        out["amp"] = to8b_np(normalize_np(scaled[2].copy(), rg[4], rg[5]))
        if v["phasor"].shape[0] == 7:
            out["quad"] = to8b_np(np.abs(v["phasor"][3:]))                                      # :142-144
        d = depth_from_tof_np(v["phasor"], v["depth_range"], v["phase_offset"])                 # :146
        out["depth_tof_f"] = d
        out["depth_tof"] = magma_np(table, disp_np(d, v["znear"], v["zfar"]))                   # :148-150
    if "depth" in v:
        out["depth"] = magma_np(table, disp_np(v["depth"][0], v["znear"], v["zfar"]))           # :153-157
        if "acc" in v:
            with np.errstate(invalid="ignore", divide="ignore"):
                dn = v["depth"][0] / v["acc"][0]                                                # :160
            out["depth_norm_f"] = dn
            out["depth_norm"] = magma_np(table, disp_np(dn, v["znear"], v["zfar"]))             # :162-164
    if "dd" in v:
        im = v["dd"][0]
        out["dd"] = to8b_np(normalize_np(im.copy(), np.min(im), np.max(im)))                    # :180-183
    return out


def ranges_np(gt_tofs):
    """render.py:46-47, 61: np.min / np.max over the sequence of red / blue images and amplitudes"""
    reals, imags, amps = [red_blue_np(g[0]) for g in gt_tofs], [red_blue_np(g[1]) for g in gt_tofs], [g[2] for g in gt_tofs]
    return np.array([f(seq) for seq in (reals, imags, amps) for f in (np.min, np.max)], np.float32)


# ---- inputs -------------------------------------------------------------------------------------------------------------

def conditioned(phasor, depth_range, phase_offset, znear, zfar):
    """[H, W] bool: the pixels at which depth_tof's colour does not hang on the last bits of arctan2 (the module docstring)"""
    off = np.float32(phase_offset)
    p64 = np.arctan2(phasor[1].astype(np.float64), phasor[0].astype(np.float64)) - np.float64(off)
    p32 = np.arctan2(phasor[1], phasor[0]) - off
    w64 = np.where(p64 < 0, p64 + TWO_PI, p64)
    d64 = w64 * np.float64(np.float32(depth_range)) / (4 * np.pi)
    zn, zf = np.float64(np.float32(znear)), np.float64(np.float32(zfar))
    s = (1 - (d64 - zn) / (zf - zn)) * 256
    return (np.abs(s - np.round(s)) >= 1e-3) & (w64 >= 0.05) & (w64 <= TWO_PI - 0.05) & ((p64 < 0) == (p32 < 0))


def draw_view(rng, H, W, planes, depth_range=10.0, phase_offset=0.0, tof_multiplier=1.0, inputs=INPUTS):
    """Every input of one view as float32 (read-only): `image` with values outside [0, 1] and on multiples of 1 / 255;
    a `planes`-plane `phasor` whose planes 0 / 1 are conditioned as the module docstring says (asserted for every pixel), the
    others in [-1.3, 1.3]; `depth` from below znear to beyond zfar with pixels exactly on both; `acc` in [0.2, 1]; `dd`;
    ranges that clip part of real, imag and amp; znear / zfar of render.py:54."""
    znear, zfar = zplanes_np(depth_range)
    v = dict(depth_range=np.float32(depth_range), phase_offset=np.float32(phase_offset), tof_multiplier=np.float32(tof_multiplier),
             znear=np.float32(znear), zfar=np.float32(zfar))
    n = H * W
    if "image" in inputs:
        im = rng.uniform(-0.2, 1.2, size=(3, H, W))
        edge = rng.random((3, H, W)) < 0.25
        im[edge] = rng.integers(0, 256, size=int(edge.sum())) / 255.0
        v["image"] = im.astype(np.float32)
    if "phasor" in inputs and planes:
        ph = rng.uniform(-1.3, 1.3, size=(planes, H, W)).astype(np.float32)
        todo = np.ones((H, W), bool)
        for _ in range(200):
            k = int(todo.sum())
            if not k:
                break
            theta = rng.uniform(0.06, TWO_PI - 0.06, size=k) + f32(phase_offset)
            length = rng.uniform(0.05, 1.0, size=k)
            ph[0][todo], ph[1][todo] = (length * np.cos(theta)).astype(np.float32), (length * np.sin(theta)).astype(np.float32)
            todo = ~conditioned(ph, depth_range, phase_offset, znear, zfar)
        assert conditioned(ph, depth_range, phase_offset, znear, zfar).all()
        ph[2] = rng.uniform(0.02, 1.0, size=(H, W)).astype(np.float32)
        v["phasor"] = ph
        v["ranges"] = np.array([0.0, 0.8, 0.0, 0.7, 0.1, 0.9], np.float32) * np.float32(tof_multiplier)
    if "depth" in inputs:
        d = rng.uniform(0.0, 0.7 * depth_range, size=n).astype(np.float32)
        if n >= 4:
            d[rng.permutation(n)[:2]] = (np.float32(znear), np.float32(zfar))
        v["depth"] = d.reshape(1, H, W)
    if "acc" in inputs:
        v["acc"] = rng.uniform(0.2, 1.0, size=(1, H, W)).astype(np.float32)
    if "dd" in inputs:
        v["dd"] = rng.uniform(0.0, 3.0, size=(1, H, W)).astype(np.float32)
    for a in v.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def make_view(H, W, planes=7, tof_multiplier=2.0, phase_offset=0.3, depth_range=7.5):
    return draw_view(np.random.default_rng(1000 * H + W + planes), H, W, planes, depth_range, phase_offset, tof_multiplier)


@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    out = {c: {k[len(c) + 1:]: z[k] for k in z.files if k.startswith(c + "_")} for c in CASES}
    out["magma_u8"], out["ref_err_depth_tof"] = z["magma_u8"], float(z["ref_err_depth_tof"])
    return out


def golden_inputs(g):
    keys = INPUTS + ("ranges", "znear", "zfar", "depth_range", "phase_offset", "tof_multiplier")
    return {k: g[k] for k in keys if k in g}


_NP = {}


def reference_np(key, v, table):
    """`view_np`, computed once per input set and shared"""
    if key not in _NP:
        _NP[key] = view_np(v, table)
    return _NP[key]


def kwargs_on(dev, v, **over):
    """the keyword arguments of view_images for the inputs `v`"""
    kw = {k: torch.tensor(np.ascontiguousarray(v[k]), device=dev) for k in INPUTS if k in v}
    if "phasor" in v:
        kw.update(ranges=[float(x) for x in v["ranges"]], depth_range=float(v["depth_range"]), phase_offset=float(v["phase_offset"]),
                  tof_multiplier=float(v["tof_multiplier"]))
    if "phasor" in v or "depth" in v:
        kw["zplanes"] = (float(v["znear"]), float(v["zfar"]))
    kw.update(over)
    return kw


def check_images(got, want, v, ref_err, what):
    """a dict of device tensors (or numpy arrays) against `view_np`'s (or the fixture's): keys, shapes, dtypes; every uint8 image
    and depth_norm_f bit-equal; depth_tof_f against the float64 restatement"""
    got = {k: (t.cpu().numpy() if isinstance(t, torch.Tensor) else t) for k, t in got.items()}
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in IMAGES:
        if k not in want:
            continue
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].shape, got[k].dtype)
        if k == "depth_tof_f":
            d64 = depth_from_tof_np(v["phasor"], f32(v["depth_range"]), f32(v["phase_offset"]), np.float64)
            err, bound = float(np.abs(got[k] - d64).max()), 3 * ref_err * f32(v["depth_range"])
            print("%s depth_tof_f: err %.3g bound %.3g" % (what, err, bound))
            assert err <= bound, (what, err, bound)
        elif k == "depth_norm_f":
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k)
        else:
            bad = np.argwhere(got[k] != want[k])
            assert not len(bad), (what, k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


# ---- CPU-runnable checks ------------------------------------------------------------------------------------------------

def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c_and_every_symbol_is_exported(tmp_path, lib):
    from gftorf_amd import _lib, build, present
    import gftorf_amd
    names = declared_functions()
    assert set(names) == set(_lib.PRESENT_EXPORTS), names
    assert not set(names) & (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.FEATURE_EXPORTS) | set(_lib.REG_EXPORTS) |
                             set(_lib.TOF_EXPORTS) | set(_lib.QUERY_EXPORTS) | set(_lib.METRICS_EXPORTS))
    for n in names:
        assert hasattr(lib, n), n
    assert "k_present.hip" in build.SOURCES and gftorf_amd.present is present
    assert "struct" not in re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    prog = tmp_path / "present_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_present.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "present_abi.o")])
    # the header's constants are the Python side's
    words = (["GFT_PRESENT_" + k.upper() for k in IMAGES] +
             ["GFT_PRESENT_" + k for k in ("IMAGES", "HAS_COLOR", "HAS_PHASOR", "HAS_QUAD", "HAS_DEPTH", "HAS_ACC", "HAS_DD", "ALIGN",
                                           "PARTIAL_WORDS", "RANGE_WORDS", "MAGMA_ROWS")])
    out = subprocess.check_output(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-include", "gftorf_present.h",
                                   "-x", "c", "-"], input="PRESENT_WORDS_ARE " + " ".join(words) + "\n", text=True)
    consts = [int(x) for x in out.split("PRESENT_WORDS_ARE", 1)[1].split()]
    assert consts == list(range(11)) + [11, HAS_COLOR, HAS_PHASOR, HAS_QUAD, HAS_DEPTH, HAS_ACC, HAS_DD, _lib.PRESENT_ALIGN,
                                        _lib.PRESENT_PARTIAL_WORDS, _lib.PRESENT_RANGE_WORDS, _lib.PRESENT_MAGMA_ROWS]
    assert tuple(n for n, _, _, _ in _lib.PRESENT_IMAGES) == IMAGES == present.IMAGES
    assert (_lib.PRESENT_HAS_COLOR, _lib.PRESENT_HAS_PHASOR, _lib.PRESENT_HAS_QUAD, _lib.PRESENT_HAS_DEPTH, _lib.PRESENT_HAS_ACC,
            _lib.PRESENT_HAS_DD) == (1, 2, 4, 8, 16, 32)
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16


def test_the_colour_table_is_the_fixtures(lib, golden):
    from gftorf_amd import present
    table = present.magma_table()
    assert table.shape == (257, 4) and table.dtype == np.uint8 and np.array_equal(table, golden["magma_u8"])
    assert not table[256].any() and (table[:256, 3] == 255).all()


def test_the_numpy_statements_give_the_reference_bytes(golden):
    """`view_np` against what the reference's own functions and cm.magma wrote into the fixture: every image exactly, the
    float32 ToF depth too (both are numpy on the CPU), and that depth within ref_err_depth_tof of the float64 restatement"""
    assert 0 < golden["ref_err_depth_tof"] < 4e-7                  # a float32 result's error, not a disagreement
    for c, (H, W, planes, mult, off, dr, inputs) in CASES.items():
        g = golden[c]
        v = golden_inputs(g)
        assert set(k for k in INPUTS if k in v) == set(inputs) and v[inputs[0]].shape[1:] == (H, W), c
        assert ("phasor" not in v or v["phasor"].shape[0] == planes) and f32(g["tof_multiplier"]) == mult and abs(f32(g["phase_offset"]) - off) < 1e-6
        assert (f32(g["znear"]), f32(g["zfar"])) == tuple(float(z) for z in zplanes_np(g["depth_range"]))
        out = view_np(v, golden["magma_u8"])
        want = {k: g["out_" + k] for k in IMAGES if "out_" + k in g}
        assert set(out) == set(want), (c, sorted(out), sorted(want))
        for k in want:
            assert out[k].dtype == want[k].dtype and out[k].shape == want[k].shape, (c, k)
            assert np.array_equal(out[k], want[k], equal_nan=(want[k].dtype == np.float32)), (c, k)
        if "phasor" in v:
            assert conditioned(v["phasor"], g["depth_range"], g["phase_offset"], g["znear"], g["zfar"]).all()
            d64 = depth_from_tof_np(v["phasor"], f32(g["depth_range"]), f32(g["phase_offset"]), np.float64)
            assert np.abs(out["depth_tof_f"] - d64).max() <= golden["ref_err_depth_tof"] * f32(g["depth_range"])
    assert set(golden["plain"]) >= {"out_" + k for k in IMAGES if k != "quad"} and "out_quad" not in golden["plain"]
    assert set(k[4:] for k in golden["tofcam"] if k.startswith("out_")) == {"depth", "depth_norm", "depth_norm_f"}
    assert golden["quad"]["out_quad"].shape == (4, 19, 27)


def test_size_and_layout_queries(lib):
    import ctypes as C
    from gftorf_amd import _lib, present
    assert present.blocks(0) == 0 and lib.gft_present_blocks(-3) == 0
    assert present.blocks(1) == 1 and present.blocks(256) == 1 and present.blocks(257) == 2 and present.blocks(513) == 3
    assert present.blocks(640 * 480) == 1024 == present.blocks(1 << 40)
    every = HAS_COLOR | HAS_PHASOR | HAS_QUAD | HAS_DEPTH | HAS_ACC | HAS_DD
    bpp = dict(zip(IMAGES, (3, 3, 3, 1, 4, 4, 4, 4, 1, 4, 4)))
    for H, W in ((1, 1), (5, 7), (19, 27), (480, 640)):
        total, off = present.sheet_layout(H, W, every)
        assert tuple(off) == IMAGES and off["color"] == 0 and total % 16 == 0
        ends = [off[k] + bpp[k] * H * W for k in IMAGES]
        assert all(o % 16 == 0 for o in off.values())
        assert all(0 <= nxt - end < 16 for end, nxt in zip(ends, [off[k] for k in IMAGES[1:]] + [total]))
        # absent groups shrink the sheet: each group's images leave, the others close up
        for groups, names in ((HAS_COLOR, ("color",)), (HAS_DEPTH, ("depth",)), (HAS_DEPTH | HAS_ACC, ("depth", "depth_norm", "depth_norm_f")),
                              (HAS_DD, ("dd",)), (HAS_PHASOR, ("real", "imag", "amp", "depth_tof", "depth_tof_f")),
                              (HAS_PHASOR | HAS_QUAD | HAS_DD, ("real", "imag", "amp", "quad", "depth_tof", "dd", "depth_tof_f"))):
            t, o = present.sheet_layout(H, W, groups)
            assert tuple(o) == names and t < total and t == sum((bpp[k] * H * W + 15) // 16 * 16 for k in names)
    offs = (C.c_int64 * 11)()
    for bad in ((0, 4, every), (4, 0, every), (4, 4, 0), (4, 4, 64), (4, 4, HAS_QUAD), (4, 4, HAS_ACC), (4, 4, -1)):
        assert lib.gft_present_sheet_bytes(*bad, offs) == 0, bad
    assert lib.gft_present_sheet_bytes(4, 4, HAS_COLOR, None) == 48
    x = C.c_void_p(16)                                         # never dereferenced: the calls fail before any launch
    six = (C.c_float * 6)(0, 1, 0, 1, 0, 1)

    def view(H=4, W=4, im=x, ph=x, planes=3, d=x, a=x, dd=x, rg=six, stride=16, part=x, sheet=x):
        return lib.gft_present_view(None, H, W, im, stride, ph, stride, planes, d, a, dd, None, rg, None, 7.5, None, 0.0, 0.3, 4.5, 1.0, part, sheet)
    for bad, msg in ((dict(H=0), "bad size"), (dict(W=-1), "bad size"), (dict(im=None, ph=None, planes=0, d=None, a=None, dd=None), "no image"),
                     (dict(planes=2), "at least 3 planes"), (dict(ph=None), "at least 3 planes"), (dict(d=None), "acc without depth"),
                     (dict(rg=None), "phasor without ranges"), (dict(stride=-1), "bad plane stride"), (dict(part=None), "dd needs partials"),
                     (dict(sheet=None), "sheet is NULL"), (dict(sheet=C.c_void_p(24)), "16-byte aligned")):
        assert view(**bad) != 0, bad
        assert msg in _lib.last_error(), (bad, _lib.last_error())
    assert lib.gft_present_ranges(None, 0, x, 4, x, x) != 0 and "bad size" in _lib.last_error()
    assert lib.gft_present_ranges(None, 4, None, 4, x, x) != 0 and "NULL" in _lib.last_error()
    assert lib.gft_present_ranges(None, 4, x, 4, None, x) != 0 and "partials" in _lib.last_error()
    assert lib.gft_present_ranges_reset(None, None) != 0 and "NULL" in _lib.last_error()
    assert present.zplanes(7.5) == tuple(float(z) for z in zplanes_np(7.5)) == (f32(f32(f32(0.05) * 7.5) * f32(0.9)), f32(f32(f32(0.55) * 7.5) * f32(1.1)))


def test_wrapper_rejects_bad_arguments_before_any_launch(lib, monkeypatch):
    from gftorf_amd import present
    im, ph, d = torch.rand(3, 4, 6), torch.rand(7, 4, 6), torch.rand(1, 4, 6)
    full = dict(ranges=[0, 1, 0, 1, 0, 1], zplanes=(0.3, 4.5), depth_range=7.5)

    class NoLaunch:
        def __getattr__(self, name):
            real = getattr(lib, name)
            assert name not in ("gft_present_view", "gft_present_ranges"), name
            return real
    monkeypatch.setattr(present._lib, "load", lambda: NoLaunch())
    for c in (lambda: present.view_images(image=im), lambda: present.view_images(phasor=ph, depth=d, acc=d, dd=d, **full),
              lambda: present.view_images(depth=d, zplanes=(0.3, 4.5)), lambda: present.PhasorRanges(device="cpu")):
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            c()
    for c, msg in [(lambda: present.view_images(image=torch.rand(4, 4, 6)), r"image must be \[3, H, W\]"),
                   (lambda: present.view_images(image=im[0]), r"image must be \[3, H, W\]"),
                   (lambda: present.view_images(phasor=ph[:2], **full), r"phasor must be \[>=3, H, W\]"),
                   (lambda: present.view_images(image=im, depth=d[:, :, :5], zplanes=(0.3, 4.5)), "depth is 4 x 5, image 4 x 6: the inputs of one call have one size"),
                   (lambda: present.view_images(depth=d, acc=d[:, :3], zplanes=(0.3, 4.5)), "acc is 3 x 6, depth 4 x 6"),
                   (lambda: present.view_images(depth=ph[:2], zplanes=(0.3, 4.5)), r"depth must be \[1, H, W\]"),
                   (lambda: present.view_images(phasor=ph[:5], quad=True, **full), "quad needs a phasor of exactly 7 planes"),
                   (lambda: present.view_images(image=im, quad=True), "quad needs a phasor of exactly 7 planes, got none"),
                   (lambda: present.view_images(phasor=ph, **dict(full, ranges=[0, 1, 0, 1])), "ranges must be six numbers"),
                   (lambda: present.view_images(phasor=ph, **dict(full, ranges=torch.zeros(5))), "ranges must be six numbers"),
                   (lambda: present.view_images(phasor=ph, **dict(full, depth_range=torch.ones(2))), "depth_range must be a number or a one-element")]:
        with pytest.raises(RuntimeError, match=msg):
            c()
    for c, msg in [(lambda: present.view_images(acc=d, zplanes=(0.3, 4.5)), "acc is given without depth"),
                   (lambda: present.view_images(phasor=ph, zplanes=(0.3, 4.5), depth_range=7.5), "need ranges"),
                   (lambda: present.view_images(phasor=ph, ranges=[0, 1] * 3, zplanes=(0.3, 4.5)), "needs depth_range"),
                   (lambda: present.view_images(phasor=ph, ranges=[0, 1] * 3, depth_range=7.5), "needs zplanes"),
                   (lambda: present.view_images(depth=d), "needs zplanes"),
                   (lambda: present.view_images(), "nothing to show"),
                   (lambda: present.ViewSheets(slots=0), "at least one slot")]:
        with pytest.raises(ValueError, match=msg):
            c()
    with pytest.raises(TypeError, match="image must be a tensor"):
        present.view_images(image=im.numpy())
    with pytest.raises(TypeError, match="dd must be torch.float32"):
        present.view_images(dd=d.double())
    with pytest.raises(TypeError, match="ranges must be torch.float32"):
        present.view_images(phasor=ph, **dict(full, ranges=torch.zeros(6, dtype=torch.float64)))


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def three_block_shape():
    """the smallest pixel count with three workgroups, as H x W with the smallest odd W > 1 that divides it"""
    from gftorf_amd import present
    n = next(n for n in range(1, 1 << 20) if present.blocks(n) >= 3)
    W = next(w for w in range(3, n + 1, 2) if n % w == 0)
    return n // W, W


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (19, 27), (37, 53), "three-blocks"], ids=str)
def test_view_images_matches_the_numpy_statements(shape, gpu, golden):
    from gftorf_amd import present
    H, W = three_block_shape() if shape == "three-blocks" else shape
    if shape == "three-blocks":
        assert W % 2 == 1 and present.blocks(H * W) >= 3 and present.blocks(H * W - 1) < 3
    v = make_view(H, W)
    got = present.view_images(**kwargs_on(gpu, v))
    assert all(t.device.type == "cuda" and not t.requires_grad for t in got.values())
    base = min(t.data_ptr() for t in got.values())
    assert base % 16 == 0 and all((t.data_ptr() - base) % 16 == 0 for t in got.values()) and got["color"].data_ptr() == base
    check_images(got, reference_np((H, W), v, golden["magma_u8"]), v, golden["ref_err_depth_tof"], "%dx%d" % (H, W))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_fixture_cases_give_the_reference_bytes(case, gpu, golden):
    from gftorf_amd import present
    g = golden[case]
    v = golden_inputs(g)
    got = present.view_images(**kwargs_on(gpu, v))
    check_images(got, {k: g["out_" + k] for k in IMAGES if "out_" + k in g}, v, golden["ref_err_depth_tof"], case)


@pytest.mark.gpu
def test_special_values(gpu, golden):
    """hand-placed pixels: the colour map's ends and beyond, 0 / 0 and x / 0 of depth / acc, a phasor on the negative real axis,
    a constant dd, a dd with a NaN, a range without width"""
    from gftorf_amd import present
    table = golden["magma_u8"]
    H, W, dr = 3, 5, 10.0
    znear, zfar = (np.float32(z) for z in zplanes_np(dr))
    inf = np.float32(np.inf)
    depth = np.full((1, H, W), 2.0, np.float32)
    acc = np.ones((1, H, W), np.float32)
    flat, aflat = depth.reshape(-1), acc.reshape(-1)
    flat[:8] = [zfar, znear, np.nextafter(zfar, inf), np.nextafter(znear, -inf), 0.0, 3.0, 2 * zfar, np.nextafter(znear, inf)]
    aflat[4:6] = 0.0
    phasor = np.array(make_view(H, W, 3, 1.0, 0.0, dr)["phasor"])
    phasor[0, 0, 0], phasor[1, 0, 0] = -1e-7, 0.0
    phasor[0, 0, 1], phasor[1, 0, 1] = 0.0, 0.5
    v = dict(phasor=phasor, depth=depth, acc=acc, dd=np.full((1, H, W), 1.5, np.float32), ranges=np.array([0, 0.5, 0.25, 0.25, 0, 0], np.float32),
             znear=znear, zfar=zfar, depth_range=np.float32(dr), phase_offset=np.float32(0.0), tof_multiplier=np.float32(1.0))
    want = view_np(v, table)
    # what the statements give there, spelled out
    dep, dn = want["depth"].reshape(-1, 4), want["depth_norm"].reshape(-1, 4)
    assert (dep[0] == table[0]).all() and (dep[1] == table[255]).all() and (dep[2] == table[0]).all() and (dep[3] == table[255]).all()
    assert (dep[6] == table[0]).all() and (dep[7] == table[255]).all() and not (dep[8] == table[255]).all()
    assert not dn[4].any() and (dn[5] == table[0]).all() and np.isnan(want["depth_norm_f"].reshape(-1)[4]) and want["depth_norm_f"].reshape(-1)[5] == inf
    assert abs(float(want["depth_tof_f"][0, 0]) - dr / 4) < 1e-5 and abs(float(want["depth_tof_f"][0, 1]) - dr / 8) < 1e-5      # phase pi, pi / 2
    assert not want["dd"].any()
    assert set(np.unique(want["imag"])) <= {0, 255} and not want["amp"][phasor[2] <= 0].any()
    got = present.view_images(**kwargs_on(gpu, v))
    check_images(got, want, v, golden["ref_err_depth_tof"], "special")
    nan_dd = np.array(make_view(H, W)["dd"])
    nan_dd[0, 1, 2] = np.nan
    for dd in (nan_dd, np.array([[[0.0, np.inf, 1.0]]], np.float32), np.array([[[-0.0, 0.0, 1.0, 0.5]]], np.float32)):
        w = view_np(dict(dd=dd), table)["dd"]
        assert w.any() == (not np.isnan(dd).any() and not np.isinf(dd).any())
        g = present.view_images(dd=torch.tensor(dd, device=gpu))
        assert set(g) == {"dd"} and np.array_equal(g["dd"].cpu().numpy(), w)


@pytest.mark.gpu
def test_planes_in_place_copies_and_absent_groups(gpu, golden, monkeypatch):
    """phasor[:3] of the 7-plane tensor is read where it lies; a transposed input is copied; every combination of groups the
    wrapper allows gives its keys, the bytes of the full call and a sheet of the size the layout query states"""
    from gftorf_amd import present
    H, W = 19, 27
    v = make_view(H, W)
    want = reference_np((H, W), v, golden["magma_u8"])
    kw = kwargs_on(gpu, v)
    real, seen = present._lib.load(), []

    class Spy:
        def __getattr__(self, name):
            def f(*args):
                seen.append((name, args))
                return getattr(real, name)(*args)
            return f
    monkeypatch.setattr(present._lib, "load", lambda: Spy())
    part = present.view_images(phasor=kw["phasor"][:3].requires_grad_(False), **{k: kw[k] for k in ("ranges", "zplanes", "depth_range", "phase_offset", "tof_multiplier")})
    args = [a for name, a in seen if name == "gft_present_view"]
    assert len(args) == 1 and args[0][1:3] == (H, W) and args[0][5] == kw["phasor"].data_ptr() and args[0][6:8] == (H * W, 3)
    v3 = dict(v, phasor=v["phasor"][:3])
    check_images(part, {k: want[k] for k in ("real", "imag", "amp", "depth_tof", "depth_tof_f")}, v3, golden["ref_err_depth_tof"], "phasor[:3]")
    no_quad = present.view_images(**dict(kw, quad=False))
    check_images(no_quad, {k: x for k, x in want.items() if k != "quad"}, v, golden["ref_err_depth_tof"], "quad=False")
    # a [H, W, C] tensor seen as [C, H, W], and a view with a row stride: both are copied
    seen.clear()
    odd = dict(kw, image=kw["image"].permute(1, 2, 0).contiguous().permute(2, 0, 1),
               depth=torch.cat([kw["depth"], kw["depth"]], dim=2)[:, :, :W])
    assert not odd["image"].is_contiguous() and not odd["depth"].is_contiguous()
    check_images(present.view_images(**odd), want, v, golden["ref_err_depth_tof"], "copied")
    a = [a for name, a in seen if name == "gft_present_view"][0]
    assert a[3] != odd["image"].data_ptr() and a[4] == H * W and a[8] != odd["depth"].data_ptr()
    monkeypatch.undo()
    scal = {k: kw[k] for k in ("ranges", "zplanes", "depth_range", "phase_offset", "tof_multiplier")}
    full = present.view_images(**kw)
    for mask in range(1, 32):
        names = [n for bit, n in enumerate(("image", "phasor", "depth", "acc", "dd")) if mask >> bit & 1]
        if "acc" in names and "depth" not in names:
            continue
        sub = {n: kw[n] for n in names}
        sub.update(scal if "phasor" in names else (dict(zplanes=kw["zplanes"]) if "depth" in names else {}))
        got = present.view_images(**sub)
        keys = ([("color",)] if "image" in names else []) + ([("real", "imag", "amp", "quad", "depth_tof", "depth_tof_f")] if "phasor" in names else []) + \
               ([("depth",)] if "depth" in names else []) + ([("depth_norm", "depth_norm_f")] if "acc" in names else []) + ([("dd",)] if "dd" in names else [])
        keys = [k for group in keys for k in group]
        assert set(got) == set(keys) and [k for k in IMAGES if k in got] == list(got), (names, sorted(got))
        for k in keys:
            assert torch.equal(got[k].view(torch.uint8), full[k].view(torch.uint8)), (names, k)
        groups = sum(bit for bit, n in ((1, "image"), (2, "phasor"), (4, "phasor"), (8, "depth"), (16, "acc"), (32, "dd")) if n in names)
        total, off = present.sheet_layout(H, W, groups)
        base = got[keys[0]].data_ptr()
        assert {k: t.data_ptr() - base for k, t in got.items()} == off


@pytest.mark.gpu
def test_scalars_by_value_and_from_the_device_give_the_same_bytes(gpu, golden):
    """ranges, depth_range and phase_offset from device tensors; a rewritten tensor is followed by the next call and by a
    replayed graph of view_images"""
    from gftorf_amd import present
    H, W = 19, 27
    v = make_view(H, W)
    kw = kwargs_on(gpu, v)
    by_value = present.view_images(**kw)
    rg = torch.tensor(v["ranges"], device=gpu)
    dr, off = torch.tensor([float(v["depth_range"])], device=gpu), torch.tensor(float(v["phase_offset"]), device=gpu)
    same = lambda a, b: set(a) == set(b) and all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)
    for over in (dict(ranges=rg, depth_range=dr, phase_offset=off), dict(ranges=rg), dict(depth_range=dr), dict(phase_offset=off)):
        assert same(present.view_images(**dict(kw, **over)), by_value), sorted(over)
    dev = dict(kw, ranges=rg, depth_range=dr, phase_offset=off)
    sheet = torch.zeros(present.sheet_layout(H, W, 63)[0], device=gpu, dtype=torch.uint8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        present.view_images(out=sheet, **dev)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = present.view_images(out=sheet, **dev)
    assert captured["color"].data_ptr() == sheet.data_ptr()
    # other ranges: real, imag and amp follow, in the next call and in the replayed graph
    new_rg = np.array([0.0, 0.3, 0.0, 1.1, 0.2, 0.5], np.float32)
    rg.copy_(torch.tensor(new_rg, device=gpu))
    moved_v = dict(v, ranges=new_rg)
    want = view_np(moved_v, golden["magma_u8"])
    assert not np.array_equal(want["real"], reference_np((H, W), v, golden["magma_u8"])["real"])
    check_images(present.view_images(**dev), want, moved_v, golden["ref_err_depth_tof"], "moved ranges")
    sheet.zero_()
    graph.replay()
    torch.cuda.synchronize()
    check_images(captured, want, moved_v, golden["ref_err_depth_tof"], "replayed ranges")
    # another offset and range: against the same numbers by value (the ToF depth's colours are the device's either way)
    off.fill_(0.25)
    dr.fill_(9.0)
    eager = present.view_images(**dev)
    assert same(eager, present.view_images(**dict(kw, ranges=[float(x) for x in new_rg], depth_range=9.0, phase_offset=0.25)))
    assert not torch.equal(eager["depth_tof_f"], by_value["depth_tof_f"]) and torch.equal(eager["depth"], by_value["depth"])
    graph.replay()
    torch.cuda.synchronize()
    assert same(captured, eager)


@pytest.mark.gpu
def test_phasor_ranges(gpu):
    """three views of different content (19 x 27: three workgroups) against np.min / np.max of the reference's stacked arrays; reset; a NaN stays"""
    from gftorf_amd import present
    rng = np.random.default_rng(5)
    gts = [(rng.uniform(-s, s, size=(c, H, W)) + b).astype(np.float32) for s, b, c, H, W in ((0.5, 0.0, 3, 19, 27), (1.5, 0.2, 7, 19, 27), (0.1, -0.05, 3, 19, 27))]
    ranges = present.PhasorRanges(device=gpu)
    assert np.array_equal(ranges.result(), np.array([np.inf, -np.inf] * 3, np.float32))
    seen = []
    for g in gts:
        ranges.add(torch.tensor(g, device=gpu))
        seen.append(g)
        want = ranges_np(seen)
        assert want[0] == 0 and want[2] == 0 and want[4] < 0
        assert np.array_equal(ranges.result(), want), (len(seen), ranges.result(), want)
    assert ranges.tensor.shape == (6,) and ranges.tensor.dtype == torch.float32 and ranges.tensor.device == gpu
    positive = np.abs(gts[0]) + np.float32(0.5)                 # no negative part: the blue channel is -0.0, the green 0
    ranges.reset()
    ranges.add(torch.tensor(positive, device=gpu))
    assert np.array_equal(ranges.result(), ranges_np([positive])) and ranges.result()[0] == 0 and ranges.result()[4] >= 0.5
    bad = gts[1].copy()
    bad[1, 3, 4] = np.nan
    ranges.add(torch.tensor(bad, device=gpu)[:3])
    ranges.add(torch.tensor(gts[2], device=gpu))
    got, want = ranges.result(), ranges_np([positive, bad, gts[2]])
    assert np.isnan(got[2:4]).all() and np.array_equal(got, want, equal_nan=True) and np.isfinite(got[[0, 1, 4, 5]]).all()
    ranges.reset()
    assert np.array_equal(ranges.result(), np.array([np.inf, -np.inf] * 3, np.float32))


@pytest.mark.gpu
def test_reproducible_and_without_host_sync(gpu):
    """two runs are bit-equal; view_images, PhasorRanges.add and ViewSheets.submit with every device-to-host synchronisation an
    error"""
    from gftorf_amd import present
    v = make_view(37, 53)
    kw = kwargs_on(gpu, v)
    a, b = present.view_images(**kw), present.view_images(**kw)
    assert all(torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) for k in a)
    ranges, sheets = present.PhasorRanges(device=gpu), present.ViewSheets(slots=2)
    on_device = dict(kw, ranges=ranges.tensor, depth_range=torch.tensor([7.5], device=gpu), phase_offset=torch.tensor(0.3, device=gpu))
    ranges.add(kw["phasor"])                      # warm-up: the library's first load and the pinned buffers are not the question
    sheets.submit("warm", **kw)
    list(sheets.ready(wait=True))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ranges.reset()
        ranges.add(kw["phasor"])
        ranges.add(kw["phasor"][:3])
        present.view_images(**kw)
        present.view_images(**on_device)
        sheets.submit(0, **kw)
        sheets.submit(1, **on_device)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert [tag for tag, _ in sheets.ready()] == [0, 1]
    assert np.array_equal(ranges.result(), ranges_np([v["phasor"]]))


@pytest.mark.gpu
def test_view_sheets(gpu, golden):
    """three views of two sizes through two slots: a third submit before any ready() raises; tags and contents come back in
    order and equal view_images"""
    from gftorf_amd import present
    views = [make_view(19, 27), make_view(37, 53), make_view(5, 7)]
    kws = [kwargs_on(gpu, v) for v in views]
    kws[2] = {k: kws[2][k] for k in ("depth", "acc", "zplanes")}
    direct = [{k: t.cpu().numpy() for k, t in present.view_images(**kw).items()} for kw in kws]
    sheets = present.ViewSheets(slots=2)
    assert list(sheets.ready()) == []
    sheets.submit("a", **kws[0])
    sheets.submit("b", **kws[1])
    with pytest.raises(RuntimeError, match="all 2 slots"):
        sheets.submit("c", **kws[2])
    torch.cuda.synchronize()
    out = []
    for tag, images in sheets.ready():
        out.append((tag, {k: a.copy() for k, a in images.items()}))
        if tag == "a":
            with pytest.raises(RuntimeError, match="all 2 slots"):          # a's arrays are still the caller's, b is in flight
                sheets.submit("c", **kws[2])
        elif tag == "b":
            sheets.submit("c", **kws[2])                                    # the loop moved past a: its slot is free
    out += [(tag, {k: a.copy() for k, a in images.items()}) for tag, images in sheets.ready(wait=True)]
    assert [tag for tag, _ in out] == ["a", "b", "c"]
    for (tag, images), want in zip(out, direct):
        assert list(images) == list(want), tag
        for k in want:
            assert images[k].dtype == want[k].dtype and images[k].shape == want[k].shape
            assert np.array_equal(images[k].view(np.uint8), want[k].view(np.uint8)), (tag, k)
    assert list(sheets.ready(wait=True)) == []


@pytest.mark.gpu
def test_composed_with_the_rasterizer(gpu, golden):
    """one small scene rendered by the rasterizer; its outputs go into view_images where they lie.  The frame's phasor is what
    the rasterizer gives: depth_tof is compared at the pixels `conditioned` accepts, which must be at least 99 % of the frame
    (all of them when the whole frame is accepted); everything else at every pixel"""
    import helpers as Hh
    from gftorf_amd import present
    # chosen with the CPU oracle: a thin slab of depth, 4 of the 1961 pixels are not conditioned (19 may be)
    scene = Hh.small_scene(P=1500, W=53, H=37, seed=9, z_lo=2.0, z_hi=2.6)
    _, _, t = Hh.run_gpu(scene, gpu, backward=False)
    o = {k: t["outs"][k].detach() for k in ("color", "phasor", "depth", "acc", "depth_distortion")}
    H, W = 37, 53
    assert tuple(o["phasor"].shape)[1:] == (H, W) and tuple(o["color"].shape) == (3, H, W) and tuple(o["depth_distortion"].shape) == (1, H, W)
    dr, off = scene["depth_range"], scene["phase_offset"]
    ranges = present.PhasorRanges(device=gpu)
    ranges.add(o["phasor"])
    zp = present.zplanes(dr)
    got = present.view_images(image=o["color"], phasor=o["phasor"], depth=o["depth"], acc=o["acc"], dd=o["depth_distortion"],
                              ranges=ranges.tensor, zplanes=zp, depth_range=dr, phase_offset=off, tof_multiplier=2.0)
    v = dict(image=o["color"].cpu().numpy(), phasor=o["phasor"].cpu().numpy(), depth=o["depth"].cpu().numpy(), acc=o["acc"].cpu().numpy(),
             dd=o["depth_distortion"].cpu().numpy(), ranges=ranges.result(), znear=np.float32(zp[0]), zfar=np.float32(zp[1]),
             depth_range=np.float32(dr), phase_offset=np.float32(off), tof_multiplier=np.float32(2.0))
    assert np.array_equal(v["ranges"], ranges_np([v["phasor"]]))
    want = view_np(v, golden["magma_u8"])
    ok = conditioned(v["phasor"], dr, off, zp[0], zp[1])
    print("composed: %d of %d pixels conditioned, planes %d" % (int(ok.sum()), ok.size, v["phasor"].shape[0]))
    assert ok.mean() >= 0.99
    got = {k: x.cpu().numpy() for k, x in got.items()}
    d64 = depth_from_tof_np(v["phasor"], f32(dr), f32(off), np.float64)
    err = np.abs(got["depth_tof_f"] - d64)[ok].max()
    assert err <= 3 * golden["ref_err_depth_tof"] * f32(dr), err
    assert np.array_equal(got["depth_tof"][ok], want["depth_tof"][ok])
    for k in want:
        if k not in ("depth_tof", "depth_tof_f"):
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    assert len(np.unique(got["color"])) > 20 and len(np.unique(got["depth"].reshape(-1, 4), axis=0)) > 5
