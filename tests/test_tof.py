"""gftorf_amd.tof: the ToF depth of scene/torf_utils.py:59-64 and the scalars of the training log (train.py:188-200, 402-433).
The yardsticks are the reference's own float32 results (tests/golden/tof.npz, written by tests/golden/make_golden_tof.py) and
`depth64` / `log64` below -- depth_from_tof_torch and the log's statements restated, to be read against those lines -- run in
float64 on the CPU over the float32 inputs.

Inputs are drawn so that the reference alone is well-conditioned: the wrapped phase after the offset lies in
[0.05, 2 pi - 0.05] (no pixel changes its `+ 2 pi` branch between float32 and float64: `draw_phasor` asserts it), amplitudes
in [0.02, 1].

Tolerances:
  depth_from_tof    max |device - f64| <= 4e-7 * depth_range / 2.  The reference's own float32 result is within 1.1e-7 to
                    1.3e-7 of the largest value depth_range / 2; the margin of about three is for the device's atan2f.
  a mean of the log 1e-6 * (the sum of the means of the magnitudes of the slot's two operands), for a plain mean 1e-6 * the
                    mean's magnitude: the per-element fp32 error of amp * d^2 is at most about 4e-7 relative, and the sums
                    finish in double.
  visible count     exact
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_tof.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tof.npz")
CASES = ("plain", "ragged", "full")
SH_C0 = 0.28209479177387814
# pixels = 1, 63, 64, 65, 257, 37 x 53, and 513 x 512 > 256 threads x the cap of 1024 workgroups: the stride loop runs twice
SHAPES = [(1, 1), (7, 9), (8, 8), (5, 13), (1, 257), (37, 53), (513, 512)]
ROWS = [0, 1, 65, 70_001]
SLOTS = ("sp", "sp_tof", "gsp", "sp_err", "sp_tof_err", "depth_err", "tof_depth_err", "amp_err", "dd", "gs_sp", "gs_sp_visible")


def f32(x):
    """the float32 the device is handed for a Python number, as a float"""
    return float(np.float32(x))


# ---- the restatement ---------------------------------------------------------------------------------------------------

def depth64(tof, depth_range, phase_offset):
    """torf_utils.py:60-64 in float64 over float32 planes; the threshold is compared in float32, as torch compares a
    Python scalar against a float32 tensor"""
    tiny = np.float32(1e-6)
    real = np.where(np.abs(tof[0]) < tiny, np.float64(tiny), tof[0].astype(np.float64))
    tof_phase = np.arctan2(tof[1].astype(np.float64), real)
    tof_phase = tof_phase - phase_offset
    tof_phase = np.where(tof_phase < 0, tof_phase + 2 * np.pi, tof_phase)
    return tof_phase * depth_range / (4 * np.pi)


def log64(inp):
    """(means, tolerances, visible count) of train.py:188-200, 420-433 in float64, for the inputs present in `inp`; an
    absent input and an empty selection give 0"""
    d = lambda k: inp[k].astype(np.float64)
    dr, off = f32(inp["depth_range"]), f32(inp["phase_offset"])
    pd, gpd = depth64(inp["phasor"], dr, off), depth64(inp["gt_phasor"], dr, off)
    amp, gt_amp, depth = d("phasor")[2] * f32(inp["tof_multiplier"]), d("gt_phasor")[2], d("depth")[0]
    sp, sp_tof, gsp = amp * depth ** 2, amp * pd ** 2, gt_amp * gpd ** 2
    m = lambda a: float(np.abs(a).mean())
    means = dict(sp=sp.mean(), sp_tof=sp_tof.mean(), gsp=gsp.mean(), sp_err=np.abs(gsp - sp).mean(),
                 sp_tof_err=np.abs(gsp - sp_tof).mean(), tof_depth_err=np.abs(pd - gpd).mean(), amp_err=np.abs(amp - gt_amp).mean())
    tol = dict(sp=m(sp), sp_tof=m(sp_tof), gsp=m(gsp), sp_err=m(gsp) + m(sp), sp_tof_err=m(gsp) + m(sp_tof),
               tof_depth_err=m(pd) + m(gpd), amp_err=m(amp) + m(gt_amp))
    if "gt_depth" in inp:
        means["depth_err"], tol["depth_err"] = np.abs(depth - d("gt_depth")[0]).mean(), m(depth) + m(d("gt_depth"))
    if "dd" in inp:
        means["dd"], tol["dd"] = d("dd").mean(), abs(d("dd").mean())
    n_vis = 0
    coeff = inp.get("features_phasor", inp.get("amp_f_dc"))
    if coeff is not None and coeff.shape[0] > 0:
        a = coeff.astype(np.float64)[:, 0, -1]                   # [:, 0, 1] of features_phasor, [:, 0, 0] of amp_f_dc
        sh2pa = a * SH_C0 + 0.5
        means["gs_sp"], tol["gs_sp"] = sh2pa.mean(), abs(sh2pa.mean())
        if "visible" in inp:
            vis = inp["visible"] > 0
            n_vis = int(vis.sum())
            if n_vis:
                means["gs_sp_visible"], tol["gs_sp_visible"] = sh2pa[vis].mean(), abs(sh2pa[vis].mean())
    return ({k: float(means.get(k, 0.0)) for k in SLOTS}, {k: 1e-6 * float(tol.get(k, 0.0)) for k in SLOTS}, n_vis)


# ---- inputs -------------------------------------------------------------------------------------------------------------

def draw_phasor(rng, planes, H, W, phase_offset):
    """as tests/golden/make_golden_tof.py: the wrapped phase in [0.05, 2 pi - 0.05], plane 2 in [0.02, 1]; a real part
    below 1e-4 is pushed out to 1e-4 (the vector is at least 0.05 long, so the phase moves by 2e-3 at the most: the clamp of
    the real part has its own test)"""
    off = f32(phase_offset)
    theta = rng.uniform(0.05, 2 * np.pi - 0.05, size=(H, W)) + off
    length = rng.uniform(0.05, 1.0, size=(H, W))
    out = rng.uniform(-1.0, 1.0, size=(planes, H, W))
    out[0], out[1], out[2] = length * np.cos(theta), length * np.sin(theta), rng.uniform(0.02, 1.0, size=(H, W))
    out[0] = np.where(np.abs(out[0]) < 1e-4, np.copysign(1e-4, out[0]), out[0])
    out = out.astype(np.float32)
    p64 = np.arctan2(out[1].astype(np.float64), out[0].astype(np.float64)) - off
    p32 = np.arctan2(out[1], out[0]) - np.float32(off)
    assert np.array_equal(p64 < 0, p32 < 0), "a pixel changes its +2 pi branch between float32 and float64"
    return out


@functools.lru_cache(maxsize=None)
def make_pixels(H, W):
    """the images of one size: a 7-plane phasor, gt_phasor, depth, gt_depth, dd; depth_range 7.5, offset -0.2 or 0.3"""
    rng = np.random.default_rng(100 * H + W)
    off = -0.2 if (H * W) % 2 else 0.3
    out = dict(phasor=draw_phasor(rng, 7, H, W, off), gt_phasor=draw_phasor(rng, 3, H, W, off), depth_range=7.5, phase_offset=off,
               tof_multiplier=2.0 if H == 37 else 1.0, depth=rng.uniform(0.3, 3.7, size=(1, H, W)).astype(np.float32))
    out["gt_depth"] = (out["depth"] + rng.normal(0.0, 0.2, size=(1, H, W))).astype(np.float32)
    out["dd"] = rng.uniform(0.0, 0.4, size=(1, H, W)).astype(np.float32)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def make_rows(P):
    """features_phasor [P, 4, 2] with SH2PA of the amplitude coefficient in 0.2-0.9, the same coefficients as amp_f_dc
    [P, 1, 1], a bool visibility of ~60 % and radii (0 and negative values are invisible)"""
    rng = np.random.default_rng(7 + P)
    feats = rng.normal(0.0, 1.0, size=(P, 4, 2)).astype(np.float32)
    feats[:, 0, 1] = rng.uniform(-1.0, 1.4, size=P)
    visible = rng.random(P) < 0.6
    radii = rng.integers(-3, 40, P).astype(np.int32)
    radii[rng.random(P) < 0.4] = 0
    if P:
        visible[0], radii[0] = True, 5
    out = dict(features_phasor=feats, amp_f_dc=np.ascontiguousarray(feats[:, :1, 1:]), visible=visible, radii=radii)
    for a in out.values():
        a.setflags(write=False)
    return out


_F64 = {}


def reference64(key, inp):
    """float64 on the CPU, computed once per input set and shared"""
    if key not in _F64:
        _F64[key] = log64(inp)
    return _F64[key]


def on(dev, inp):
    return {k: torch.tensor(v, device=dev) if isinstance(v, np.ndarray) else v for k, v in inp.items()}


def call_row(t, f=None, **over):
    """tof.train_log_row (or `f`, a TrainLog's record) on the dict's entries"""
    from gftorf_amd import tof
    kw = dict(depth_range=t["depth_range"], phase_offset=t["phase_offset"], tof_multiplier=t["tof_multiplier"],
              gt_depth=t.get("gt_depth"), depth_distortion=t.get("dd"), features_phasor=t.get("features_phasor"),
              amp_f_dc=t.get("amp_f_dc"), visible=t.get("visible"), extras=t.get("extras", ()))
    kw.update(over)
    return (f or tof.train_log_row)(t["phasor"][:3], t["depth"], t["gt_phasor"], **kw)


def host(row):
    from gftorf_amd import tof
    return {k: v[0] for k, v in tof.unpack(row.cpu().numpy()).items()}


MEASURED = {}          # largest error per check relative to its bound (pytest -s)


def _note(key, err):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(err))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\ntof errors measured, relative to their bounds:", {k: "%.3g" % v for k, v in sorted(MEASURED.items())})


def check_row(key, inp, got, what):
    """every mean of a row against the float64 statements; the presence word, the count"""
    from gftorf_amd import _lib
    means, tols, n_vis = reference64(key, inp)
    for k in SLOTS:
        err = abs(float(got[k]) - means[k])
        print("%s %s: %.9g ref %.9g err %.3g bound %.3g" % (key, k, got[k], means[k], err, tols[k]))
        if tols[k] > 0:
            _note("%s %s" % (what, k), err / tols[k])
        assert err <= tols[k], (key, k, float(got[k]), means[k], err, tols[k])
    assert int(got["visible"]) == n_vis, key
    has_amp = any(k in inp and inp[k].shape[0] > 0 for k in ("features_phasor", "amp_f_dc"))
    present = ((_lib.TOF_HAS_GT_DEPTH if "gt_depth" in inp else 0) | (_lib.TOF_HAS_DD if "dd" in inp else 0) |
               (_lib.TOF_HAS_AMP if has_amp else 0) | (_lib.TOF_HAS_VISIBLE if has_amp and "visible" in inp else 0))
    assert int(got["present"]) == present, (key, int(got["present"]), present)


# ---- CPU-runnable checks: header, exports, argument errors, the wrapper's checks ------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c_and_every_symbol_is_exported(tmp_path, lib):
    from gftorf_amd import _lib, tof
    names = declared_functions()
    assert set(names) == set(_lib.TOF_EXPORTS), names
    assert not set(names) & (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.FEATURE_EXPORTS) | set(_lib.REG_EXPORTS))
    for n in names:
        assert hasattr(lib, n), n
    prog = tmp_path / "tof_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_tof.h"', '#include "gftorf_reg.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "tof_abi.o")])
    # the header's constants are the Python side's
    words = ["GFT_TOF_LOG_" + k.upper() for k in SLOTS] + ["GFT_TOF_LOG_VISIBLE", "GFT_TOF_LOG_PRESENT", "GFT_TOF_LOG_NUM_EXTRAS",
                                                           "GFT_TOF_LOG_SEQ", "GFT_TOF_LOG_EXTRAS", "GFT_TOF_LOG_MAX_EXTRAS",
                                                           "GFT_TOF_LOG_WORDS", "GFT_TOF_PARTIAL_WORDS", "GFT_TOF_HAS_GT_DEPTH",
                                                           "GFT_TOF_HAS_DD", "GFT_TOF_HAS_AMP", "GFT_TOF_HAS_VISIBLE"]
    out = subprocess.check_output(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-include", "gftorf_tof.h",
                                   "-x", "c", "-"], input="TOF_WORDS_ARE " + " ".join(words) + "\n", text=True)
    consts = [int(v) for v in out.split("TOF_WORDS_ARE", 1)[1].split()]
    assert tuple(tof.FLOATS) == SLOTS == _lib.TOF_LOG_FLOATS
    assert consts == list(range(len(SLOTS))) + [_lib.TOF_LOG_VISIBLE, _lib.TOF_LOG_PRESENT, _lib.TOF_LOG_NUM_EXTRAS, _lib.TOF_LOG_SEQ,
                                                _lib.TOF_LOG_EXTRAS, _lib.TOF_LOG_MAX_EXTRAS, _lib.TOF_LOG_WORDS, _lib.TOF_PARTIAL_WORDS,
                                                _lib.TOF_HAS_GT_DEPTH, _lib.TOF_HAS_DD, _lib.TOF_HAS_AMP, _lib.TOF_HAS_VISIBLE]
    assert _lib.TOF_LOG_EXTRAS + _lib.TOF_LOG_MAX_EXTRAS == _lib.TOF_LOG_WORDS and tof.MAX_EXTRAS == 8
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16


def test_size_query_and_argument_errors(lib):
    from gftorf_amd import _lib
    assert lib.gft_tof_log_blocks(0, 5) == 0 and lib.gft_tof_log_blocks(-1, 5) == 0 and lib.gft_tof_log_blocks(5, -1) == 0
    assert lib.gft_tof_log_blocks(1, 0) == 1 and lib.gft_tof_log_blocks(256, 0) == 1 and lib.gft_tof_log_blocks(256, 1) == 2
    assert lib.gft_tof_log_blocks(320 * 240, 100_000) == 691
    assert lib.gft_tof_log_blocks(256 * 1024, 0) == 1024 and lib.gft_tof_log_blocks(513 * 512, 0) == 1024      # then grid-stride
    assert lib.gft_tof_log_blocks(640 * 480, 1_000_000) == 1024
    x = C.c_void_p(16)                                         # never dereferenced: the calls fail before any launch
    depth = lambda n, tof=x, stride=4, out=x: lib.gft_tof_depth(None, n, tof, stride, None, 10.0, None, 0.0, out)
    assert depth(-1) != 0 and "bad sizes" in _lib.last_error()
    assert depth(4, tof=None) != 0 and "NULL" in _lib.last_error()
    assert depth(4, out=None) != 0 and "NULL" in _lib.last_error()
    assert depth(4, stride=-4) != 0 and "plane_stride" in _lib.last_error()
    assert depth(0, tof=None, out=None) == 0                  # nothing to do
    two = (C.c_void_p * 2)(16, 16)
    hole = (C.c_void_p * 2)(16, None)

    def row(pixels=4, P=4, ph=x, d=x, gt=x, ph_stride=4, gt_stride=4, amp=x, amp_stride=1, vis=x, extras=two, n=2, part=x, rows=x,
            slots=1, cursor=None):
        return lib.gft_tof_log_row(None, pixels, P, ph, ph_stride, d, gt, gt_stride, None, 10.0, None, 0.0, 1.0, None, None, amp,
                                   amp_stride, vis, 1, extras, n, part, rows, slots, cursor)
    for bad, msg in ((dict(pixels=0), "bad sizes"), (dict(pixels=-4), "bad sizes"), (dict(P=-1), "bad sizes"), (dict(P=1 << 31), "bad sizes"),
                     (dict(ph=None), "is NULL"), (dict(d=None), "is NULL"), (dict(gt=None), "is NULL"),
                     (dict(ph_stride=-1), "bad plane stride"), (dict(gt_stride=-1), "bad plane stride"),
                     (dict(amp=None), "visible without the amplitude coefficients"), (dict(amp_stride=0), "bad amp_stride"),
                     (dict(n=9), "num_extras=9 is not in 0..8"), (dict(n=-1), "num_extras=-1"), (dict(extras=None), "extras is NULL"),
                     (dict(extras=hole), "extras[1] is NULL"), (dict(part=None), "partials or rows is NULL"),
                     (dict(rows=None), "partials or rows is NULL"), (dict(slots=0), "bad slots"), (dict(slots=-3), "bad slots")):
        assert row(**bad) != 0, bad
        assert msg in _lib.last_error(), (bad, _lib.last_error())


def test_wrapper_rejects_cpu_tensors_shapes_and_too_many_extras():
    from gftorf_amd import tof
    H, W, P = 4, 6, 5
    ph, gt, d = torch.rand(7, H, W), torch.rand(3, H, W), torch.rand(1, H, W)
    feats, dc = torch.rand(P, 4, 2), torch.rand(P, 1, 1)
    vis, radii, one = torch.ones(P, dtype=torch.bool), torch.ones(P, dtype=torch.int32), torch.tensor(0.5)
    calls = [lambda: tof.depth_from_tof(ph[:3], 10.0), lambda: tof.depth_from_tof(gt, 10.0, phase_offset=0.1),
             lambda: tof.train_log_row(ph[:3], d, gt, 10.0), lambda: tof.train_log_row(ph, d, gt, 10.0, 0.1, 2.0, gt_depth=d, depth_distortion=d,
                                                                                      features_phasor=feats, visible=radii, extras=(one,)),
             lambda: tof.train_log_row(ph, d, gt, 10.0, amp_f_dc=dc, visible=vis), lambda: tof.TrainLog(slots=4, device="cpu")]
    for c in calls:
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            c()
    # shapes, dtypes and counts are checked before any device
    one8 = [one] * 9
    shapes = [(lambda: tof.depth_from_tof(ph[:1], 10.0), r"tof must be \[>=2, H, W\]"),
              (lambda: tof.depth_from_tof(ph[0], 10.0), r"tof must be \[>=2, H, W\]"),
              (lambda: tof.depth_from_tof(ph, torch.ones(2)), "depth_range must be a number or a one-element tensor"),
              (lambda: tof.train_log_row(ph[:2], d, gt, 10.0), r"phasor must be \[>=3, H, W\]"),
              (lambda: tof.train_log_row(ph, d, gt[:, :-1], 10.0), r"gt_phasor must be \[>=3, 4, 6\]"),
              (lambda: tof.train_log_row(ph, d[0], gt, 10.0), r"depth must be \[1, 4, 6\]"),
              (lambda: tof.train_log_row(ph, d, gt, 10.0, gt_depth=d[:, :, :-1]), r"gt_depth must be \[1, 4, 6\]"),
              (lambda: tof.train_log_row(ph, d, gt, 10.0, depth_distortion=gt), r"depth_distortion must be \[1, 4, 6\]"),
              (lambda: tof.train_log_row(ph, d, gt, 10.0, features_phasor=feats[:, :, :1]), r"features_phasor must be \[P, M, 2\]"),
              (lambda: tof.train_log_row(ph, d, gt, 10.0, amp_f_dc=feats), r"amp_f_dc must be \[P, 1, 1\]"),
              (lambda: tof.train_log_row(ph, d, gt, 10.0, amp_f_dc=dc, visible=vis[:-1]), r"visible must be \[5\]"),
              (lambda: tof.train_log_row(ph, d, gt, 10.0, extras=[torch.zeros(2)]), r"extras\[0\] must be 0-dim or one-element"),
              (lambda: tof.train_log_row(ph, d, gt, 10.0, phase_offset=torch.zeros(3)), "phase_offset must be a number or a one-element")]
    for c, msg in shapes:
        with pytest.raises(RuntimeError, match=msg):
            c()
    with pytest.raises(ValueError, match="at most 8 extras fit a row, got 9"):
        tof.train_log_row(ph, d, gt, 10.0, extras=one8)
    with pytest.raises(ValueError, match="visible selects among the amplitude coefficients"):
        tof.train_log_row(ph, d, gt, 10.0, visible=vis)
    with pytest.raises(ValueError, match="two forms of the same coefficients"):
        tof.train_log_row(ph, d, gt, 10.0, features_phasor=feats, amp_f_dc=dc)
    with pytest.raises(TypeError, match="visible must be torch.bool or torch.int32"):
        tof.train_log_row(ph, d, gt, 10.0, amp_f_dc=dc, visible=vis.long())
    with pytest.raises(TypeError, match="tof must be a tensor"):
        tof.depth_from_tof(ph.numpy(), 10.0)
    with pytest.raises(TypeError, match="tof must be torch.float32"):
        tof.depth_from_tof(ph.double(), 10.0)
    with pytest.raises(TypeError, match="phasor must be torch.float32"):
        tof.train_log_row(ph.half(), d, gt, 10.0)
    with pytest.raises(ValueError, match="slots must be in"):
        tof.TrainLog(slots=0)


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {c: {k[len(c) + 1:]: z[k] for k in z.files if k.startswith(c + "_")} for c in CASES}


def depth_bound(depth_range):
    return 4e-7 * f32(depth_range) / 2


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_depth_from_tof_matches_the_float64_statements(shape, gpu):
    from gftorf_amd import tof
    inp = make_pixels(*shape)
    for name in ("phasor", "gt_phasor"):
        got = tof.depth_from_tof(torch.tensor(inp[name], device=gpu), inp["depth_range"], inp["phase_offset"])
        ref = depth64(inp[name], f32(inp["depth_range"]), f32(inp["phase_offset"]))
        assert tuple(got.shape) == shape and got.dtype == torch.float32 and not got.requires_grad
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
        print("%s %s: max |device - f64| %.3g bound %.3g" % (shape, name, err, depth_bound(inp["depth_range"])))
        _note("depth_from_tof f64", err / depth_bound(inp["depth_range"]))
        assert err <= depth_bound(inp["depth_range"]), (shape, name, err)


@pytest.mark.gpu
def test_depth_from_tof_matches_the_reference_fixture(gpu, golden):
    """the reference's own float32 results; two float32 routes, each within its distance of float64: the reference's
    1.3e-7 of the largest value and the device's 4e-7"""
    from gftorf_amd import tof
    for c in CASES:
        g = golden[c]
        for src, res in (("phasor", "phase_depth"), ("gt_phasor", "gt_phase_depth")):
            t = torch.tensor(g[src], device=gpu).requires_grad_()
            got = tof.depth_from_tof(t[:3], float(g["depth_range"]), phase_offset=float(g["phase_offset"]))
            assert not got.requires_grad and got.grad_fn is None          # detached: the documented difference
            ref64 = depth64(g[src], float(g["depth_range"]), float(g["phase_offset"]))
            half = float(g["depth_range"]) / 2
            assert float(np.abs(g[res].astype(np.float64) - ref64).max()) <= 1.3e-7 * half, (c, src)
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref64).max())
            _note("depth_from_tof f64", err / depth_bound(g["depth_range"]))
            assert err <= depth_bound(g["depth_range"]), (c, src, err)
            e32 = float(np.abs(got.cpu().numpy().astype(np.float64) - g[res]).max())
            _note("depth_from_tof fixture", e32 / ((4e-7 + 1.3e-7) * half))
            assert e32 <= (4e-7 + 1.3e-7) * half, (c, src, e32)


@pytest.mark.gpu
def test_depth_from_tof_clamp_branch(gpu):
    """hand-placed pixels around the clamp of the real part: |re| < 1e-6 (compared in float32) becomes +1e-6"""
    from gftorf_amd import tof
    res = [0.0, -0.0, 5e-7, -5e-7, 1e-6, -1e-6, 2e-6, -2e-6]
    planes = np.array([[r for r in res for _ in (0, 1)], [s * 0.3 for _ in res for s in (1, -1)]], np.float32).reshape(2, 2, 8)
    for off in (0.0, 0.3, -0.2):
        got = tof.depth_from_tof(torch.tensor(planes, device=gpu), 7.5, off).cpu().numpy().astype(np.float64)
        ref = depth64(planes, 7.5, f32(off))
        err = float(np.abs(got - ref).max())
        _note("depth_from_tof clamp", err / depth_bound(7.5))
        assert err <= depth_bound(7.5), (off, err, got, ref)
    # the branch itself: -5e-7 is clamped to +1e-6 (the phase of +0.3 i stays below pi / 2), -2e-6 is not
    flat = tof.depth_from_tof(torch.tensor(planes, device=gpu), 7.5, 0.0).cpu().numpy().reshape(-1)
    quarter = 7.5 / 8          # phase pi / 2
    assert flat[6] < quarter and flat[10] > quarter > flat[8] and flat[14] > quarter


@pytest.mark.gpu
def test_depth_from_tof_reads_its_scalars_when_it_runs(gpu, monkeypatch):
    from gftorf_amd import tof
    inp = make_pixels(37, 53)
    wide = torch.tensor(inp["phasor"], device=gpu)
    assert wide.shape[0] == 7
    by_value = tof.depth_from_tof(wide[:3], 7.5, -0.2)
    dr, off = torch.tensor([7.5], device=gpu), torch.tensor(-0.2, device=gpu)
    assert torch.equal(tof.depth_from_tof(wide[:3], dr, off), by_value)
    assert torch.equal(tof.depth_from_tof(wide[:3], dr, -0.2), by_value) and torch.equal(tof.depth_from_tof(wide[:3], 7.5, off), by_value)
    dr.fill_(9.0)
    off.fill_(0.25)
    assert torch.equal(tof.depth_from_tof(wide[:3], dr, off), tof.depth_from_tof(wide[:3], 9.0, 0.25))
    assert not torch.equal(tof.depth_from_tof(wide[:3], dr, off), by_value)
    # the view is read in place: the pointer handed to the C call is the wide tensor's, the plane stride its own
    real, seen = tof._lib.load(), []

    class Spy:
        def __getattr__(self, name):
            def f(*args):
                seen.append((name, args))
                return getattr(real, name)(*args)
            return f
    monkeypatch.setattr(tof._lib, "load", lambda: Spy())
    tof.depth_from_tof(wide[:3], 7.5, -0.2)
    tof.depth_from_tof(wide[1:4], 7.5, -0.2)
    rows = tof.depth_from_tof(wide[:, 1:, :][:3], 7.5, -0.2)             # whole rows of every plane: still in place
    cols = tof.depth_from_tof(wide[:, :, 1:][:3], 7.5, -0.2)             # planes no longer contiguous: copied
    assert [name for name, _ in seen] == ["gft_tof_depth"] * 4
    assert seen[0][1][2] == wide.data_ptr() and seen[0][1][3] == 37 * 53
    assert seen[1][1][2] == wide[1].data_ptr() and seen[1][1][3] == 37 * 53
    assert seen[2][1][2] == wide[:, 1:, :].data_ptr() and seen[2][1][3] == 37 * 53 and seen[2][1][1] == 36 * 53
    assert seen[3][1][2] not in (wide.data_ptr(), wide[:, :, 1:].data_ptr()) and seen[3][1][3] == 37 * 52
    assert torch.equal(rows, by_value[1:]) and torch.equal(cols, by_value[:, 1:])


@pytest.mark.gpu
@pytest.mark.parametrize("P", ROWS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_train_log_row_matches_the_float64_statements(shape, P, gpu):
    """every mean; both layouts of the amplitude coefficients; bool and radii visibility"""
    pix, rows = make_pixels(*shape), make_rows(P)
    for layout, vis in (("features_phasor", "visible"), ("amp_f_dc", "radii")):
        inp = dict(pix, **{layout: rows[layout], "visible": rows[vis]})
        t = on(gpu, inp)
        if layout == "features_phasor":
            assert not t[layout][:, 0, 1].is_contiguous() or P <= 1
        got = host(call_row(t))
        check_row((shape, P, layout), inp, got, "row f64")
        assert int(got["seq"]) == 0 and int(got["num_extras"]) == 0 and not got["extras"].any()


@pytest.mark.gpu
def test_train_log_row_reads_planes_by_their_stride(gpu):
    """whole rows cut from every plane: the planes stay contiguous, but lie further apart than they are long, so the row
    must equal, bit for bit, that of contiguous copies of the same planes"""
    from gftorf_amd import tof
    pix, rows = make_pixels(37, 53), make_rows(65)
    t = on(gpu, dict(pix, features_phasor=rows["features_phasor"], visible=rows["radii"]))
    cut = lambda a: a[:, 1:, :]
    ph, gt = cut(t["phasor"]), cut(t["gt_phasor"])
    taken = tof._planes(ph, "phasor", 3)
    assert ph.stride(0) == 37 * 53 != 36 * 53 and taken[0].data_ptr() == ph.data_ptr() and taken[1:] == (37 * 53, 36, 53)
    assert tof._planes(gt, "gt_phasor", 3)[0].data_ptr() == gt.data_ptr()          # taken in place
    kw = dict(depth_range=7.5, phase_offset=-0.2, tof_multiplier=2.0, gt_depth=cut(t["gt_depth"]), depth_distortion=cut(t["dd"]),
              features_phasor=t["features_phasor"], visible=t["visible"])
    strided = tof.train_log_row(ph, cut(t["depth"]), gt, **kw)
    packed = tof.train_log_row(ph[:3].contiguous(), cut(t["depth"]), gt.contiguous(), **kw)
    assert torch.equal(strided.view(torch.int32), packed.view(torch.int32))
    whole = call_row(t)
    assert not torch.equal(strided[:9], whole[:9])          # other pixels: the cut is not a no-op
    inp = {k: (v[:, 1:, :] if isinstance(v, np.ndarray) and v.ndim == 3 and v.shape[1:] == (37, 53) else v) for k, v in pix.items()}
    check_row((36, 53, 65, "strided"), dict(inp, features_phasor=rows["features_phasor"], visible=rows["radii"]), host(strided), "row f64")
    log = tof.TrainLog(slots=2, device="cuda")          # a device without an index is the current one
    log.record(ph, cut(t["depth"]), gt, **kw)
    got, lost = log.drain(wait=True)
    assert lost == 0 and all(got[k][0].tobytes() == host(strided)[k].tobytes() for k in SLOTS)


@pytest.mark.gpu
def test_every_optional_input_absent_in_turn_and_extras(gpu):
    pix, rows = make_pixels(37, 53), make_rows(65)
    full = dict(pix, features_phasor=rows["features_phasor"], visible=rows["radii"])
    extras = [torch.tensor(0.25 * (k + 1), device=gpu).reshape(() if k % 2 else (1,)) for k in range(8)]
    for drop in ((), ("gt_depth",), ("dd",), ("visible",), ("features_phasor", "visible"), ("gt_depth", "dd", "features_phasor", "visible")):
        inp = {k: v for k, v in full.items() if k not in drop}
        got = host(call_row(dict(on(gpu, inp), extras=extras[:8 - len(drop)])))
        check_row((37, 53, 65, drop), inp, got, "row f64")
        for k, slots in (("gt_depth", ("depth_err",)), ("dd", ("dd",)), ("visible", ("gs_sp_visible",)), ("features_phasor", ("gs_sp", "gs_sp_visible"))):
            if k in drop:
                assert all(float(got[s]) == 0.0 for s in slots), (drop, k)
        assert int(got["num_extras"]) == 8 - len(drop)
        assert got["extras"].tolist() == [0.25 * (k + 1) if k < 8 - len(drop) else 0.0 for k in range(8)]
    from gftorf_amd import tof
    t = on(gpu, full)
    with pytest.raises(ValueError, match="at most 8 extras"):
        call_row(dict(t, extras=extras + [extras[0]]))
    with pytest.raises(ValueError, match="visible selects among the amplitude coefficients"):
        call_row(dict(t, features_phasor=None))
    with pytest.raises(ValueError, match="two forms of the same coefficients"):
        call_row(dict(t, amp_f_dc=torch.tensor(rows["amp_f_dc"], device=gpu)))
    with pytest.raises(RuntimeError, match=r"extras\[0\] must be 0-dim or one-element"):
        call_row(dict(t, extras=[torch.zeros(2, device=gpu)]))
    with pytest.raises(RuntimeError, match=r"depth must be \[1, 37, 53\]"):
        call_row(dict(t, depth=t["depth"][:, :-1]))
    with pytest.raises(RuntimeError, match=r"gt_phasor must be \[>=3, 37, 53\]"):
        call_row(dict(t, gt_phasor=t["gt_phasor"][:, :-1]))
    with pytest.raises(RuntimeError, match=r"phasor must be \[>=3, H, W\]"):
        tof.train_log_row(t["phasor"][:2], t["depth"], t["gt_phasor"], 7.5)
    with pytest.raises(RuntimeError, match=r"visible must be \[65\]"):
        call_row(dict(t, visible=t["visible"][:-1]))
    with pytest.raises(RuntimeError, match="extras\\[0\\] is on cpu"):
        call_row(dict(t, extras=[torch.tensor(1.0)]))


@pytest.mark.gpu
def test_all_invisible_gives_zero_not_nan(gpu):
    pix, rows = make_pixels(5, 13), make_rows(257)
    for vis in (np.zeros(257, bool), np.where(rows["radii"] > 0, 0, rows["radii"]).astype(np.int32)):
        inp = dict(pix, amp_f_dc=rows["amp_f_dc"], visible=vis)
        got = host(call_row(on(gpu, inp)))
        check_row((5, 13, 257, "invisible", str(vis.dtype)), inp, got, "row f64")
        assert float(got["gs_sp_visible"]) == 0.0 and int(got["visible"]) == 0 and float(got["gs_sp"]) > 0


@pytest.mark.gpu
def test_train_log_row_matches_the_reference_fixture(gpu, golden):
    """the reference's own float32 scalars: within the same bounds of the device's row"""
    for c in CASES:
        g = dict(golden[c])
        inp = {k: g[k] for k in ("phasor", "gt_phasor", "depth", "gt_depth", "features_phasor", "visible") if k in g}
        inp.update(depth_range=float(g["depth_range"]), phase_offset=float(g["phase_offset"]), tof_multiplier=float(g["tof_multiplier"]))
        got = host(call_row(on(gpu, inp)))
        check_row(("golden", c), inp, got, "row f64")
        _, tols, n_vis = reference64(("golden", c), inp)
        for k in SLOTS:
            if k in g:
                err = abs(float(got[k]) - float(g[k]))
                _note("row fixture " + k, err / tols[k])
                assert err <= tols[k], (c, k, float(got[k]), float(g[k]), tols[k])
        assert sum(k in g for k in SLOTS) == (10 if c == "full" else 7)
        assert int(got["visible"]) == (int(g["visible"].sum()) if c == "full" else 0)


@pytest.mark.gpu
def test_bit_reproducible(gpu):
    pix, rows = make_pixels(513, 512), make_rows(70_001)
    t = on(gpu, dict(pix, features_phasor=rows["features_phasor"], visible=rows["radii"]))
    t["extras"] = (torch.tensor(1.5, device=gpu),)
    a, b = call_row(t), call_row(t)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(tof_depth(t), tof_depth(t))


def tof_depth(t):
    from gftorf_amd import tof
    return tof.depth_from_tof(t["phasor"][:3], t["depth_range"], t["phase_offset"])


@pytest.mark.gpu
def test_no_host_sync(gpu):
    """record, depth_from_tof and a drain that does not wait, with every device-to-host synchronisation an error"""
    from gftorf_amd import tof
    pix, rows = make_pixels(37, 53), make_rows(65)
    t = on(gpu, dict(pix, features_phasor=rows["features_phasor"], visible=rows["radii"]))
    t.update(depth_range=torch.tensor([7.5], device=gpu), phase_offset=torch.tensor(0.3, device=gpu), extras=(torch.tensor(2.0, device=gpu),))
    log = tof.TrainLog(slots=8)
    call_row(t, f=log.record)                   # warm-up: the library's first load and the scratch are not the question
    log.drain()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            call_row(t, f=log.record)
            tof_depth(t)
            rows_out, lost = log.drain()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    rest, lost = log.drain(wait=True)
    assert lost == 0 and int(rest["seq"][-1]) == 3


@pytest.mark.gpu
def test_ring_without_capture(gpu):
    from gftorf_amd import tof
    pix = make_pixels(7, 9)
    t = on(gpu, pix)
    log = tof.TrainLog(slots=4)
    extra = torch.zeros((), device=gpu)
    for k in range(6):
        extra.fill_(float(k))
        call_row(dict(t, extras=(extra,)), f=log.record)
    rows, lost = log.drain(wait=True)
    assert lost == 2 and rows["seq"].tolist() == [2, 3, 4, 5] and rows["extras"][:, 0].tolist() == [2.0, 3.0, 4.0, 5.0]
    single = host(call_row(dict(t, extras=(extra,))))
    for k in SLOTS:
        assert all(np.float32(v).tobytes() == np.float32(single[k]).tobytes() for v in rows[k]), k
    again, lost = log.drain(wait=True)
    assert lost == 0 and again["seq"].size == 0 and all(again[k].size == 0 for k in SLOTS)
    call_row(dict(t, extras=(extra,)), f=log.record)
    rows, lost = log.drain(wait=True)
    assert lost == 0 and rows["seq"].tolist() == [6]


@pytest.mark.gpu
def test_ring_under_capture(gpu):
    """a graph of one record replayed three times; between replays phasor, depth, radii, the offset tensor and one extra are
    rewritten in place: consecutive sequence numbers, each row bit for bit a fresh eager train_log_row of its inputs"""
    from gftorf_amd import tof
    H, W, P = 37, 53, 257
    rows = make_rows(P)
    t = on(gpu, dict(make_pixels(H, W), features_phasor=rows["features_phasor"], visible=rows["radii"]))
    t.update(depth_range=torch.tensor([7.5], device=gpu), phase_offset=torch.tensor(0.3, device=gpu),
             extras=(torch.tensor(1.0, device=gpu), torch.tensor([0.125], device=gpu)))
    log = tof.TrainLog(slots=8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            call_row(t, f=log.record)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call_row(t, f=log.record)
    fresh = []
    for k in range(3):
        rng = np.random.default_rng(50 + k)
        off = (0.3, -0.2, 0.1)[k]
        t["phasor"].copy_(torch.tensor(draw_phasor(rng, 7, H, W, off), device=gpu))
        t["depth"].copy_(torch.tensor(rng.uniform(0.3, 3.7, size=(1, H, W)).astype(np.float32), device=gpu))
        t["visible"].copy_(torch.tensor(np.where(rng.random(P) < 0.5, 3, 0).astype(np.int32), device=gpu))
        t["phase_offset"].fill_(off)
        t["extras"][0].fill_(10.0 + k)
        graph.replay()
        torch.cuda.synchronize()
        fresh.append(call_row(t).cpu().numpy())
    got, lost = log.drain(wait=True)
    assert lost == 0 and got["seq"].tolist() == [0, 1, 2, 3, 4]          # two warm-up records, then the replays
    assert got["extras"][2:, 0].tolist() == [10.0, 11.0, 12.0] and got["extras"][2:, 1].tolist() == [0.125] * 3
    assert all(0 < int(v) < P for v in got["visible"][2:])
    for k in range(3):
        want = tof.unpack(fresh[k])
        for name in SLOTS + ("visible", "present", "num_extras", "extras"):
            assert want[name][0].tobytes() == got[name][2 + k].tobytes(), (k, name)


@pytest.mark.gpu
def test_with_the_rasterizer(gpu):
    """A ToF call at 64x48: its phasor, depth, depth_distortion and radii straight into record, with the scene's phasor
    coefficients as features_phasor; against the float64 statements on the same tensors"""
    from gftorf_amd import GaussianRasterizer, tof
    P, W, H = 3000, 64, 48
    scene = Hh.small_scene(P=P, W=W, H=H, seed=21, scale_lo=0.01, scale_hi=0.08)
    g = scene["gaussians"]
    geo = {k: torch.tensor(g[k], dtype=torch.float32, device=gpu) for k in ("means3D", "opacities", "scales", "rotations", "shs", "shs_p")}
    rast = GaussianRasterizer(raster_settings=Hh.gpu_settings(scene, gpu))
    outs = rast(means3D=geo["means3D"], means2D=torch.zeros((P, 3), device=gpu), opacities=geo["opacities"], shs=geo["shs"],
                shs_p=geo["shs_p"], scales=geo["scales"], rotations=geo["rotations"], phase_offset=scene["phase_offset"],
                dc_offset=scene["dc_offset"])
    phasor, depth, dd, radii = outs[1], outs[2], outs[6], outs[10]
    assert phasor.shape[0] >= 3 and tuple(depth.shape) == (1, H, W) and tuple(geo["shs_p"].shape[1:]) == (16, 2)
    rng = np.random.default_rng(4)
    gt_phasor = torch.tensor(draw_phasor(rng, 3, H, W, scene["phase_offset"]), device=gpu)
    loss = torch.tensor(0.75, device=gpu)
    log = tof.TrainLog(slots=2)
    log.record(phasor, depth, gt_phasor, scene["depth_range"], scene["phase_offset"], depth_distortion=dd,
               features_phasor=geo["shs_p"], visible=radii, extras=(loss,))
    rows, lost = log.drain(wait=True)
    inp = dict(phasor=phasor.detach().cpu().numpy(), gt_phasor=gt_phasor.cpu().numpy(), depth=depth.detach().cpu().numpy(),
               dd=dd.detach().cpu().numpy(), features_phasor=geo["shs_p"].cpu().numpy(), visible=radii.cpu().numpy(),
               depth_range=scene["depth_range"], phase_offset=scene["phase_offset"], tof_multiplier=1.0)
    # the rendered phasor is not drawn to be well-conditioned: no pixel may sit on the +2 pi branch or at the clamp
    p64 = np.arctan2(inp["phasor"][1].astype(np.float64), inp["phasor"][0].astype(np.float64)) - f32(scene["phase_offset"])
    assert float(np.abs(p64).min()) > 1e-5 and float(np.abs(np.abs(inp["phasor"][0]) - 1e-6).min()) > 1e-8
    got = {k: v[0] for k, v in rows.items()}
    check_row("rasterizer", inp, got, "row rasterizer")
    assert lost == 0 and 0 < int(got["visible"]) < P and float(got["extras"][0]) == 0.75 and float(got["sp"]) > 0
