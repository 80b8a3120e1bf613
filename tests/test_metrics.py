"""gftorf_amd.metrics: a view's evaluation metrics (train.py:535-579; utils/image_utils.py:14-19; utils/loss_utils.py l1_loss /
l2_loss; scene/torf_utils.py:59-64).  The yardsticks are the reference's own float32 results (tests/golden/metrics.npz, written
by tests/golden/make_golden_metrics.py) and `view64` below -- train.py:535-566 restated, to be read against those lines -- run in
float64 on the CPU over the float32 inputs.

Inputs are drawn so that the reference alone is well-conditioned: colour values in [0, 1], every channel's mse at least 1e-4
(except where a test says otherwise), the wrapped phase after the offset in [0.05, 2 pi - 0.05] with no pixel changing its
`+ 2 pi` branch between float32 and float64 (`draw_phasor` asserts it).

Tolerances:
  l1*, l2*    |device - f64| <= 1e-6 * f64 (every term of these sums is non-negative): the per-element fp32 error of (a - b)^2 is
              about 2e-7 relative, and the sums finish in double.  The bound of tests/test_tof.py.
  psnr*       5e-6 dB per channel, and so for the mean over channels: d psnr = (10 / ln 10) d mse / mse.
  l2_d_tof    the above plus the ToF depth's own bound of tests/test_tof.py, eps = 4e-7 * depth_range / 2 per pixel, propagated
              through the square: 2 mean|pd - g| eps + eps^2.
  the fixture the reference's float32 results against `view64`: three times the distance measured when the fixture was written
              (stored in the npz as ref_err_rel for l1* / l2*, relative, and ref_err_db for psnr*, in dB), for the CPU test and
              for the device's three-view averages against the golden ones.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_metrics.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics.npz")
CASES = ("plain", "ragged", "full")
VALUES = ("l1", "psnr", "l1_p", "l2_p", "psnr_p", "l1_d", "l2_d", "l2_d_tof")
HAS_COLOUR, HAS_TOF, HAS_DEPTH, HAS_TOF_DEPTH = 1, 2, 4, 8
# (colour, ToF): one pixel; 63 / 64; 65 / 257; more than one workgroup with either camera the larger; 513 x 512 > 256 threads x
# the cap of 1024 workgroups, so the stride loop runs twice on one group while the other has ended
SHAPES = [((1, 1), (1, 1)), ((7, 9), (8, 8)), ((5, 13), (1, 257)), ((37, 53), (24, 32)), ((24, 32), (37, 53)),
          ((513, 512), (8, 8)), ((8, 8), (513, 512))]


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


def mse64(img1, img2):
    """image_utils.py:15"""
    return ((img1 - img2) ** 2).reshape(img1.shape[0], -1).mean(1, keepdims=True)


def psnr64(img1, img2):
    """image_utils.py:18-19; a channel without a difference gives +inf, as torch's 1.0 / 0 does"""
    with np.errstate(divide="ignore"):
        return 20 * np.log10(1.0 / np.sqrt(mse64(img1, img2)))


def l1_loss64(network_output, gt):
    return np.abs(network_output - gt).mean()


def l2_loss64(network_output, gt):
    return ((network_output - gt) ** 2).mean()


def view64(v):
    """train.py:535-566 for one view in float64: `v` holds the float32 inputs present (`image` / `gt_image`; `phasor` with
    `tof_planes` = (first, last) of the selected ToF channels and `gt_tof`; `depth`, `gt_depth`, `depth_range`,
    `phase_offset`).  Returns the eight values (0.0 where the reference adds nothing) and the bound of l2_d_tof's own term."""
    d = lambda a: np.asarray(a, np.float64)
    out = dict.fromkeys(VALUES, 0.0)
    extra = 0.0
    if "image" in v:
        rendered_image, gt_image = d(v["image"]), d(v["gt_image"])                              # :535-536
        out["l1"] = l1_loss64(rendered_image, gt_image).mean()                                   # :537
        out["psnr"] = psnr64(rendered_image, gt_image).mean()                                    # :538
    if "gt_tof" in v:
        first, last = v["tof_planes"]
        tof_rendered, tof_gt = d(v["phasor"][first:last]), d(v["gt_tof"])                       # :546 / :549
        out["l1_p"] = l1_loss64(tof_rendered, tof_gt).mean()                                     # :550
        out["l2_p"] = l2_loss64(tof_rendered, tof_gt).mean()                                     # :551
        out["psnr_p"] = psnr64(tof_rendered, tof_gt).mean()                                      # :552
    if "gt_depth" in v:                                                                          # :559
        gt_depth = d(v["gt_depth"])
        if "depth" in v:
            rendered_depth = d(v["depth"])                                                       # :561
            out["l1_d"] = l1_loss64(rendered_depth, gt_depth).mean()                             # :564
            out["l2_d"] = l2_loss64(rendered_depth, gt_depth).mean()                             # :565
        if "depth_range" in v:
            rendered_depth_tof = depth64(v["phasor"], f32(v["depth_range"]), f32(v["phase_offset"]))[None]     # :562-563
            out["l2_d_tof"] = l2_loss64(rendered_depth_tof, gt_depth).mean()                     # :566
            eps = 4e-7 * f32(v["depth_range"]) / 2
            extra = 2 * float(np.abs(rendered_depth_tof - gt_depth).mean()) * eps + eps * eps
    return {k: float(x) for k, x in out.items()}, extra


def bound(name, ref, extra=0.0):
    """the device's bound against the float64 value `ref` of the slot `name`"""
    if name.startswith("psnr"):
        return 5e-6
    return 1e-6 * abs(ref) + (extra if name == "l2_d_tof" else 0.0)


def present_of(v):
    return ((HAS_COLOUR if "image" in v else 0) | (HAS_TOF if "gt_tof" in v else 0) |
            (HAS_DEPTH if "gt_depth" in v and "depth" in v else 0) | (HAS_TOF_DEPTH if "gt_depth" in v and "depth_range" in v else 0))


# ---- inputs -------------------------------------------------------------------------------------------------------------

def draw_phasor(rng, planes, H, W, phase_offset):
    """as tests/golden/make_golden_metrics.py: planes 0 / 1 a vector of length 0.05-1 whose phase, less the offset and wrapped,
    lies in [0.05, 2 pi - 0.05]; a real part below 1e-4 is pushed out to 1e-4; the other planes in [-1, 1]"""
    off = f32(phase_offset)
    theta = rng.uniform(0.05, 2 * np.pi - 0.05, size=(H, W)) + off
    length = rng.uniform(0.05, 1.0, size=(H, W))
    out = rng.uniform(-1.0, 1.0, size=(planes, H, W))
    out[0], out[1] = length * np.cos(theta), length * np.sin(theta)
    out[0] = np.where(np.abs(out[0]) < 1e-4, np.copysign(1e-4, out[0]), out[0])
    out = out.astype(np.float32)
    p64 = np.arctan2(out[1].astype(np.float64), out[0].astype(np.float64)) - off
    p32 = np.arctan2(out[1], out[0]) - np.float32(off)
    assert np.array_equal(p64 < 0, p32 < 0), "a pixel changes its +2 pi branch between float32 and float64"
    return out


@functools.lru_cache(maxsize=None)
def make_view(colour, tof):
    """every input of one view: a 3-channel colour image of size `colour`; on the ToF sensor of size `tof` a 7-plane phasor, a
    ground truth for each of its planes, depth and gt_depth; depth_range 7.5, offset -0.2 or 0.3"""
    (Hc, Wc), (Ht, Wt) = colour, tof
    rng = np.random.default_rng(10_000 * Hc + 100 * Wc + 10 * Ht + Wt)
    off = -0.2 if (Ht * Wt) % 2 else 0.3
    noisy = lambda a, lo, hi: np.clip(a + rng.normal(0.0, 0.05, size=a.shape), lo, hi).astype(np.float32)
    out = dict(image=rng.uniform(0.0, 1.0, size=(3, Hc, Wc)).astype(np.float32), phasor=draw_phasor(rng, 7, Ht, Wt, off),
               depth=rng.uniform(0.3, 3.7, size=(1, Ht, Wt)).astype(np.float32), depth_range=7.5, phase_offset=off)
    out["gt_image"] = noisy(out["image"], 0.0, 1.0)
    out["gt_phasor"] = noisy(out["phasor"], -2.0, 2.0)
    out["gt_depth"] = (out["depth"] + rng.normal(0.0, 0.2, size=(1, Ht, Wt))).astype(np.float32)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def select(view, colour=3, tof=(0, 3), depth=True, tof_depth=True):
    """the inputs of one call: the first `colour` colour channels (0: none), the phasor's planes tof = (first, last) as the ToF
    channels (None: none), depth and the ToF depth against gt_depth"""
    v = {}
    if colour:
        v.update(image=view["image"][:colour], gt_image=view["gt_image"][:colour])
    if tof is not None or tof_depth:
        v["phasor"] = view["phasor"]
    if tof is not None:
        v.update(tof_planes=tof, gt_tof=view["gt_phasor"][tof[0]:tof[1]])
    if depth or tof_depth:
        v["gt_depth"] = view["gt_depth"]
    if depth:
        v["depth"] = view["depth"]
    if tof_depth:
        v.update(depth_range=view["depth_range"], phase_offset=view["phase_offset"])
    return v


_F64 = {}


def reference64(key, v):
    """float64 on the CPU, computed once per input set and shared"""
    if key not in _F64:
        _F64[key] = view64(v)
    return _F64[key]


def kwargs_on(dev, v, **over):
    """the keyword arguments of view_metrics / add_view for the inputs `v`; the ToF channels are a view of the device's phasor"""
    up = lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)
    kw = {k: up(v[k]) for k in ("image", "gt_image", "gt_tof", "depth", "gt_depth") if k in v}
    if "phasor" in v:
        phasor = up(v["phasor"])
        if "gt_tof" in v:
            kw["tof"] = phasor[v["tof_planes"][0]:v["tof_planes"][1]]
        if "depth_range" in v:
            kw.update(phasor=phasor, depth_range=v["depth_range"], phase_offset=v["phase_offset"])
    kw.update(over)
    return kw


MEASURED = {}          # largest error per check relative to its bound (pytest -s)


def _note(key, err):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(err))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nmetrics errors measured, relative to their bounds:", {k: "%.3g" % v for k, v in sorted(MEASURED.items())})


def check_values(key, v, got, what):
    """eight values (a sequence in the order of VALUES, or a dict) against the float64 statements"""
    ref, extra = reference64(key, v)
    got = got if isinstance(got, dict) else dict(zip(VALUES, (float(x) for x in got)))
    for k in VALUES:
        err, b = abs(got[k] - ref[k]), bound(k, ref[k], extra)
        print("%s %s: %.9g ref %.9g err %.3g bound %.3g" % (key, k, got[k], ref[k], err, b))
        if b > 0:
            _note("%s %s" % (what, k), err / b)
        assert err <= b, (key, k, got[k], ref[k], err, b)


# ---- CPU-runnable checks ------------------------------------------------------------------------------------------------

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
    out = {c: {k[len(c) + 1:]: z[k] for k in z.files if k.startswith(c + "_")} for c in CASES + ("avg",)}
    out["ref_err_rel"], out["ref_err_db"] = float(z["ref_err_rel"]), float(z["ref_err_db"])
    return out


def golden_view(g):
    """a fixture case as the inputs of `view64`"""
    v = {k: g[k] for k in ("image", "gt_image", "phasor", "gt_tof", "depth", "gt_depth") if k in g}
    v["tof_planes"] = tuple(int(x) for x in g["tof_planes"])
    if "gt_depth" in g:
        v.update(depth_range=float(g["depth_range"]), phase_offset=float(g["phase_offset"]))
    return v


def golden_bound(golden, name, ref):
    return 3 * (golden["ref_err_db"] if name.startswith("psnr") else golden["ref_err_rel"] * abs(ref))


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c_and_every_symbol_is_exported(tmp_path, lib):
    from gftorf_amd import _lib, build, metrics
    import gftorf_amd
    names = declared_functions()
    assert set(names) == set(_lib.METRICS_EXPORTS), names
    assert not set(names) & (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.FEATURE_EXPORTS) | set(_lib.REG_EXPORTS) |
                             set(_lib.TOF_EXPORTS) | set(_lib.QUERY_EXPORTS))
    for n in names:
        assert hasattr(lib, n), n
    assert "k_metrics.hip" in build.SOURCES and gftorf_amd.metrics is metrics
    prog = tmp_path / "metrics_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_metrics.h"', '#include "gftorf_tof.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "metrics_abi.o")])
    # the header's constants are the Python side's
    words = (["GFT_METRICS_" + k.upper() for k in VALUES] +
             ["GFT_METRICS_" + k for k in ("VALUES", "MAX_PLANES", "PARTIAL_WORDS", "ROW_MSE", "ROW_PSNR", "ROW_PRESENT", "ROW_PLANES",
                                           "ROW_WORDS", "ACC_SUMS", "ACC_VIEWS", "ACC_PRESENT", "ACC_WORDS", "HAS_COLOUR", "HAS_TOF",
                                           "HAS_DEPTH", "HAS_TOF_DEPTH")])
    out = subprocess.check_output(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-include", "gftorf_metrics.h",
                                   "-x", "c", "-"], input="METRICS_WORDS_ARE " + " ".join(words) + "\n", text=True)
    consts = [int(x) for x in out.split("METRICS_WORDS_ARE", 1)[1].split()]
    assert tuple(metrics.VALUES) == VALUES == _lib.METRICS_VALUES
    assert consts == list(range(8)) + [8, _lib.METRICS_MAX_PLANES, _lib.METRICS_PARTIAL_WORDS, _lib.METRICS_ROW_MSE, _lib.METRICS_ROW_PSNR,
                                       _lib.METRICS_ROW_PRESENT, _lib.METRICS_ROW_PLANES, _lib.METRICS_ROW_WORDS, _lib.METRICS_ACC_SUMS,
                                       _lib.METRICS_ACC_VIEWS, _lib.METRICS_ACC_PRESENT, _lib.METRICS_ACC_WORDS, HAS_COLOUR, HAS_TOF,
                                       HAS_DEPTH, HAS_TOF_DEPTH]
    assert (_lib.METRICS_HAS_COLOUR, _lib.METRICS_HAS_TOF, _lib.METRICS_HAS_DEPTH, _lib.METRICS_HAS_TOF_DEPTH) == (1, 2, 4, 8)
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16


def test_the_float64_statements_agree_with_the_reference_fixture(golden):
    """The reference's own float32 results (per view, and the three-view averages of train.py:570-579) against `view64`.  The
    bound is the float32 error of the reference's own means: tests/golden/make_golden_metrics.py measured the largest distance
    between the two when it wrote the fixture (ref_err_rel, relative, over l1* / l2*; ref_err_db, in dB, over psnr*), and three
    times that distance is allowed here."""
    assert 0 < golden["ref_err_rel"] < 1e-6 and 0 < golden["ref_err_db"] < 5e-6      # a float32 mean's error, not a disagreement
    total = dict.fromkeys(VALUES, 0.0)
    for c in CASES:
        ref, _ = view64(golden_view(golden[c]))
        for k in VALUES:
            got = float(golden[c][k])
            assert golden[c][k].dtype == np.float32
            assert abs(got - ref[k]) <= golden_bound(golden, k, ref[k]), (c, k, got, ref[k])
            total[k] += ref[k]
    for k in VALUES:
        assert golden["avg"][k].dtype == np.float64
        assert abs(float(golden["avg"][k]) - total[k] / 3) <= golden_bound(golden, k, total[k] / 3), (k, float(golden["avg"][k]), total[k] / 3)
    # what the cases are: ToF of the colour's size / of its own / both groups of 48 x 64; absent groups stay 0.0
    shapes = {c: (golden[c]["image"].shape, golden[c]["phasor"].shape, golden[c]["gt_tof"].shape) for c in CASES}
    assert shapes == {"plain": ((3, 24, 32), (3, 24, 32), (2, 24, 32)), "ragged": ((3, 37, 53), (7, 24, 40), (1, 24, 40)),
                      "full": ((3, 48, 64), (3, 48, 64), (3, 48, 64))}
    assert "gt_depth" not in golden["plain"] and all(float(golden["plain"][k]) == 0.0 for k in ("l1_d", "l2_d", "l2_d_tof"))
    assert tuple(golden["ragged"]["tof_planes"]) == (6, 7) and abs(float(golden["ragged"]["phase_offset"]) - 0.3) < 1e-6


def test_size_query_and_argument_errors(lib):
    import ctypes as C
    from gftorf_amd import _lib
    assert lib.gft_metrics_blocks(0) == 0 and lib.gft_metrics_blocks(-3) == 0
    assert lib.gft_metrics_blocks(1) == 1 and lib.gft_metrics_blocks(256) == 1 and lib.gft_metrics_blocks(257) == 2
    assert lib.gft_metrics_blocks(320 * 240) == 300 and lib.gft_metrics_blocks(513 * 512) == 1024 == lib.gft_metrics_blocks(1 << 40)
    x = C.c_void_p(16)                                         # never dereferenced: the calls fail before any launch

    def view(pa=4, ca=3, im=x, gi=x, pb=4, cb=3, tf=x, gt=x, d=x, gd=x, ph=x, stride=4, part=x, row=x, acc=None):
        return lib.gft_view_metrics(None, pa, ca, im, stride, gi, stride, pb, cb, tf, stride, gt, stride, d, gd, ph, stride, None, 7.5,
                                    None, 0.0, part, row, acc)
    for bad, msg in ((dict(ca=-1), "bad channel counts"), (dict(ca=9, cb=0), "bad channel counts"), (dict(cb=9), "bad channel counts"),
                     (dict(ca=4), "9 plane pairs, at most 8"), (dict(ca=0, cb=0, d=None, gd=None, ph=None), "no plane pair"),
                     (dict(pa=0), "bad sizes"), (dict(pb=-1), "bad sizes"), (dict(im=None), "image or gt_image is NULL"),
                     (dict(gi=None), "image or gt_image is NULL"), (dict(tf=None), "tof or gt_tof is NULL"),
                     (dict(gd=None), "without gt_depth"), (dict(d=None, ph=None), "gt_depth without depth or phasor"),
                     (dict(stride=-1), "bad plane stride"), (dict(part=None), "partials is NULL"), (dict(part=C.c_void_p(12)), "8-byte aligned"),
                     (dict(row=None), "row and accum are both NULL"), (dict(acc=C.c_void_p(20)), "accum is not 8-byte aligned")):
        assert view(**bad) != 0, bad
        assert msg in _lib.last_error(), (bad, _lib.last_error())
    assert lib.gft_metrics_reset(None, None) != 0 and "NULL" in _lib.last_error()
    assert lib.gft_metrics_reset(None, C.c_void_p(12)) != 0 and "8-byte aligned" in _lib.last_error()


def test_wrapper_rejects_cpu_tensors_shapes_and_nine_channels():
    from gftorf_amd import metrics
    im, ph, d = torch.rand(3, 4, 6), torch.rand(7, 5, 5), torch.rand(1, 5, 5)
    calls = [lambda: metrics.mse(im, im), lambda: metrics.psnr(im, im), lambda: metrics.view_metrics(image=im, gt_image=im),
             lambda: metrics.view_metrics(tof=ph[:2], gt_tof=ph[1:3], depth=d, gt_depth=d, phasor=ph, depth_range=7.5),
             lambda: metrics.EvalReport(device="cpu")]
    for c in calls:
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            c()
    shapes = [(lambda: metrics.mse(torch.rand(9, 4, 6), torch.rand(9, 4, 6)), "9 channels, one call takes 1..8"),
              (lambda: metrics.psnr(torch.rand(9, 4), torch.rand(9, 4)), "9 channels, one call takes 1..8"),
              (lambda: metrics.mse(im, im[:, :-1]), "img1 and img2 must have one shape"),
              (lambda: metrics.view_metrics(image=torch.rand(4, 4, 6), gt_image=torch.rand(4, 4, 6)), r"image must be \[1..3, H, W\]"),
              (lambda: metrics.view_metrics(image=im, gt_image=im[:2]), r"gt_image must be \[3, 4, 6\]"),
              (lambda: metrics.view_metrics(image=im[0], gt_image=im[0]), r"image must be \[1..3, H, W\]"),
              (lambda: metrics.view_metrics(tof=ph[:4], gt_tof=ph[:4]), r"tof must be \[1..3, H, W\]"),
              (lambda: metrics.view_metrics(tof=ph[:2], gt_tof=ph[:2], depth=im[:1], gt_depth=im[:1]), "the ToF camera's images have one size"),
              (lambda: metrics.view_metrics(depth=d, gt_depth=d[:, :-1]), "the ToF camera's images have one size"),
              (lambda: metrics.view_metrics(depth=ph[:2], gt_depth=d), r"depth must be \[1..1, H, W\]"),
              (lambda: metrics.view_metrics(gt_depth=d, phasor=ph[:1], depth_range=7.5), r"phasor must be \[>=2, H, W\]"),
              (lambda: metrics.view_metrics(gt_depth=d, phasor=ph, depth_range=torch.ones(2)), "depth_range must be a number or a one-element")]
    for c, msg in shapes:
        with pytest.raises(RuntimeError, match=msg):
            c()
    for c, msg in [(lambda: metrics.view_metrics(image=im), "image and gt_image come together, gt_image is missing"),
                   (lambda: metrics.view_metrics(gt_tof=ph[:2]), "tof and gt_tof come together, tof is missing"),
                   (lambda: metrics.view_metrics(depth=d), "gt_depth, which is missing"),
                   (lambda: metrics.view_metrics(image=im, gt_image=im, gt_depth=d), "gt_depth is given without depth or phasor"),
                   (lambda: metrics.view_metrics(gt_depth=d, phasor=ph), "needs depth_range"),
                   (lambda: metrics.view_metrics(), "nothing to compare")]:
        with pytest.raises(ValueError, match=msg):
            c()
    with pytest.raises(TypeError, match="image must be a tensor"):
        metrics.view_metrics(image=im.numpy(), gt_image=im)
    with pytest.raises(TypeError, match="gt_image must be torch.float32"):
        metrics.view_metrics(image=im, gt_image=im.double())


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_view_metrics_matches_the_float64_statements(shape, gpu):
    """all eight planes: 3 colour channels, 3 ToF channels, depth and the ToF depth; the two cameras' sizes differ"""
    from gftorf_amd import metrics
    v = select(make_view(*shape))
    got = metrics.view_metrics(**kwargs_on(gpu, v))
    assert tuple(got.shape) == (8,) and got.dtype == torch.float32 and not got.requires_grad and got.device.type == "cuda"
    check_values(shape, v, got.cpu().numpy(), "view f64")


@pytest.mark.gpu
@pytest.mark.parametrize("colour", [1, 3])
@pytest.mark.parametrize("tof", [(0, 1), (0, 2), (0, 3), (6, 7), (4, 6)], ids=lambda t: "planes%d-%d" % t)
def test_channel_counts_and_planes_read_in_place(colour, tof, gpu, monkeypatch):
    """colour 1 and 3; ToF 1, 2, 3; one quad plane (and two) of the 7-plane phasor as a view: the pointer handed to the C call
    is the wide tensor's plane, the stride its own"""
    from gftorf_amd import metrics
    v = select(make_view((37, 53), (24, 32)), colour=colour, tof=tof)
    kw = kwargs_on(gpu, v, gt_image=torch.tensor(v["gt_image"], device=gpu).requires_grad_())
    real, seen = metrics._lib.load(), []

    class Spy:
        def __getattr__(self, name):
            def f(*args):
                seen.append((name, args))
                return getattr(real, name)(*args)
            return f
    monkeypatch.setattr(metrics._lib, "load", lambda: Spy())
    got = metrics.view_metrics(**kw)
    assert not got.requires_grad and got.grad_fn is None
    check_values(((37, 53), (24, 32), colour, tof), v, got.cpu().numpy(), "channels f64")
    args = [a for name, a in seen if name == "gft_view_metrics"]
    assert len(args) == 1 and args[0][1:3] == (37 * 53, colour) and args[0][7:9] == (24 * 32, tof[1] - tof[0])
    assert args[0][9] == kw["phasor"][tof[0]].data_ptr() and args[0][10] == (24 * 32 if tof[1] - tof[0] > 1 else 0)
    assert args[0][15] == kw["phasor"].data_ptr() and args[0][16] == 24 * 32


@pytest.mark.gpu
def test_absent_groups_leave_zero_and_clear_their_bit(gpu):
    from gftorf_amd import _lib, metrics
    view = make_view((37, 53), (24, 32))
    for what in (dict(tof=None), dict(depth=False, tof_depth=False), dict(tof=None, depth=False, tof_depth=False), dict(depth=False),
                 dict(tof_depth=False), dict(colour=0), dict(colour=0, tof=None, tof_depth=False), dict()):
        v = select(view, **what)
        row = torch.empty(_lib.METRICS_ROW_WORDS, device=gpu)
        metrics._launch(row, None, None, **kwargs_on(gpu, v))
        host = row.cpu().numpy()
        key = ((37, 53), (24, 32), tuple(sorted(what.items())))
        check_values(key, v, host[:8], "absent f64")
        assert int(host.view(np.uint32)[_lib.METRICS_ROW_PRESENT]) == present_of(v), what
        zero = [k for k, bit in (("l1", 1), ("psnr", 1), ("l1_p", 2), ("l2_p", 2), ("psnr_p", 2), ("l1_d", 4), ("l2_d", 4), ("l2_d_tof", 8))
                if not present_of(v) & bit]
        assert all(host[VALUES.index(k)] == 0.0 for k in zero) and all(host[VALUES.index(k)] != 0.0 for k in VALUES if k not in zero)
        planes = int(host.view(np.uint32)[_lib.METRICS_ROW_PLANES])
        assert planes == sum((len(v.get("image", ())), len(v.get("gt_tof", ())), "depth" in v, "depth_range" in v))
        assert not host[_lib.METRICS_ROW_MSE + planes:_lib.METRICS_ROW_PSNR].any() and not host[_lib.METRICS_ROW_PSNR + planes:_lib.METRICS_ROW_PRESENT].any()
        report = metrics.EvalReport(device=gpu)
        report.add_view(**kwargs_on(gpu, v))
        res = report.result()
        assert res["present"] == present_of(v) and res["views"] == 1 and all(res[k] == 0.0 for k in zero)


@pytest.mark.gpu
def test_identical_images_give_zero_and_infinity(gpu):
    """l1 == 0 and psnr == +inf, as the reference: no clamp; one identical channel of three makes the mean infinite too"""
    from gftorf_amd import metrics
    view = make_view((37, 53), (24, 32))
    im, ph = torch.tensor(view["image"], device=gpu), torch.tensor(view["phasor"], device=gpu)
    got = metrics.view_metrics(image=im, gt_image=im.clone(), tof=ph[:2], gt_tof=ph[:2].clone()).cpu().numpy()
    assert got[0] == 0.0 and got[1] == np.inf and got[2] == 0.0 and got[3] == 0.0 and got[4] == np.inf
    assert torch.equal(metrics.psnr(im, im.clone()).cpu(), torch.full((3, 1), float("inf")))
    assert torch.equal(metrics.mse(im, im.clone()).cpu(), torch.zeros(3, 1))
    gt = torch.tensor(view["gt_image"], device=gpu)
    gt[1] = im[1]
    per_channel = metrics.psnr(im, gt).cpu().numpy()
    assert per_channel[1, 0] == np.inf and np.isfinite(per_channel[[0, 2], 0]).all()
    assert metrics.view_metrics(image=im, gt_image=gt).cpu().numpy()[1] == np.inf
    report = metrics.EvalReport(device=gpu)
    report.add_view(image=im, gt_image=gt)
    assert report.result()["psnr"] == np.inf


@pytest.mark.gpu
def test_scalars_by_value_and_from_the_device_give_the_same_bits(gpu):
    from gftorf_amd import metrics
    v = select(make_view((37, 53), (24, 32)))
    kw = kwargs_on(gpu, v)
    by_value = metrics.view_metrics(**kw)
    dr, off = torch.tensor([v["depth_range"]], device=gpu), torch.tensor(v["phase_offset"], device=gpu)
    bits = lambda t: t.view(torch.int32)
    for over in (dict(depth_range=dr, phase_offset=off), dict(depth_range=dr), dict(phase_offset=off)):
        assert torch.equal(bits(metrics.view_metrics(**dict(kw, **over))), bits(by_value)), sorted(over)
    dr.fill_(9.0)
    off.fill_(0.25)
    moved = metrics.view_metrics(**dict(kw, depth_range=dr, phase_offset=off))                  # read when the kernel runs
    assert torch.equal(bits(moved), bits(metrics.view_metrics(**dict(kw, depth_range=9.0, phase_offset=0.25))))
    assert torch.equal(bits(moved[:7]), bits(by_value[:7])) and moved[7] != by_value[7]


@pytest.mark.gpu
def test_mse_and_psnr_drop_ins(gpu):
    """[C, 1] as image_utils.py:14-19; C up to 8, any trailing shape; the values of `mse64` / `psnr64` at the bounds above"""
    from gftorf_amd import metrics
    view = make_view((37, 53), (24, 32))
    for a, b in ((view["image"], view["gt_image"]), (view["phasor"], view["gt_phasor"]), (view["image"][:1], view["gt_image"][:1]),
                 (np.concatenate([view["phasor"], view["depth"]]), np.concatenate([view["gt_phasor"], view["gt_depth"]])),
                 (view["image"].reshape(3, -1), view["gt_image"].reshape(3, -1))):
        ta, tb = torch.tensor(a, device=gpu).requires_grad_(), torch.tensor(b, device=gpu)
        m, p = metrics.mse(ta, tb), metrics.psnr(ta, tb)
        C = a.shape[0]
        assert tuple(m.shape) == tuple(p.shape) == (C, 1) and m.dtype == p.dtype == torch.float32 and not m.requires_grad and m.device == ta.device
        m64, p64 = mse64(a.astype(np.float64), b.astype(np.float64)), psnr64(a.astype(np.float64), b.astype(np.float64))
        em, ep = np.abs(m.cpu().numpy() - m64) / m64, np.abs(p.cpu().numpy() - p64)
        _note("mse drop-in", em.max() / 1e-6)
        _note("psnr drop-in", ep.max() / 5e-6)
        assert (em <= 1e-6).all() and (ep <= 5e-6).all(), (C, em.max(), ep.max())
    nine = torch.rand(9, 4, 6, device=gpu)
    with pytest.raises(RuntimeError, match="9 channels, one call takes 1..8"):
        metrics.mse(nine, nine)
    with pytest.raises(RuntimeError, match="9 channels, one call takes 1..8"):
        metrics.psnr(nine, nine)


def add_golden_views(report, golden, dev):
    for c in CASES:
        report.add_view(**kwargs_on(dev, golden_view(golden[c])))


@pytest.mark.gpu
def test_eval_report_accumulates_three_views(gpu, golden):
    """the fixture's three views, of three shapes: each against its float64 statements and the reference's float32 values; the
    averages against the float64 average at the device's bounds and against the golden averages at the CPU test's bound"""
    from gftorf_amd import metrics
    report = metrics.EvalReport(device=gpu)
    total, extra = dict.fromkeys(VALUES, 0.0), 0.0
    for c in CASES:
        v = golden_view(golden[c])
        ref, e = reference64(("golden", c), v)
        got = metrics.view_metrics(**kwargs_on(gpu, v)).cpu().numpy()
        check_values(("golden", c), v, got, "fixture f64")
        for k in VALUES:
            total[k] += ref[k]
        extra += e
    add_golden_views(report, golden, gpu)
    res = report.result()
    assert res["views"] == 3 and res["present"] == 15 and set(res) == set(VALUES) | {"views", "present"}
    for k in VALUES:
        ref = total[k] / 3
        err, b = abs(res[k] - ref), bound(k, ref, extra / 3)
        print("average %s: %.12g ref %.12g golden %.12g err %.3g bound %.3g golden bound %.3g"
              % (k, res[k], ref, float(golden["avg"][k]), err, b, golden_bound(golden, k, ref)))
        _note("average f64 " + k, err / b)
        assert err <= b, (k, res[k], ref, err, b)
        e32 = abs(res[k] - float(golden["avg"][k]))
        _note("average fixture " + k, e32 / golden_bound(golden, k, ref))
        assert e32 <= golden_bound(golden, k, ref), (k, res[k], float(golden["avg"][k]), e32, golden_bound(golden, k, ref))


@pytest.mark.gpu
def test_reset_and_bit_reproducibility(gpu, golden):
    """the same view twice gives identical rows; the same three views in the same order give identical sums, from a fresh
    report and from one that was used and reset"""
    from gftorf_amd import metrics
    v = select(make_view((513, 512), (8, 8)))
    kw = kwargs_on(gpu, v)
    a, b = metrics.view_metrics(**kw), metrics.view_metrics(**kw)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    first, second = metrics.EvalReport(device=gpu), metrics.EvalReport(device="cuda")          # without an index: the current one
    add_golden_views(first, golden, gpu)
    add_golden_views(second, golden, gpu)
    fresh = first._sums.clone()
    assert torch.equal(fresh.view(torch.int32), second._sums.view(torch.int32))
    second.add_view(**kw)
    assert not torch.equal(fresh.view(torch.int32), second._sums.view(torch.int32)) and second.result()["views"] == 4
    second.reset()
    assert not second._sums.view(torch.int32).any()
    with pytest.raises(RuntimeError, match="no view was added"):
        second.result()
    add_golden_views(second, golden, gpu)
    assert torch.equal(fresh.view(torch.int32), second._sums.view(torch.int32)) and second.result() == first.result()


@pytest.mark.gpu
def test_no_host_sync(gpu):
    """add_view, view_metrics, the drop-ins and reset with every device-to-host synchronisation an error"""
    from gftorf_amd import metrics
    v = select(make_view((37, 53), (24, 32)))
    kw = kwargs_on(gpu, v)
    on_device = dict(kw, depth_range=torch.tensor([7.5], device=gpu), phase_offset=torch.tensor(0.3, device=gpu))
    report = metrics.EvalReport(device=gpu)
    report.add_view(**kw)                       # warm-up: the library's first load is not the question
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        report.reset()
        for _ in range(2):
            report.add_view(**kw)
            report.add_view(**on_device)
            metrics.view_metrics(**on_device)
            metrics.psnr(kw["image"], kw["gt_image"])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert report.result()["views"] == 4


@pytest.mark.gpu
def test_add_view_under_capture(gpu):
    """a graph of one add_view replayed three times; between replays every static input and the offset tensor are rewritten in
    place: the report equals, bit for bit, an eager report of the same three views"""
    from gftorf_amd import metrics
    shape = ((37, 53), (24, 32))
    kw = kwargs_on(gpu, select(make_view(*shape)))
    kw.update(depth_range=torch.tensor([7.5], device=gpu), phase_offset=torch.tensor(0.3, device=gpu))
    report, eager = metrics.EvalReport(device=gpu), metrics.EvalReport(device=gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            report.add_view(**kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        report.add_view(**kw)
    report.reset()                              # the two warm-up views
    for k in range(3):
        rng = np.random.default_rng(70 + k)
        off = (0.3, -0.2, 0.1)[k]
        kw["phasor"].copy_(torch.tensor(draw_phasor(rng, 7, 24, 32, off), device=gpu))          # kw["tof"] is a view of it
        for name in ("image", "gt_image", "gt_tof", "depth", "gt_depth"):
            kw[name].copy_(torch.tensor(rng.uniform(0.0, 1.0, size=tuple(kw[name].shape)).astype(np.float32), device=gpu))
        kw["phase_offset"].fill_(off)
        graph.replay()
        torch.cuda.synchronize()
        eager.add_view(**kw)
    got, want = report.result(), eager.result()
    assert got["views"] == 3 and got["present"] == 15
    assert torch.equal(report._sums.view(torch.int32), eager._sums.view(torch.int32)) and got == want
    assert all(np.isfinite(got[k]) and got[k] > 0 for k in VALUES)
