"""gftorf_amd.reg: the four regularisers of train.py:237-240 and :266-277 (motion, depth distortion, opacity entropy of the
dynamic Gaussians, scale of the visible ones).  The reference has them as inline statements only, so the yardstick is
`statements` below -- train.py:240, 267, 271-272, 276-277 restated, to be read against those lines -- run in float64 on the
CPU, and the same statements run eagerly in fp32 by torch on the device.

Tolerances:
  value of a term   (depth + 1) * 2^-24 * sum|t_i| / N, depth = the fp32 additions on the longest path of k_reg_fwd's
                    summation tree in front of the double-precision finish: k per thread + 6 wave shuffles + 3 LDS slots,
                    k = ceil(T / (workgroups * 256)) (<= 4 up to 2^20 elements)
  gradients         the larger of 2 x the largest absolute error of torch's eager fp32 autograd against float64 on the same
                    inputs, and 4 * 2^-24 * max|g|
  row counts        exact
"""
import ctypes as C
import functools
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_reg.h")
TERMS = ("mlp", "oe", "scale", "dd")
EPS24 = 2.0 ** -24


# ---- the restatement ---------------------------------------------------------------------------------------------------

def statements(t, raw):
    """The per-element tensors whose `.mean()` the reference adds to the loss, for the inputs present in `t` (tensors of any
    one dtype and device): d_xyz; opacity with mask (bool); scaling with visible (bool); dd."""
    out = {}
    if "d_xyz" in t:
        out["mlp"] = torch.abs(t["d_xyz"])                                                    # train.py:240
    if "opacity" in t:
        get_opacity = torch.sigmoid(t["opacity"]) if raw else t["opacity"]                    # gaussian_model.py get_opacity
        dynamic_opacities = get_opacity[t["mask"]]                                            # train.py:271
        out["oe"] = (-dynamic_opacities * torch.log(dynamic_opacities + 1e-10)
                     - (1 - dynamic_opacities) * torch.log(1 - dynamic_opacities + 1e-10))    # train.py:272
    if "scaling" in t:
        get_scaling = torch.exp(t["scaling"]) if raw else t["scaling"]
        if get_scaling.shape[1] == 1:
            get_scaling = get_scaling.repeat(1, 3)                                            # gaussian_model.py:125
        vis_scales = get_scaling[t["visible"]]                                                # train.py:276
        out["scale"] = vis_scales.mean(dim=-1) ** 2                                           # train.py:277
    if "dd" in t:
        out["dd"] = t["dd"]                                                                   # train.py:267
    return out


LEAF = {"mlp": "d_xyz", "oe": "opacity", "scale": "scaling", "dd": "dd"}


def run_statements(inp, raw, weights, up, dtype, dev):
    """means, mean |t_i|, counts and the gradients of up * sum(w_k * mean_k), by torch autograd in `dtype` on `dev`.  An
    empty selection counts as 0 with zero gradients (the documented difference from the reference's NaN)."""
    t = {}
    for k, v in inp.items():
        if k == "visible":
            t[k] = torch.tensor(v > 0 if v.dtype != np.bool_ else v, device=dev)
        elif k == "mask":
            t[k] = torch.tensor(v, device=dev)
        else:
            t[k] = torch.tensor(v, dtype=dtype, device=dev, requires_grad=True)
    elems = statements(t, raw)
    means, absmeans, loss = {}, {}, 0.0
    for k, e in elems.items():
        if e.numel() == 0:
            means[k], absmeans[k] = 0.0, 0.0
            continue
        m = e.mean()
        loss = loss + weights[k] * m
        means[k], absmeans[k] = float(m.detach()), float(e.detach().abs().mean())
    if isinstance(loss, torch.Tensor):
        (up * loss).backward()
    grads = {k: (t[LEAF[k]].grad if t[LEAF[k]].grad is not None else torch.zeros_like(t[LEAF[k]])).detach() for k in elems}
    counts = (int(t["mask"].sum()) if "mask" in t else 0, int(t["visible"].sum()) if "visible" in t else 0)
    return means, absmeans, counts, grads


# ---- inputs -------------------------------------------------------------------------------------------------------------

PATTERNS = ("none_dynamic", "all_dynamic_radii", "mixed_bool", "none_visible")
WEIGHTS = dict(mlp=0.7, oe=0.3, scale=1.9, dd=0.05)
EXTREME_RAW = (-120.0, -20.0, 0.0, 20.0, 120.0)


@functools.lru_cache(maxsize=None)
def make_inputs(P, pattern, cols, raw, seed=0, extreme=False):
    """d_xyz [Nd, 3] with exact zeros, opacity [P, 1], scaling [P, cols], a 7x9 distortion image (63 is no multiple of 4),
    the mask and the visibility of the pattern.  Raw tensors are logits / logs of the same activated values."""
    rng = np.random.default_rng(1000 * P + 10 * seed + cols + (5 if raw else 0))
    Nd = max(1, (3 * P) // 10)
    d_xyz = (0.05 * rng.standard_normal((Nd, 3))).astype(np.float32)
    d_xyz[rng.random((Nd, 3)) < 0.2] = 0.0
    d_xyz[0, 0] = 0.0
    o = rng.uniform(0.02, 0.98, (P, 1))
    s = np.exp(rng.uniform(np.log(0.004), np.log(0.3), (P, cols)))
    opacity = (np.log(o / (1 - o)) if raw else o).astype(np.float32)
    scaling = (np.log(s) if raw else s).astype(np.float32)
    if extreme:
        assert raw and P >= 2 * len(EXTREME_RAW)
        opacity[:len(EXTREME_RAW), 0] = EXTREME_RAW
        opacity[-len(EXTREME_RAW):, 0] = EXTREME_RAW
    mask = {"none_dynamic": np.zeros(P, bool), "all_dynamic_radii": np.ones(P, bool)}.get(pattern)
    if mask is None:
        mask = rng.random(P) < 0.3
        if extreme:
            mask[:len(EXTREME_RAW)] = True
    if pattern == "all_dynamic_radii":        # the rasterizer's radii: 0 and negative values are invisible
        visible = rng.integers(-3, 40, P).astype(np.int32)
        visible[rng.random(P) < 0.4] = 0
        visible[0] = 0
        visible[-1] = -7
    elif pattern == "none_visible":
        visible = np.zeros(P, bool)
    else:
        visible = rng.random(P) < 0.6
    dd = rng.uniform(0.0, 0.4, (1, 7, 9)).astype(np.float32)
    for a in (d_xyz, opacity, scaling, mask, visible, dd):
        a.setflags(write=False)
    return dict(d_xyz=d_xyz, opacity=opacity, mask=mask, scaling=scaling, visible=visible, dd=dd)


def subset(inp, present):
    keep = {"mlp": ("d_xyz",), "oe": ("opacity", "mask"), "scale": ("scaling", "visible"), "dd": ("dd",)}
    return {k: inp[k] for name in present for k in keep[name]}


_F64 = {}


def reference64(key, inp, raw, up):
    """float64 on the CPU, computed once per input set and shared"""
    key = (key, up)
    if key not in _F64:
        _F64[key] = run_statements(inp, raw, WEIGHTS, up, torch.float64, "cpu")
    return _F64[key]


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
    from gftorf_amd import _lib
    names = declared_functions()
    assert set(names) == set(_lib.REG_EXPORTS), names
    assert not set(names) & (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.FEATURE_EXPORTS))
    for n in names:
        assert hasattr(lib, n), n
    prog = tmp_path / "reg_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_reg.h"', '#include "gftorf_loss.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "reg_abi.o")])
    # the header's constants are the Python side's
    out = subprocess.check_output(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-include", "gftorf_reg.h",
                                   "-x", "c", "-"], input="REG_WORDS_ARE GFT_REG_PARTIAL_WORDS GFT_REG_MEANS GFT_REG_COUNTS GFT_REG_RECIPS GFT_REG_TOTAL\n",
                                  text=True)
    consts = [int(v) for v in out.split("REG_WORDS_ARE", 1)[1].split()]
    assert consts == [_lib.REG_PARTIAL_WORDS, _lib.REG_MEANS, _lib.REG_COUNTS, _lib.REG_RECIPS, _lib.REG_TOTAL]
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16
    assert lib.gft_reg_result_words() > _lib.REG_TOTAL


def test_size_query_and_argument_errors(lib):
    from gftorf_amd import _lib
    assert lib.gft_reg_blocks(0, 0, 0) == 0
    assert lib.gft_reg_blocks(-3, 5, 5) == 0 and lib.gft_reg_blocks(3, -1, 5) == 0 and lib.gft_reg_blocks(3, 5, -1) == 0
    assert lib.gft_reg_blocks(3, 0, 0) == 1 and lib.gft_reg_blocks(0, 1, 0) == 1 and lib.gft_reg_blocks(0, 0, 1) == 1
    assert lib.gft_reg_blocks(0, 512, 0) == 1 and lib.gft_reg_blocks(3, 512, 0) == 2      # four elements per thread, 256 threads
    assert lib.gft_reg_blocks(90_000, 100_000, 320 * 240) == 359
    assert lib.gft_reg_blocks(900_000, 1_000_000, 640 * 480) == 1024                        # then grid-stride
    x = C.c_void_p(16)                                         # never dereferenced: the calls fail before any launch
    w = (None, 1.0, 1.0, 1.0, 1.0)
    fwd = lambda n, P, px, d, o, m, s, cols, v, dd, part=x, res=x: lib.gft_reg_forward(None, n, P, px, d, o, m, 1, s, cols, 1, v, 1, dd,
                                                                                      *w, part, res)
    bwd = lambda n, P, px, d, o, m, s, cols, v, res, g, gd, go, gs, gdd: lib.gft_reg_backward(None, n, P, px, d, o, m, 1, s, cols, 1, v, 1,
                                                                                               *w, res, g, gd, go, gs, gdd)
    for bad in ((-3, 4, 4), (3, -4, 4), (3, 4, -4), (4, 4, 4)):          # (n_dxyz is 3 * Nd)
        assert fwd(*bad, x, x, x, x, 3, x, x) != 0
        assert "bad sizes" in _lib.last_error(), bad
        assert bwd(*bad, x, x, x, x, 3, x, x, x, x, x, x, x) != 0
        assert "bad sizes" in _lib.last_error(), bad
    cases = [((x, None, x, 3, x), "opacity without its motion_mask"), ((None, x, x, 3, x), "motion_mask without its opacity"),
             ((x, x, x, 3, None), "scaling without its visible"), ((x, x, None, 3, x), "visible without its scaling"),
             ((x, x, x, 2, x), "scaling_cols=2 is neither 1 nor 3"), ((x, x, x, 0, x), "scaling_cols=0 is neither 1 nor 3")]
    for (o, m, s, cols, v), msg in cases:
        assert fwd(3, 4, 4, x, o, m, s, cols, v, x) != 0
        assert msg in _lib.last_error(), msg
        assert bwd(3, 4, 4, x, o, m, s, cols, v, x, x, x, None, None, x) != 0
        assert msg in _lib.last_error(), msg
    assert fwd(3, 4, 4, x, x, x, x, 3, x, x, part=None) != 0
    assert "NULL" in _lib.last_error()
    assert fwd(3, 4, 4, x, x, x, x, 3, x, x, res=None) != 0
    assert "NULL" in _lib.last_error()
    assert fwd(3, 4, 4, None, None, None, None, 3, None, None) != 0
    assert "no term" in _lib.last_error()
    assert bwd(3, 4, 4, x, x, x, x, 3, x, None, x, x, x, x, x) != 0
    assert "NULL" in _lib.last_error()
    assert bwd(3, 4, 4, None, x, x, x, 3, x, x, x, x, x, x, x) != 0
    assert "a gradient without its tensor" in _lib.last_error()
    # backward with no gradient to write: nothing to launch, success
    assert bwd(3, 4, 4, x, x, x, x, 3, x, x, x, None, None, None, None) == 0


def test_wrapper_rejects_cpu_tensors_shapes_and_mask_gradients():
    from gftorf_amd import reg
    P = 6
    d, o, s, dd = torch.zeros(4, 3), torch.full((P, 1), 0.5), torch.ones(P, 3), torch.zeros(1, 7, 9)
    m, v, radii = torch.zeros(P, dtype=torch.bool), torch.ones(P, dtype=torch.bool), torch.ones(P, dtype=torch.int32)
    calls = [lambda: reg.regularizers(d_xyz=d, w_mlp=1.0, opacity=o, motion_mask=m, w_oe=1.0, scaling=s, visible=radii, w_scale=1.0,
                                      depth_distortion=dd, w_dd=1.0),
             lambda: reg.regularizers(d_xyz=d, opacity=o, motion_mask=m, weights=torch.ones(4)),
             lambda: reg.motion_reg(d), lambda: reg.dd_loss(dd), lambda: reg.opacity_entropy(o, m), lambda: reg.opacity_entropy(o[:, 0], m, raw=True),
             lambda: reg.scale_loss(s, v), lambda: reg.scale_loss(s[:, :1], radii, raw=True)]
    for c in calls:
        with pytest.raises(RuntimeError, match="HIP device only, there is no CPU path"):
            c()
    shapes = [(lambda: reg.motion_reg(torch.zeros(4, 2)), r"d_xyz must be \[\*, 3\]"),
              (lambda: reg.motion_reg(torch.zeros(12)), r"d_xyz must be \[\*, 3\]"),
              (lambda: reg.opacity_entropy(torch.zeros(P, 2), m), r"opacity must be \[P, 1\] or \[P\]"),
              (lambda: reg.opacity_entropy(o, m[:-1]), r"motion_mask must be \[6\]"),
              (lambda: reg.opacity_entropy(o, m[:, None]), r"motion_mask must be \[6\]"),
              (lambda: reg.scale_loss(torch.ones(P, 2), v), r"scaling must be \[P, 3\] or \[P, 1\]"),
              (lambda: reg.scale_loss(torch.ones(P), v), r"scaling must be \[P, 3\] or \[P, 1\]"),
              (lambda: reg.scale_loss(s, radii[:-1]), r"visible must be \[6\]"),
              (lambda: reg.regularizers(opacity=o, motion_mask=m, w_oe=1.0, scaling=torch.ones(P + 1, 3), visible=torch.ones(P + 1, dtype=torch.bool),
                                        w_scale=1.0), r"scaling must be \[6, 3\] or \[6, 1\]"),
              (lambda: reg.regularizers(d_xyz=d, weights=torch.ones(3)), r"weights must be \[4\]")]
    for c, msg in shapes:
        with pytest.raises(RuntimeError, match=msg):
            c()
    with pytest.raises(NotImplementedError, match="motion_mask requires grad"):
        reg.opacity_entropy(o, torch.zeros(P, requires_grad=True))
    with pytest.raises(NotImplementedError, match="visible requires grad"):
        reg.scale_loss(s, torch.ones(P, requires_grad=True))
    with pytest.raises(NotImplementedError, match="weights requires grad"):
        reg.regularizers(d_xyz=d, weights=torch.ones(4, requires_grad=True))
    with pytest.raises(TypeError, match="motion_mask must be torch.bool"):
        reg.opacity_entropy(o, torch.zeros(P))
    with pytest.raises(TypeError, match="visible must be torch.bool or torch.int32"):
        reg.scale_loss(s, torch.ones(P, dtype=torch.int64))
    with pytest.raises(TypeError, match="opacity must be torch.float32"):
        reg.opacity_entropy(o.double(), m)
    with pytest.raises(ValueError, match="opacity and motion_mask come together"):
        reg.regularizers(opacity=o, w_oe=1.0)
    # absent terms: None, a Python number for d_xyz (train.py:164), a float weight of 0.0 -- nothing left is the float 0.0
    assert reg.regularizers() == 0.0
    assert reg.regularizers(d_xyz=0.0, w_mlp=1.0) == 0.0
    assert reg.regularizers(d_xyz=d, w_mlp=0.0, opacity=o, motion_mask=m, w_oe=0.0, depth_distortion=dd) == 0.0
    assert reg.regularizers(d_xyz=0.0, w_mlp=1.0, return_terms=True) == (0.0, None)
    assert reg.regularizers(d_xyz=0.0, w_mlp=1.0, opacity=None, motion_mask=m, w_oe=1.0, scaling=None, visible=radii, w_scale=1.0) == 0.0
    with pytest.raises(ValueError, match="scaling and visible come together"):
        reg.regularizers(scaling=s, w_scale=1.0)


# ---- GPU ---------------------------------------------------------------------------------------------------------------

MEASURED = {}          # largest error per check relative to its bound, and both routes' gradient errors (pytest -s)


def _note(key, err):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(err))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nreg errors measured:", {k: "%.3g" % v for k, v in sorted(MEASURED.items())})


def depth_of(lib, inp):
    """fp32 additions on the longest path of k_reg_fwd's tree for these inputs: per thread, wave shuffles, LDS slots"""
    rows = max(inp["opacity"].shape[0] if "opacity" in inp else 0, inp["scaling"].shape[0] if "scaling" in inp else 0)
    sizes = (inp["d_xyz"].size if "d_xyz" in inp else 0, rows, inp["dd"].size if "dd" in inp else 0)
    total = sizes[0] + 2 * sizes[1] + sizes[2]
    return math.ceil(total / (lib.gft_reg_blocks(*sizes) * 256)) + 6 + 3


def fused(inp, raw, dev, up=1.0, weights=WEIGHTS, weights_tensor=None):
    """regularizers forward + backward on the inputs present: (loss, means, counts, grads)"""
    from gftorf_amd import reg
    t = {k: torch.tensor(v, device=dev) for k, v in inp.items()}
    leaves = {k: t[LEAF[k]].requires_grad_() for k in TERMS if LEAF[k] in t}
    kw = dict(d_xyz=t.get("d_xyz"), opacity=t.get("opacity"), motion_mask=t.get("mask"), scaling=t.get("scaling"),
              visible=t.get("visible"), depth_distortion=t.get("dd"), raw=raw, return_terms=True)
    if weights_tensor is not None:
        kw["weights"] = weights_tensor
    else:
        kw.update(w_mlp=weights["mlp"], w_oe=weights["oe"], w_scale=weights["scale"], w_dd=weights["dd"])
    loss, terms = reg.regularizers(**kw)
    (up * loss).backward()
    grads = {k: leaf.grad for k, leaf in leaves.items()}
    return loss.detach(), terms.means, terms.counts, grads


def check(lib, dev, key, inp, raw, up=1.0, what="f64", **kw):
    """fused against the float64 restatement (and torch's eager fp32 run for the gradient tolerance)"""
    means64, abs64, counts64, grads64 = reference64(key, inp, raw, up)
    _, _, _, grads32 = run_statements(inp, raw, WEIGHTS, up, torch.float32, dev)
    loss, means, counts, grads = fused(inp, raw, dev, up, **kw)
    means, counts = means.cpu().tolist(), counts.cpu().tolist()
    depth = depth_of(lib, inp)
    assert depth <= 13
    total64, total_bound = 0.0, 0.0
    for i, k in enumerate(TERMS):
        if k not in means64:
            assert means[i] == 0.0, (key, k)
            continue
        bound = (depth + 1) * EPS24 * abs64[k]
        err = abs(means[i] - means64[k])
        print("%s %s: value %.9g ref %.9g err %.3g bound %.3g" % (key, k, means[i], means64[k], err, bound))
        if bound > 0:
            _note("value err / bound " + what, err / bound)
        assert err <= bound, (key, k, means[i], means64[k], err, bound)
        total64 += WEIGHTS[k] * means64[k]
        total_bound += WEIGHTS[k] * bound
        g, g64 = grads[k].double().cpu(), grads64[k]
        assert g.shape == g64.shape and bool(torch.isfinite(g).all()), (key, k)
        gmax = float(g64.abs().max())
        e_torch = float((grads32[k].double().cpu() - g64).abs().max())
        e_fused = float((g - g64).abs().max())
        tol = max(2.0 * e_torch, 4.0 * EPS24 * gmax)
        print("%s %s: grad max %.3g fused err %.3g eager err %.3g tol %.3g" % (key, k, gmax, e_fused, e_torch, tol))
        if gmax > 0:
            _note("grad err / max|g| fused " + k, e_fused / gmax)
            _note("grad err / max|g| eager " + k, e_torch / gmax)
        assert e_fused <= tol, (key, k, e_fused, e_torch, gmax)
        if abs64[k] == 0.0 and k in ("oe", "scale"):          # an empty selection: exactly 0, no NaN
            assert means[i] == 0.0 and not bool(g.any()), (key, k)
    if "opacity" in inp:
        assert counts[0] == counts64[0], key
    if "scaling" in inp:
        assert counts[1] == counts64[1], key
    # the weighted total: the terms' bounds and its own rounding
    assert abs(float(loss) - total64) <= total_bound + EPS24 * abs(total64), (key, float(loss), total64)
    return loss, grads


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 70_001])
def test_all_four_terms_match_the_float64_statements(P, pattern, gpu, lib):
    for cols, raw in itertools.product((3, 1), (True, False)):
        inp = make_inputs(P, pattern, cols, raw)
        check(lib, gpu, (P, pattern, cols, raw), inp, raw, up=0.37 if cols == 1 else 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [65, 257])
def test_every_subset_of_one_and_three_terms(P, gpu, lib):
    for n in (1, 3):
        for present in itertools.combinations(TERMS, n):
            for cols, raw in ((3, True), (1, False)):
                inp = subset(make_inputs(P, "mixed_bool", cols, raw), present)
                check(lib, gpu, (P, "mixed_bool", cols, raw, present), inp, raw, what="subsets")


@pytest.mark.gpu
def test_drop_ins_are_the_single_terms(gpu):
    from gftorf_amd import reg
    inp = make_inputs(257, "mixed_bool", 3, True)
    t = {k: torch.tensor(v, device=gpu) for k, v in inp.items()}
    one = dict(mlp=1.0, oe=1.0, scale=1.0, dd=1.0)
    for k, f in (("mlp", lambda: reg.motion_reg(t["d_xyz"])), ("dd", lambda: reg.dd_loss(t["dd"])),
                 ("oe", lambda: reg.opacity_entropy(t["opacity"], t["mask"], raw=True)),
                 ("scale", lambda: reg.scale_loss(t["scaling"], t["visible"], raw=True))):
        loss, means, _, _ = fused(subset(inp, (k,)), True, gpu, weights=one)
        assert torch.equal(f(), loss) and float(loss) == float(means[TERMS.index(k)]), k


@pytest.mark.gpu
def test_extreme_raw_opacities_stay_finite(gpu, lib):
    """raw opacities of -120, -20, 0, 20 and 120 among ordinary ones: sigmoid saturates to exactly 0 and 1 in fp32, the
    entropy and its gradient stay finite (the reference's 1e-10 inside the logarithms) and within the same tolerances"""
    for pattern in ("mixed_bool", "all_dynamic_radii"):
        inp = make_inputs(257, pattern, 3, True, extreme=True)
        _, grads = check(lib, gpu, (257, pattern, "extreme"), inp, True)
        g = grads["oe"].cpu()[:len(EXTREME_RAW), 0]
        assert bool(torch.isfinite(g).all()) and float(g[0]) == 0.0 and float(g[4]) == 0.0 and float(g[2]) == 0.0


@pytest.mark.gpu
def test_misaligned_view_of_d_xyz(gpu, lib):
    """d_xyz = base[1:]: contiguous, its data pointer 12 bytes past a 16-byte boundary"""
    inp = make_inputs(257, "mixed_bool", 3, True)
    base = torch.zeros((inp["d_xyz"].shape[0] + 1, 3), device=gpu)
    base[1:] = torch.tensor(inp["d_xyz"], device=gpu)
    base.requires_grad_()
    view = base[1:]
    assert view.is_contiguous() and base.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 12
    from gftorf_amd import reg
    loss = reg.regularizers(d_xyz=view, w_mlp=WEIGHTS["mlp"], depth_distortion=torch.tensor(inp["dd"], device=gpu), w_dd=WEIGHTS["dd"])
    loss.backward()
    ref_loss, _, _, ref = fused(subset(inp, ("mlp", "dd")), True, gpu)
    assert torch.equal(loss.detach(), ref_loss)
    assert torch.equal(base.grad[1:], ref["mlp"]) and not bool(base.grad[0].any())
    check(lib, gpu, (257, "mixed_bool", 3, True, ("mlp", "dd")), subset(inp, ("mlp", "dd")), True, what="subsets")


@pytest.mark.gpu
def test_agrees_with_eager_torch_on_the_device(gpu, lib):
    """the statements run eagerly in fp32 on the device, P = 70 001: the same two tolerances"""
    for cols, raw, pattern in ((3, True, "mixed_bool"), (1, False, "all_dynamic_radii")):
        inp = make_inputs(70_001, pattern, cols, raw)
        _, abs64, counts64, grads64 = reference64((70_001, pattern, cols, raw), inp, raw, 1.0)
        means32, _, counts32, grads32 = run_statements(inp, raw, WEIGHTS, 1.0, torch.float32, gpu)
        _, means, counts, grads = fused(inp, raw, gpu)
        depth = depth_of(lib, inp)
        assert counts.cpu().tolist() == list(counts32) == list(counts64)
        for i, k in enumerate(TERMS):
            bound = (depth + 1) * EPS24 * abs64[k]
            err = abs(float(means[i]) - means32[k])
            _note("value err / bound eager", err / bound)
            assert err <= bound, (k, float(means[i]), means32[k], bound)
            e_torch = float((grads32[k].double().cpu() - grads64[k]).abs().max())
            tol = max(2.0 * e_torch, 4.0 * EPS24 * float(grads64[k].abs().max()))
            e = float((grads[k] - grads32[k]).abs().max())
            assert e <= tol, (k, e, tol)


@pytest.mark.gpu
def test_weights_tensor_computes_every_term_and_zero_weights_give_zero_gradients(gpu, lib):
    inp = make_inputs(257, "mixed_bool", 3, True)
    wt = torch.tensor([WEIGHTS[k] for k in TERMS], device=gpu)
    a = fused(inp, True, gpu)
    b = fused(inp, True, gpu, weights_tensor=wt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[3][k], b[3][k]) for k in TERMS)
    wt[1] = 0.0
    wt[3] = 0.0
    c = fused(inp, True, gpu, weights_tensor=wt)
    assert torch.equal(c[1], a[1]) and torch.equal(c[2], a[2])          # the means and counts are still computed
    assert not bool(c[3]["oe"].any()) and not bool(c[3]["dd"].any())
    assert torch.equal(c[3]["mlp"], a[3]["mlp"]) and torch.equal(c[3]["scale"], a[3]["scale"])
    d = fused(subset(inp, ("mlp", "scale")), True, gpu)
    assert abs(float(c[0]) - float(d[0])) <= 2 * 14 * EPS24 * abs(float(d[0]))      # (another workgroup layout)


@pytest.mark.gpu
def test_bit_reproducible(gpu):
    inp = make_inputs(70_001, "mixed_bool", 3, True)
    a = fused(inp, True, gpu, up=0.5)
    b = fused(inp, True, gpu, up=0.5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(a[3][k], b[3][k]) for k in TERMS)


def _static(inp, dev):
    t = {k: torch.tensor(v, device=dev) for k, v in inp.items()}
    for k in TERMS:
        t[LEAF[k]].requires_grad_()
    return t


def _step(t, wt):
    from gftorf_amd import reg
    loss, terms = reg.regularizers(d_xyz=t["d_xyz"], opacity=t["opacity"], motion_mask=t["mask"], scaling=t["scaling"],
                                   visible=t["visible"], depth_distortion=t["dd"], raw=True, weights=wt, return_terms=True)
    (0.5 * loss).backward()
    return torch.cat([loss.detach().reshape(1), terms.means, terms.counts.float()])


@pytest.mark.gpu
def test_no_host_sync(gpu):
    t = _static(make_inputs(70_001, "all_dynamic_radii", 3, True), gpu)
    wt = torch.tensor([WEIGHTS[k] for k in TERMS], device=gpu)
    _step(t, wt)                                # warm-up: the library's first load is not the question
    from gftorf_amd import reg
    reg.regularizers(d_xyz=t["d_xyz"], w_mlp=0.1, opacity=t["opacity"], motion_mask=t["mask"], w_oe=0.2, raw=True).backward()
    torch.cuda.synchronize()
    for k in TERMS:
        t[LEAF[k]].grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        _step(t, wt)
        reg.regularizers(d_xyz=t["d_xyz"], w_mlp=0.1, opacity=t["opacity"], motion_mask=t["mask"], w_oe=0.2, scaling=t["scaling"],
                         visible=t["visible"], w_scale=0.0, raw=True).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert all(t[LEAF[k]].grad is not None for k in TERMS)


@pytest.mark.gpu
def test_captured_step_follows_masks_radii_opacities_and_weights(gpu):
    """regularizers + backward captured on static tensors, all four terms, the weights a device tensor.  Between replays the
    radii, the mask, the raw opacities and the weights are rewritten in place (one weight becomes 0): every replay, the
    second and later ones included, equals an eager call on the same contents bit for bit.  Nothing in the path issues a
    memset: every buffer is written in full by a kernel."""
    P = 4099
    first = make_inputs(P, "all_dynamic_radii", 3, True)
    t = _static(first, gpu)
    wt = torch.tensor([WEIGHTS[k] for k in TERMS], device=gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            for k in TERMS:
                t[LEAF[k]].grad = None
            _step(t, wt)
    torch.cuda.current_stream().wait_stream(side)
    for k in TERMS:
        t[LEAF[k]].grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _step(t, wt)
    rng = np.random.default_rng(5)
    contents = [None]                # the first replay: the captured contents
    for seed, zero in ((1, 1), (2, 3), (3, None), (4, 2)):
        new = make_inputs(P, "all_dynamic_radii", 3, True, seed=seed)
        w = [WEIGHTS[k] * (1.0 + 0.25 * seed) for k in TERMS]
        if zero is not None:
            w[zero] = 0.0
        mask = rng.random(P) < (0.0 if seed == 3 else 0.3)              # (seed 3: no dynamic row at all)
        contents.append(dict(visible=new["visible"], mask=mask, opacity=new["opacity"], w=w))
    for c in contents:
        if c is not None:
            with torch.no_grad():
                t["visible"].copy_(torch.tensor(c["visible"], device=gpu))
                t["mask"].copy_(torch.tensor(c["mask"], device=gpu))
                t["opacity"].copy_(torch.tensor(c["opacity"], device=gpu))
                wt.copy_(torch.tensor(c["w"], device=gpu))
        graph.replay()
        torch.cuda.synchronize()
        e = {k: v.detach().clone() for k, v in t.items()}
        for k in TERMS:
            e[LEAF[k]].requires_grad_()
        eager = _step(e, wt.clone())
        assert torch.equal(out, eager), c and c["w"]
        for k in TERMS:
            assert torch.equal(t[LEAF[k]].grad, e[LEAF[k]].grad), (k, c and c["w"])
        if c is not None and 0.0 in c["w"]:
            assert not bool(t[LEAF[TERMS[c["w"].index(0.0)]]].grad.any())
        if c is not None and not c["mask"].any():          # no dynamic row: the term and its gradient are 0, not NaN
            assert float(out[2]) == 0.0 and int(out[5]) == 0 and not bool(t["opacity"].grad.any())
        assert float(out[0]) > 0 and bool(torch.isfinite(out).all())


@pytest.mark.gpu
def test_with_the_rasterizer(gpu):
    """A torf-shaped step at 64x48: the model's raw tensors, offsets on the dynamic rows, one render, an image loss plus the
    four regularisers fed with the rasterizer's own radii and depth_distortion, backward.  The gradients of _opacity,
    _scaling and the offsets equal those of the same step with the reference's eager statements, to the rasterizer's
    gradient tolerance (helpers.assert_close: the float atomics of its backward dominate)."""
    from gftorf_amd import GaussianRasterizer, reg
    P, W, H = 3000, 64, 48
    scene = Hh.small_scene(P=P, W=W, H=H, seed=21, scale_lo=0.01, scale_hi=0.08)
    g = scene["gaussians"]
    geo = {k: torch.tensor(g[k], dtype=torch.float32, device=gpu) for k in ("means3D", "opacities", "scales", "rotations", "shs", "shs_p")}
    rast = GaussianRasterizer(raster_settings=Hh.gpu_settings(scene, gpu))
    gen = torch.Generator().manual_seed(3)
    mask = (torch.rand(P, generator=gen) < 0.3).to(gpu)
    rows = torch.nonzero(mask)[:, 0]
    op = geo["opacities"].clamp(0.02, 0.98)
    start = dict(_opacity=torch.log(op / (1 - op)), _scaling=torch.log(geo["scales"]),
                 d_xyz=(0.01 * torch.randn((int(rows.shape[0]), 3), generator=gen)).to(gpu))
    target = torch.rand((3, H, W), generator=gen).to(gpu)
    m2 = torch.zeros((P, 3), device=gpu)
    lam = dict(mlp=0.05, oe=0.01, scale=5.0, dd=0.1)

    def step(use_fused):
        p = {k: v.clone().requires_grad_() for k, v in start.items()}
        means3D = geo["means3D"].index_add(0, rows, p["d_xyz"])
        get_opacity, get_scaling = torch.sigmoid(p["_opacity"]), torch.exp(p["_scaling"])
        outs = rast(means3D=means3D, means2D=m2, opacities=get_opacity, shs=geo["shs"], shs_p=geo["shs_p"], scales=get_scaling,
                    rotations=geo["rotations"], phase_offset=scene["phase_offset"], dc_offset=scene["dc_offset"])
        image, depth_distortion, radii = outs[0], outs[6], outs[10]
        loss = torch.abs(image - target).mean()
        if use_fused:
            loss = loss + reg.regularizers(d_xyz=p["d_xyz"], w_mlp=lam["mlp"], opacity=p["_opacity"], motion_mask=mask, w_oe=lam["oe"],
                                           scaling=p["_scaling"], visible=radii, w_scale=lam["scale"],
                                           depth_distortion=depth_distortion, w_dd=lam["dd"], raw=True)
        else:
            e = statements(dict(d_xyz=p["d_xyz"], opacity=get_opacity, mask=mask, scaling=get_scaling, visible=radii > 0,
                                dd=depth_distortion), raw=False)
            for k in TERMS:
                loss = loss + lam[k] * e[k].mean()
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {k: v.grad.detach().cpu().numpy() for k, v in p.items()}, int((radii > 0).sum())

    lf, gf, nvis = step(True)
    le, ge, _ = step(False)
    assert 0 < nvis < P and abs(lf - le) <= 1e-5 * abs(le), (lf, le, nvis)
    for k in ge:
        assert float(np.abs(ge[k]).max()) > 0, k
        Hh.assert_close(k, ge[k], gf[k])
