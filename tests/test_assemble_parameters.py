"""assemble_parameters and assemble_inputs (csrc/k_assemble.hip) against CPU restatements: float32 for what is copied or added
once (bit for bit), float64 for the activations (derived bounds).  The CPU tests pin the restatement itself and the host-side
argument checks; everything marked gpu runs the kernels.

The bounds (EPS = 2^-23, one fp32 ulp of 1):
  opacity, scales          |got - ref64| <= 4 EPS |ref64|       expf within 1 ulp, an add and a divide, the reference's rounding
  rotations                |got - ref64| <= 4 EPS per component  components <= 1; sqrt, divide, four products
  g(_opacity)              <= 1e-6 |ref64| + 2^-21 |g_up|        y (1 - y): the absolute error of y where y rounds towards 1
  g(_scaling)              <= 4 EPS |ref64|
  g(_rotation), g(d_rot)   per row, max norm: <= 16 EPS ||g_up||_2 / max(||r||_2, 1e-12)   (g - y (y.g)) / n cancels where g || y
Everything else is a copy or one IEEE add: equal to the float32 reference bit for bit.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import assemble_ref as R   # noqa: E402

EPS = 2.0 ** -23
BOTH = ("static", "dynamic")
REGIONS = [BOTH, ("static",), ("dynamic",), ()]
OUTS = ["means3D", "means2D", "opacity", "scales", "rotations", "shs", "shs_p"]
OFFSETS = ["d_xyz", "d_rot", "d_sh", "d_sh_p"]
PARTS = ["f_dc", "f_rest", "phase_dc", "phase_rest", "amp_dc", "amp_rest"]
# the two entry points' argument lists as keys of a case
ARGS = {"parameters": ["xyz", "ssp", "opacity", "scaling", "rotation_raw"] + PARTS + ["mask"] + OFFSETS,
        "inputs": ["xyz", "ssp", "opacity_act", "scaling_act", "rotation", "rotation_raw", "fc", "fp", "mask"] + OFFSETS}
# what goes through an activation (a tolerance against float64); everything else is bit-equal to the float32 reference
TOL_OUT = {"parameters": ("opacity", "scales", "rotations"), "inputs": ("rotations",)}
TOL_GRAD = {"parameters": ("opacity", "scaling", "rotation_raw", "d_rot"), "inputs": ("rotation_raw", "d_rot")}
SHAPES = [(1, 1), (4, 2), (9, 9), (16, 16), (9, 16), (16, 1)]
ROW_COUNTS = [1, 63, 64, 65, 1023, 1024, 1025, 4097, 70_001]
PATTERNS = ("none", "all", "alternate", "blocks", "first", "last", "edges", "random30")


def pattern_mask(P, pattern, seed=0):
    i = np.arange(P)
    if pattern == "none":
        return np.zeros(P, bool)
    if pattern == "all":
        return np.ones(P, bool)
    if pattern == "alternate":
        return i % 2 == 1
    if pattern == "blocks":                       # whole 1024-row blocks of the rank pass, all True / all False
        return (i // 1024) % 2 == 0
    if pattern == "first":
        return i == 0
    if pattern == "last":
        return i == P - 1
    if pattern == "edges":                        # the last lane of a wave and of a block, and their neighbours
        return np.isin(i, (63, 64, 1023, 1024))
    assert pattern == "random30"
    return np.random.default_rng(100 + seed).random(P) < 0.3


def make_case(P, M, M_p, mask, offsets="tensors", seed=0, visible_rank=False):
    """raw opacity ~ N(0, 2), raw scaling ~ N(-2, 1), the rest N(0, 1), offsets 0.1 N(0, 1); `up`: the seven upstream gradients.
    Both entry points run from one case: the keys of ARGS["inputs"] hold the activated tensors."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    nd = int(mask.sum())
    c = dict(xyz=f(P, 3), ssp=f(P, 3), opacity=2 * f(P, 1), scaling=f(P, 3) - 2, rotation_raw=f(P, 4), f_dc=f(P, 1, 3),
             f_rest=f(P, M - 1, 3), phase_dc=f(P, 1, 1), phase_rest=f(P, M_p - 1, 1), amp_dc=f(P, 1, 1), amp_rest=f(P, M_p - 1, 1),
             mask=mask)
    t = dict(d_xyz=0.1 * f(nd, 3), d_rot=0.1 * f(nd, 4), d_sh=0.1 * f(nd, M, 3), d_sh_p=0.1 * f(nd, M_p, 2))
    if visible_rank:                   # means3D[mask, 0] is then the rank of every dynamic row, exact in fp32 below 2^24
        c["xyz"][:, 0] = 0
        t["d_xyz"][:, 0] = np.arange(nd)
    scalar = dict(tensors=(), scalars=OFFSETS, mlp=("d_rot", "d_sh_p"))[offsets]
    c.update({k: (0.0 if k in scalar else v) for k, v in t.items()})
    c["up"] = [f(P, 3), f(P, 3), f(P, 1), f(P, 3), f(P, 4), f(P, M, 3), f(P, M_p, 2)]
    add_activated(c)
    return c


def add_activated(c):
    with np.errstate(over="ignore"):
        c["opacity_act"] = (1 / (1 + np.exp(-c["opacity"].astype(np.float64)))).astype(np.float32)
        c["scaling_act"] = np.exp(c["scaling"].astype(np.float64)).astype(np.float32)
    n = np.maximum(np.linalg.norm(c["rotation_raw"].astype(np.float64), axis=1, keepdims=True), 1e-12)
    c["rotation"] = (c["rotation_raw"] / n).astype(np.float32)
    c["fc"] = np.concatenate((c["f_dc"], c["f_rest"]), 1)
    c["fp"] = np.concatenate((np.concatenate((c["phase_dc"], c["phase_rest"]), 1), np.concatenate((c["amp_dc"], c["amp_rest"]), 1)), 2)


def entry_fn(entry, dev):
    if str(dev) == "cpu":
        return R.parameters_eager if entry == "parameters" else R.assemble_eager
    import gftorf_amd
    return gftorf_amd.assemble_parameters if entry == "parameters" else gftorf_amd.assemble_inputs


def leaves_of(entry, c):
    return [n for n in ARGS[entry] if n != "mask" and isinstance(c[n], np.ndarray)]


def run(entry, c, dev, dtype=torch.float32, regions=BOTH, need=None, use=range(7), keep=False):
    """Outputs and the gradients of every tensor argument (None where none arrives): `need` names the leaves that require
    grad (default all), `use` the outputs a gradient comes in through (the others' upstream gradient is None)."""
    args = []
    for n in ARGS[entry]:
        v = c[n]
        if n == "mask":
            args.append(torch.tensor(v, device=dev))
        elif isinstance(v, np.ndarray):
            args.append(torch.tensor(v, device=dev, dtype=dtype).requires_grad_(need is None or n in need))
        else:
            args.append(v)
    outs = entry_fn(entry, dev)(*args, render_regions=regions)
    grads = {n: None for n in leaves_of(entry, c)}
    sel = [i for i in use if outs[i].requires_grad]
    leaves = [(n, a) for n, a in zip(ARGS[entry], args) if torch.is_tensor(a) and a.requires_grad]
    ups = None
    if sel and leaves:
        ups = [torch.tensor(c["up"][i], device=dev, dtype=dtype) for i in sel]
        gs = torch.autograd.grad([outs[i] for i in sel], [a for _, a in leaves], ups, allow_unused=True)
        grads.update({n: g for (n, _), g in zip(leaves, gs)})
    res = [o.detach() for o in outs], grads
    return res + (args, ups) if keep else res


def references(entry, c, regions=BOTH, use=range(7)):
    return (run(entry, c, "cpu", torch.float32, regions, use=use), run(entry, c, "cpu", torch.float64, regions, use=use))


MEASURED = {}          # largest error per quantity relative to its bound (pytest -s)


def _note(key, err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(np.nanmax(r)) if r.size else 0.0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nassembly errors measured, as fractions of their bounds:", {k: "%.3g" % v for k, v in sorted(MEASURED.items())})


def _np(t):
    return t.detach().cpu().numpy()


def compare(entry, c, regions, got, refs, use=range(7), skip_rows=()):
    """The rules of the module's docstring.  `skip_rows`: Gaussians whose activations the caller checks against a table of
    its own (infinities and NaN have no error)."""
    (go, gg), ((o32, g32), (o64, g64)) = got, refs
    m = c["mask"]
    P = m.shape[0]
    on = np.where(m, "dynamic" in regions, "static" in regions)
    keep = np.ones(P, bool)
    keep[list(skip_rows)] = False
    up = [c["up"][i].astype(np.float64) if i in use else np.zeros(c["up"][i].shape) for i in range(7)]
    for i, n in enumerate(OUTS):
        a = _np(go[i])
        assert a.dtype == np.float32 and a.shape == tuple(o32[i].shape), n
        assert not a[~on].any(), n                                   # a region that is not rendered: exactly 0
        if n in TOL_OUT[entry]:
            r = _np(o64[i])
            err = np.abs(a.astype(np.float64) - r)
            bound = np.full(r.shape, 4 * EPS) if n == "rotations" else 4 * EPS * np.abs(r)
            _note("%s %s" % (entry, n), err[keep], bound[keep])
            assert (err <= bound)[keep].all(), (n, float(err[keep].max()))
        else:
            np.testing.assert_array_equal(a, _np(o32[i]), err_msg=n)
    # the vector each quaternion is normalised from, and the Gaussian of every offset row
    dyn_rows = np.nonzero(m)[0]
    r = c["rotation_raw"].astype(np.float64)
    if isinstance(c["d_rot"], np.ndarray):
        k = min(len(dyn_rows), c["d_rot"].shape[0])
        r[dyn_rows[:k]] += c["d_rot"][:k]
    else:
        r[m] += c["d_rot"]
    rot_bound = 16 * EPS * np.linalg.norm(up[4], axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-12)
    for n in leaves_of(entry, c):
        g = gg[n]
        if g32[n] is None:                                           # nothing flows in the reference: zero or None
            assert g is None or not bool(g.any()), n
            continue
        assert g is not None, n
        a, r32, r64 = _np(g), _np(g32[n]), _np(g64[n])
        assert a.dtype == np.float32 and a.shape == c[n].shape, n
        per_row = n not in OFFSETS
        rows = np.arange(P) if per_row else dyn_rows[:a.shape[0]]
        if per_row:
            assert not a[~on].any(), n
        elif "dynamic" not in regions:
            assert not a.any(), n
        if n not in TOL_GRAD[entry]:
            np.testing.assert_array_equal(a, r32, err_msg="g(%s)" % n)
            continue
        err = np.abs(a.astype(np.float64) - r64)
        if n == "opacity":
            bound = 1e-6 * np.abs(r64) + 2.0 ** -21 * np.abs(up[2])
        elif n == "scaling":
            bound = 4 * EPS * np.abs(r64)
        else:
            bound = np.broadcast_to(rot_bound[rows][:, None], err.shape)
            if entry == "inputs" and n == "rotation_raw":
                assert not a[~m].any()                               # the static rows' gradient goes to `rotation`
        k = keep[rows] if n in ("opacity", "scaling") else np.ones(len(rows), bool)
        _note("%s g(%s)" % (entry, n), err[k], bound[k])
        assert (err <= bound)[k].all(), ("g(%s)" % n, float(err[k].max()))


# ---- CPU: the restatement pinned, the wrapper's and the C entry points' argument checks -------------------------------

@pytest.mark.parametrize("regions", REGIONS)
@pytest.mark.parametrize("offsets", ["tensors", "scalars"])
@pytest.mark.parametrize("M,M_p", [(1, 1), (4, 2), (9, 16)])
def test_eager_restatement_equals_loops(M, M_p, offsets, regions):
    """parameters_eager in float64 against the numpy loops that index the parts where they lie: copies and single adds
    equal, the activations (another exp, another order of the sum of squares) to 1e-14 relative"""
    P = 257
    c = make_case(P, M, M_p, pattern_mask(P, "random30"), offsets, seed=3)
    got, _ = run("parameters", c, "cpu", torch.float64, regions)
    ref = R.parameters_loops(*[np.asarray(c[n], np.float64) if isinstance(c[n], np.ndarray) and n != "mask" else c[n]
                               for n in ARGS["parameters"]], render_regions=regions)
    for n, a, b in zip(OUTS, got, ref):
        a = _np(a)
        assert a.dtype == b.dtype == np.float64 and a.shape == b.shape, n
        if n in ("opacity", "scales", "rotations"):
            np.testing.assert_allclose(a, b, rtol=1e-14, atol=0, err_msg=n)
        else:
            np.testing.assert_array_equal(a, b, err_msg=n)
    if regions == BOTH:
        assert all(np.abs(_np(a)).min() > 0 for a in got[:5]) and np.abs(_np(got[5])).max() > 0


def test_wrapper_refuses_cpu_tensors_and_wrong_parts():
    from gftorf_amd import assemble_parameters
    P = 8
    c = make_case(P, 4, 2, pattern_mask(P, "alternate"))
    args = lambda c: [torch.tensor(c[n]) if isinstance(c[n], np.ndarray) else c[n] for n in ARGS["parameters"]]
    with pytest.raises(RuntimeError, match="HIP device only"):
        assemble_parameters(*args(c))
    shape_error = "the dc tensors hold one coefficient, phase and amplitude the same number"
    bad = dict(c, f_dc=np.zeros((P, 2, 3), np.float32))
    with pytest.raises(RuntimeError, match=shape_error):
        assemble_parameters(*args(bad))
    bad = dict(c, amp_rest=np.zeros((P, 2, 1), np.float32))
    with pytest.raises(RuntimeError, match=shape_error):
        assemble_parameters(*args(bad))


@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


def test_entry_points_refuse_misaligned_pointers(lib):
    """The pointers the kernels go through 16 bytes at a time are checked on the host before any launch: made-up addresses,
    never dereferenced."""
    from gftorf_amd import _lib
    ok, off = 4096, 4096 + 4

    def fwd_io(parts, **bad):
        io = _lib.AssembleIO()
        for n in ("xyz", "screenspace", "opacity", "scaling", "rotation", "rotation_raw", "motion_mask", "d_xyz", "d_rot", "d_sh", "d_sh_p",
                  "scratch", "out_means3D", "out_means2D", "out_opacity", "out_scales", "out_rotations", "out_shs", "out_shs_p"):
            setattr(io, n, ok)
        for n in (_lib.ASSEMBLE_PARTS if parts else ("feat_color", "feat_phasor")):
            setattr(io, n, ok)
        io.num_offset_rows = 3
        for n, v in bad.items():
            setattr(io, n, v)
        return io

    def bwd_io(parts, **bad):
        io = _lib.AssembleBwdIO()
        for n in _lib.ASSEMBLE_BWD_HEAD + _lib.ASSEMBLE_BWD_TAIL:
            setattr(io, n, ok)
        io.g_feat_color = io.g_feat_phasor = None
        for n in (_lib.ASSEMBLE_BWD_RAW[2:] if parts else ("g_feat_color", "g_feat_phasor")):
            setattr(io, n, ok)
        for n, v in bad.items():
            setattr(io, n, v)
        return io

    def refused(call, io, name, M=4, M_p=2):
        assert call(None, 5, M, M_p, 1, 1, C.byref(io)) != 0, name
        assert ("%s is not 16-byte aligned" % name) in _lib.last_error(), (name, _lib.last_error())

    always_f, wide_f = ("rotation", "rotation_raw", "d_rot", "out_rotations"), ("feat_color", "d_sh", "out_shs", "feat_phasor", "d_sh_p", "out_shs_p")
    always_b = ("rotation_raw", "d_rot", "g_rotations", "g_rotation", "g_rotation_raw", "g_d_rot")
    wide_b = ("g_shs", "g_feat_color", "g_d_sh", "g_shs_p", "g_feat_phasor", "g_d_sh_p")
    for parts in (False, True):
        for n in always_f:
            refused(lib.gft_assemble_forward, fwd_io(parts, **{n: off}), n)
        for n in always_b:
            refused(lib.gft_assemble_backward, bwd_io(parts, **{n: off}), n)
    for n in wide_f:                    # rows of 12 and 4 floats, the features whole
        refused(lib.gft_assemble_forward, fwd_io(False, **{n: off}), n)
    for n in wide_b:
        refused(lib.gft_assemble_backward, bwd_io(False, **{n: off}), n)
    # a pointer that is only read or written float by float may lie anywhere: the check names the first misaligned one, so a
    # call with such a pointer and one bad quaternion pointer names the quaternion
    io = fwd_io(False, xyz=off, screenspace=off, opacity=off, scaling=off, d_xyz=off, out_means3D=off, out_scales=off, out_rotations=off)
    refused(lib.gft_assemble_forward, io, "out_rotations")
    io = fwd_io(True, d_sh=off, out_shs=off, d_sh_p=off, out_shs_p=off, feat_dc_color=off, amp_rest=off, d_rot=off)    # the parts: float by float
    refused(lib.gft_assemble_forward, io, "d_rot")
    io = fwd_io(False, feat_color=off, d_sh=off, out_shs=off, feat_phasor=off, d_sh_p=off, out_shs_p=off, rotation=off)
    refused(lib.gft_assemble_forward, io, "rotation", M=9, M_p=9)                                                     # 27 / 18 floats per row
    io = bwd_io(True, g_shs=off, g_d_sh=off, g_shs_p=off, g_d_sh_p=off, g_feat_rest_color=off, g_means3D=off, g_xyz=off, g_d_xyz=off, g_d_rot=off)
    refused(lib.gft_assemble_backward, io, "g_d_rot")
    io = bwd_io(False, g_shs=off, g_feat_color=off, g_d_sh=off, g_shs_p=off, g_feat_phasor=off, g_d_sh_p=off, g_rotations=off)
    refused(lib.gft_assemble_backward, io, "g_rotations", M=9, M_p=9)
    # no Gaussians: nothing is looked at
    assert lib.gft_assemble_forward(None, 0, 4, 2, 1, 1, C.byref(fwd_io(False, rotation=off))) == 0


# ---- GPU --------------------------------------------------------------------------------------------------------------

def check(entry, c, dev, regions=BOTH, use=range(7), skip_rows=()):
    got = run(entry, c, dev, regions=regions, use=use)
    compare(entry, c, regions, got, references(entry, c, regions, use), use, skip_rows)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("regions", REGIONS)
@pytest.mark.parametrize("offsets", ["tensors", "scalars", "mlp"])
@pytest.mark.parametrize("M,M_p", SHAPES)
def test_parameters_match_the_references(M, M_p, offsets, regions, gpu):
    """both instantiations of both split kernels for colour and phasor, the 16-byte pieces that straddle two source tensors
    ((4, 2)), empty `rest` tensors ((1, 1)) and M != M_p"""
    P = 1025
    c = make_case(P, M, M_p, pattern_mask(P, "random30"), offsets, seed=M * 100 + M_p)
    outs, grads = check("parameters", c, gpu, regions)
    if not regions:
        assert all(not bool(o.any()) for o in outs) and all(g is None or not bool(g.any()) for g in grads.values())


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("P", ROW_COUNTS)
def test_row_counts_and_mask_patterns(P, pattern, gpu):
    """the rank of every dynamic row across wave and block edges: d_xyz[k, 0] = k over xyz[:, 0] = 0 shows it in means3D"""
    mask = pattern_mask(P, pattern, seed=P)
    c = make_case(P, 4, 2, mask, seed=P, visible_rank=True)
    for regions in (BOTH, ("dynamic",)):
        outs, _ = check("parameters", c, gpu, regions)
        np.testing.assert_array_equal(_np(outs[0])[mask, 0], np.arange(int(mask.sum()), dtype=np.float32))


def num_dynamic(lib, out):
    """gft_assemble_num_dynamic over the scratch the forward left for its backward"""
    from gftorf_amd import _lib
    scratch = [t for t in out.grad_fn.saved_tensors if t.dtype == torch.uint8]
    assert len(scratch) == 1
    nd = C.c_int64(-1)
    with _lib.on_device(out.device):
        _lib.check(lib.gft_assemble_num_dynamic(_lib.raw_stream(out.device), out.shape[0], scratch[0].data_ptr(), C.byref(nd)))
    return nd.value


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["parameters", "inputs"])
def test_two_trips_of_the_rank_scan(entry, gpu, lib):
    """1026 block sums: the scan's second trip of 1024 starts from a carry of ~900 000"""
    P = 1024 * 1024 + 1024 + 5
    mask = np.arange(P) % 7 != 0
    mask[2 ** 20:] = np.random.default_rng(1).random(P - 2 ** 20) < 0.5
    c = make_case(P, 1, 1, mask, seed=2, visible_rank=True)
    nd = int(mask.sum())
    assert nd > 2 ** 20 * 6 // 7 and nd < 2 ** 24
    outs, grads, args, ups = run(entry, c, gpu, keep=True)
    assert num_dynamic(lib, entry_fn(entry, gpu)(*args)[0]) == nd
    np.testing.assert_array_equal(_np(outs[0])[mask, 0], np.arange(nd, dtype=np.float32))
    compare(entry, c, BOTH, (outs, grads), references(entry, c))


_ALL_LEAVES = {}


def all_leaves_run(entry, M, M_p, dev):
    """P = 257 with every leaf requiring grad, checked against the references once"""
    key = (entry, M, M_p)
    if key not in _ALL_LEAVES:
        P = 257
        c = make_case(P, M, M_p, pattern_mask(P, "random30"), seed=5)
        _ALL_LEAVES[key] = (c, check(entry, c, dev))
    return _ALL_LEAVES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("M,M_p", [(4, 2), (9, 9)])
@pytest.mark.parametrize("entry", ["parameters", "inputs"])
def test_frozen_leaves(entry, M, M_p, gpu):
    """every differentiable argument alone requiring grad, and alone frozen (15 for assemble_parameters: the 11 tensors of the
    model and the 4 offsets; 12 for assemble_inputs): a NULL destination in the kernels"""
    c, (outs, full) = all_leaves_run(entry, M, M_p, gpu)
    names = leaves_of(entry, c)
    assert len(names) == (15 if entry == "parameters" else 12)
    for n in names:
        for need in ({n}, set(names) - {n}):
            o, g = run(entry, c, gpu, need=need)
            assert all(torch.equal(a, b) for a, b in zip(o, outs)), (n, len(need))
            for k in names:
                if k in need:
                    assert g[k] is not None and torch.equal(g[k], full[k]), (n, len(need), k)
                else:
                    assert g[k] is None, (n, len(need), k)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(7))
@pytest.mark.parametrize("entry", ["parameters", "inputs"])
def test_unused_outputs(entry, i, gpu):
    """a gradient arrives through one output only: the other six are None (set_materialize_grads(False))"""
    P = 257
    c = make_case(P, 4, 2, pattern_mask(P, "random30"), seed=6)
    _, grads = check(entry, c, gpu, use=(i,))
    assert any(g is not None and bool(g.any()) for g in grads.values())


@pytest.mark.gpu
@pytest.mark.parametrize("P", [65, 4097])
@pytest.mark.parametrize("M,M_p", [(4, 2), (16, 16)])
def test_gather_kernel_at_short_rows(M, M_p, P, gpu):
    """the features' gradient handed on without a copy: the offsets' gradient is gathered by k_assemble_wide_gather, rows of
    3 and 1 (some of a row's four threads have no piece), 12 and 8 sixteen-byte pieces"""
    mask = pattern_mask(P, "random30", seed=M)
    c = make_case(P, M, M_p, mask, seed=8)
    outs, grads, args, ups = run("inputs", c, gpu, keep=True)
    m = torch.tensor(mask, device=gpu)
    assert torch.equal(grads["d_sh"], ups[5][m]) and torch.equal(grads["d_sh_p"], ups[6][m])
    assert grads["fc"].data_ptr() == ups[5].data_ptr() and grads["fp"].data_ptr() == ups[6].data_ptr()
    compare("inputs", c, BOTH, (outs, grads), references("inputs", c))


@pytest.mark.gpu
def test_extreme_raw_opacities_and_scalings(gpu):
    """sigmoid saturated to exactly 0 and 1, exp underflowed to 0 and overflowed to inf, and a zero quaternion"""
    P = 257
    mask = pattern_mask(P, "alternate")
    c = make_case(P, 4, 2, mask, seed=9)
    x_op = np.array([-120.0, -20.0, 0.0, 20.0, 120.0], np.float32)
    x_sc = np.array([-110.0, -87.0, 0.0, 88.0, 89.0], np.float32)
    c["opacity"][:5, 0] = x_op
    c["scaling"][:5] = x_sc[:, None]
    c["up"][3][:5] = np.array([[1.5, -2.0, 0.0]] * 5, np.float32)          # a zero among the upstream gradients: 0 inf
    c["up"][2][:5] = 1.25
    c["rotation_raw"][6] = 0                                               # a static row
    c["rotation_raw"][7] = 0                                               # a dynamic row: rank 3
    c["d_rot"][3] = 0
    add_activated(c)
    outs, grads = check("parameters", c, gpu, skip_rows=range(5))
    f32 = np.float32
    inf, nan = f32(np.inf), f32(np.nan)
    # the float64 values rounded to fp32
    sig = np.array([0.0, 1 / (1 + np.exp(20.0)), 0.5, 1.0, 1.0]).astype(f32)          # 1 / (1 + e^-20) rounds to 1
    ex = np.array([0.0, np.exp(-87.0), 1.0, np.exp(88.0), inf]).astype(f32)           # e^-110 < 2^-149, e^89 > fp32's largest
    assert sig[0] == 0 and sig[1] > 0 and ex[1] > 0 and np.isfinite(ex[3])
    op, sc = _np(outs[2])[:5, 0], _np(outs[3])[:5]
    saturated = np.array([True, False, True, True, True])
    np.testing.assert_array_equal(op[saturated], sig[saturated])
    assert abs(float(op[1]) - float(sig[1])) <= 4 * EPS * float(sig[1])
    over = np.array([True, False, True, False, True])
    np.testing.assert_array_equal(sc[over], np.repeat(ex[over, None], 3, 1))
    assert (np.abs(sc[~over].astype(np.float64) - ex[~over, None]) <= 4 * EPS * ex[~over, None]).all()
    g_op, g_sc = _np(grads["opacity"])[:5, 0], _np(grads["scaling"])[:5]
    assert np.isfinite(g_op).all()
    np.testing.assert_array_equal(g_op[[0, 3, 4]], f32(0))                            # y (1 - y) with y = 0 or 1
    np.testing.assert_array_equal(g_op[2], f32(1.25 * 0.25))
    assert abs(float(g_op[1]) - 1.25 * float(sig[1])) <= 1e-6 * 1.25 * float(sig[1]) + 2.0 ** -21 * 1.25
    # g exp(x) under fp32 rules, upstream (1.5, -2, 0)
    want = np.array([[0.0, -0.0, 0.0], [1.5 * ex[1], -2 * ex[1], 0.0], [1.5, -2.0, 0.0], [1.5 * ex[3], -2 * ex[3], 0.0], [inf, -inf, nan]])
    np.testing.assert_array_equal(g_sc[[0, 2, 4]], want[[0, 2, 4]].astype(f32))
    assert (np.abs(g_sc[[1, 3]].astype(np.float64) - want[[1, 3]]) <= 4 * EPS * np.abs(want[[1, 3]])).all()
    assert np.isinf(g_sc[3]).sum() == 0 and np.isinf(want[3]).sum() == 0              # 2 e^88 is still finite
    # the zero quaternions: v / max(|v|, 1e-12) = 0, its gradient g / 1e-12
    rot, g_rot, g_drot = _np(outs[4]), _np(grads["rotation_raw"]), _np(grads["d_rot"])
    assert not rot[6].any() and not rot[7].any()
    for got, row in ((g_rot[6], 6), (g_rot[7], 7), (g_drot[3], 7)):
        np.testing.assert_allclose(got, c["up"][4][row] * f32(1e12), rtol=2 * EPS, atol=0)


def short_offsets(c, rows):
    return dict(c, **{k: c[k][:rows] for k in OFFSETS})


def check_with_spare_rows(c, got):
    """offset tensors with more rows than the mask has Trues: the rows past the last dynamic Gaussian reach nothing, their
    gradient is zero; the rest against the references of the same case without those rows"""
    rows = int(c["mask"].sum())
    outs, grads = got
    assert all(not bool(grads[k][rows:].any()) for k in OFFSETS)
    trimmed = short_offsets(c, rows)
    compare("parameters", trimmed, BOTH, (outs, dict(grads, **{k: grads[k][:rows] for k in OFFSETS})), references("parameters", trimmed))


@pytest.mark.gpu
def test_rows_without_an_offset(gpu):
    """d_* one row short of what the mask selects: NaN in the four outputs an offset enters, zero gradients for that Gaussian,
    everybody else unchanged, every gradient finite; then no Gaussians at all, no dynamic ones, and a row too many"""
    P = 500
    mask = pattern_mask(P, "random30", seed=2)
    c = make_case(P, 4, 2, mask, seed=2)
    nd, last = int(mask.sum()), int(np.nonzero(mask)[0][-1])
    full_o, full_g = run("parameters", c, gpu)
    outs, grads = run("parameters", short_offsets(c, nd - 1), gpu)
    others = np.arange(P) != last
    for i, (o, f) in enumerate(zip(outs, full_o)):
        o, f = _np(o), _np(f)
        np.testing.assert_array_equal(o[others], f[others], err_msg=OUTS[i])
        if i in (0, 4, 5, 6):
            assert np.isnan(o[last]).all(), OUTS[i]
        else:
            np.testing.assert_array_equal(o[last], f[last], err_msg=OUTS[i])
    for n, g in grads.items():
        g, f = _np(g), _np(full_g[n])
        assert np.isfinite(g).all(), n
        if n in OFFSETS:
            np.testing.assert_array_equal(g, f[:nd - 1], err_msg=n)
        else:
            np.testing.assert_array_equal(g[others], f[others], err_msg=n)
            assert not g[last].any(), n
    # P = 0
    e = make_case(0, 4, 2, np.zeros(0, bool))
    outs, grads = run("parameters", e, gpu)
    assert [tuple(o.shape) for o in outs] == [(0, 3), (0, 3), (0, 1), (0, 3), (0, 4), (0, 4, 3), (0, 2, 2)]
    assert all(g is None or g.numel() == 0 for g in grads.values())
    # no dynamic row: d_* with 0 rows
    z = make_case(P, 4, 2, np.zeros(P, bool), seed=3)
    assert z["d_xyz"].shape == (0, 3)
    outs, grads = check("parameters", z, gpu)
    assert all(tuple(grads[k].shape) == z[k].shape for k in OFFSETS)
    # an offset row more than the mask selects reaches nothing: its gradient is zero
    more = make_case(P, 4, 2, mask, seed=2)
    fewer = mask.copy()
    fewer[last] = False
    more = dict(more, mask=fewer)
    outs, grads = run("parameters", more, gpu)
    assert grads["d_sh"].shape[0] == nd
    check_with_spare_rows(more, (outs, grads))


@pytest.mark.gpu
def test_other_dtypes_and_layouts(gpu):
    """float64 _xyz, fp16 d_xyz, a column slice as _scaling, a transposed-then-sliced features_rest: the results of the fp32
    contiguous copies, gradients in the leaves' dtypes and shapes"""
    from gftorf_amd import assemble_parameters
    P, M, M_p = 257, 4, 2
    mask = pattern_mask(P, "random30")
    c = make_case(P, M, M_p, mask, seed=10)
    c["d_xyz"] = c["d_xyz"].astype(np.float16).astype(np.float32)
    plain_o, plain_g, args, ups = run("parameters", c, gpu, keep=True)
    names = ARGS["parameters"]
    odd = {n: (a.detach().clone() if torch.is_tensor(a) else a) for n, a in zip(names, args)}
    odd["xyz"] = odd["xyz"].double()
    odd["d_xyz"] = odd["d_xyz"].half()
    wide = torch.zeros(P, 5, device=gpu)
    wide[:, 1:4] = odd["scaling"]
    wide.requires_grad_()
    rest_t = torch.zeros(M - 1 + 2, 3, P, device=gpu)
    rest_t[1:M] = odd["f_rest"].permute(1, 2, 0)
    rest_t.requires_grad_()
    leaves = {n: (t.requires_grad_() if torch.is_tensor(t) and t.is_floating_point() else t) for n, t in odd.items()}
    leaves["scaling"] = wide[:, 1:4]
    leaves["f_rest"] = rest_t.permute(2, 0, 1)[:, 1:M]
    assert not leaves["scaling"].is_contiguous() and not leaves["f_rest"].is_contiguous()
    outs = assemble_parameters(*[leaves[n] for n in names])
    assert all(torch.equal(a, b) for a, b in zip(outs, plain_o))
    order = [n for n in names if n not in ("mask", "scaling", "f_rest")]
    gs = torch.autograd.grad(list(outs), [leaves[n] for n in order] + [wide, rest_t], ups)
    for n, g in zip(order, gs):
        assert g.dtype == leaves[n].dtype and g.shape == leaves[n].shape, n
        assert torch.equal(g.float(), plain_g[n].half().float() if n == "d_xyz" else plain_g[n]), n
    g_wide, g_rest = gs[-2:]
    assert torch.equal(g_wide[:, 1:4], plain_g["scaling"]) and not bool(g_wide[:, 0].any()) and not bool(g_wide[:, 4].any())
    assert torch.equal(g_rest[1:M].permute(2, 0, 1), plain_g["f_rest"]) and not bool(g_rest[0].any()) and not bool(g_rest[M:].any())


@pytest.mark.gpu
def test_misaligned_views(gpu):
    """rotation_raw, features_dc / features_rest and d_rot as contiguous views 4 bytes past a 16-byte boundary: the wrapper
    copies them to aligned storage, the results are those of aligned tensors, the gradient arrives in the view's base"""
    from gftorf_amd import assemble_inputs, assemble_parameters
    P, M, M_p = 257, 4, 2
    c = make_case(P, M, M_p, pattern_mask(P, "random30"), seed=11)

    def shifted(t):
        """t's values in a view that starts one float into a buffer: (base, view)"""
        base = torch.zeros(1 + t.numel(), device=gpu)
        base[1:] = t.detach().reshape(-1)
        base.requires_grad_()
        view = base[1:].view(t.shape)
        assert view.is_contiguous() and base.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
        return base, view

    for entry, fn, odd in (("parameters", assemble_parameters, ("rotation_raw", "f_dc", "f_rest", "d_rot")),
                           ("inputs", assemble_inputs, ("rotation_raw", "rotation", "fc", "fp", "d_rot", "d_sh", "d_sh_p"))):
        plain_o, plain_g, args, ups = run(entry, c, gpu, keep=True)
        names = ARGS[entry]
        leaves = {n: (a.detach().clone().requires_grad_(a.is_floating_point()) if torch.is_tensor(a) else a) for n, a in zip(names, args)}
        bases = {}
        for n in odd:
            bases[n], leaves[n] = shifted(leaves[n])
        outs = fn(*[leaves[n] for n in names])
        assert all(torch.equal(a, b) for a, b in zip(outs, plain_o)), entry
        order = [n for n in names if n != "mask"]
        gs = torch.autograd.grad(list(outs), [bases.get(n, leaves[n]) for n in order], ups)
        for n, g in zip(order, gs):
            if n in bases:
                assert float(g[0]) == 0.0 and torch.equal(g[1:].view(plain_g[n].shape), plain_g[n]), (entry, n)
            else:
                assert torch.equal(g, plain_g[n]), (entry, n)
    # an upstream gradient off the boundary: copied, not handed on
    plain_o, plain_g, args, ups = run("inputs", c, gpu, keep=True)
    outs = assemble_inputs(*args)
    _, g_view = shifted(ups[5])
    g_view = g_view.detach()
    fc, d_sh = args[ARGS["inputs"].index("fc")], args[ARGS["inputs"].index("d_sh")]
    g_fc, g_dsh = torch.autograd.grad([outs[5]], [fc, d_sh], [g_view])
    assert g_fc.data_ptr() != g_view.data_ptr() and g_fc.data_ptr() % 16 == 0
    assert torch.equal(g_fc, ups[5]) and torch.equal(g_dsh, plain_g["d_sh"])


@pytest.mark.gpu
def test_captured_forward_and_backward(gpu):
    """assemble_parameters and its backward in one graph over static tensors.  Between replays the raw parameters and offsets,
    then the mask (permuted; then one True fewer, so that the last offset row belongs to nobody) are rewritten in place: every
    replay equals an eager call on the same contents bit for bit, and that eager call the CPU references."""
    from gftorf_amd import assemble_parameters
    P, M, M_p = 4097, 16, 16
    mask = pattern_mask(P, "random30")
    nd = int(mask.sum())
    c = make_case(P, M, M_p, mask, seed=12)
    names = ARGS["parameters"]
    grad_names = leaves_of("parameters", c)

    def fresh(c):
        return {n: (torch.tensor(c[n], device=gpu).requires_grad_(n != "mask")) for n in names}

    t = fresh(c)
    ups = [torch.tensor(u, device=gpu) for u in c["up"]]

    def step():
        outs = assemble_parameters(*[t[n] for n in names])
        torch.autograd.backward(list(outs), ups)
        return outs

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            for n in grad_names:
                t[n].grad = None
            step()
    torch.cuda.current_stream().wait_stream(side)
    for n in grad_names:
        t[n].grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    rng = np.random.default_rng(13)
    second = make_case(P, M, M_p, mask, seed=14)
    permuted = rng.permutation(mask)
    fewer = permuted.copy()
    fewer[np.nonzero(permuted)[0][5]] = False
    assert permuted.sum() == nd and fewer.sum() == nd - 1 and (permuted != mask).any()
    contents = dict(c)
    for update in ({n: second[n] for n in grad_names}, dict(mask=permuted), dict(mask=fewer)):
        contents.update(update)
        with torch.no_grad():
            for n, v in update.items():
                t[n].copy_(torch.tensor(v, device=gpu))
        graph.replay()
        torch.cuda.synchronize()
        got = ([o.detach() for o in outs], {n: t[n].grad for n in grad_names})
        eager = run("parameters", contents, gpu)
        assert all(torch.equal(a, b) for a, b in zip(got[0], eager[0]))
        for n in grad_names:
            assert torch.equal(got[1][n], eager[1][n]), n
        assert all(bool(torch.isfinite(x).all()) for x in list(got[0]) + list(got[1].values()))
        check_with_spare_rows(contents, eager)
    assert all(t[k].grad.shape[0] == nd and not bool(t[k].grad[nd - 1].any()) for k in OFFSETS)
