"""densify_and_prune as one plan and one pass over every tensor (gftorf_amd.densify.densify_and_prune_fused).
CPU: the per-row layout model (tests/densify_layout_ref.py) against the reference's eager statements, the float32 rounding of
the thresholds, the loud failure without a device, the header and the exported symbols.  GPU: the fused call against the
composite (gftorf_amd.densify.densify_and_prune) on twins, bit for bit -- no tolerance anywhere: data movement plus masks."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import densify_layout_ref as layout_ref
import loop_densify as L
from oracle import densify_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_GRAD, MIN_OPACITY, EXTENT = 0.0002, 0.005, 2.0
NEW_SYMBOLS = ("gft_densify_plan_scratch_bytes", "gft_densify_classify", "gft_densify_layout", "gft_rows_remap")


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,seed,max_screen_size", [(1, 1, 20), (63, 2, None), (1000, 3, 20), (20000, 5, 20), (3001, 5, None)])
def test_layout_model_reproduces_the_reference(P, seed, max_screen_size):
    """One index map (source_row, kind, child), applied to the input by plain indexing, is the reference's event: every
    parameter and moment is a row of the input, a zero row (moments of new rows) or a child's new scaling; the statistics
    are zero.  (The children's xyz rows hold torch.normal samples and are exempt.)"""
    a = densify_ref.EagerGaussians(P, "cpu", seed)
    before = a.snapshot()
    before = {k: v.clone() for k, v in before.items()}
    pl = layout_ref.plan(a, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size)
    want_rows = layout_ref.apply(before, pl)
    torch.manual_seed(11)
    a.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size)
    got = a.snapshot()
    assert set(got) == set(want_rows)
    not_child = torch.as_tensor(pl["kind"] != 2)
    for k in got:
        assert got[k].shape == want_rows[k].shape, k
        if k == "_xyz":
            assert torch.equal(got[k][not_child], want_rows[k][not_child]), k
        else:
            assert torch.equal(got[k], want_rows[k]), k
    cls, kind = pl["cls"], pl["kind"]
    n_clone, n_split = int((cls == 1).sum()), int((cls == 2).sum())
    clones_pruned, children_pruned = n_clone - int((kind == 1).sum()), 2 * n_split - int((kind == 2).sum())
    if (P, seed, max_screen_size) == (20000, 5, 20):
        assert n_clone > 0 and n_split > 0 and clones_pruned >= 1 and children_pruned >= 1
        assert (n_clone, n_split, clones_pruned, children_pruned) == (1232, 8985, 2, 164)
    if (P, seed, max_screen_size) == (63, 2, None):
        assert (n_clone, n_split, clones_pruned, children_pruned) == (2, 32, 0, 2)


def test_python_thresholds_meet_float32_tensors_as_float32():
    """torch rounds a Python number to the tensor's dtype before it compares: the kernels take the thresholds as float."""
    for x in (0.0002, 0.005, 0.01 * 2.0, 0.05 * 2.0, 0.001 * 2.0):
        x32 = float(np.float32(x))
        t = torch.tensor([x32])
        assert C.c_float(x).value == x32
        for nudged in (x32 + 1e-12, x32 - 1e-12, x):
            assert float(np.float32(nudged)) == x32                  # the nudge is below half an ulp
            assert bool((t >= nudged).all()) and bool((t <= nudged).all())
            assert not bool((t > nudged).any()) and not bool((t < nudged).any())
    # and a value that is not a float32 keeps comparing like its float32 neighbour, not like the double
    d = 0.1
    assert float(np.float32(d)) > d and bool((torch.tensor([np.float32(d)]) <= d).all())


def test_fused_fails_loudly_without_a_device():
    from gftorf_amd import densify
    a = densify_ref.EagerGaussians(8, "cpu", 1)
    with pytest.raises(RuntimeError, match="HIP device only"):
        densify.densify_and_prune_fused(a, MAX_GRAD, MIN_OPACITY, EXTENT)
    res = densify.DensifyResult(4, 4, source_row=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device only"):
        res.remap(torch.zeros(4, 3))


def test_header_is_c_and_the_library_exports_the_new_symbols(tmp_path):
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    lib = _lib.load()
    prog = tmp_path / "densify.c"
    prog.write_text('#include "gftorf_densify.h"\nint main(void){return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(prog)])
    header = open(os.path.join(ROOT, "include", "gftorf_densify.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and (name + "(") in header, name
    assert lib.gft_abi_version() == 16 == _lib.ABI_VERSION
    # the argument checks need no device
    assert lib.gft_densify_plan_scratch_bytes(0) == 64 * 4 and lib.gft_densify_plan_scratch_bytes(4097) == (2 * 2 + 64) * 4
    counts = (C.c_int64 * 2)(7, 7)
    assert lib.gft_densify_classify(None, 0, None, None, None, 1.0, 1.0, None, None, None, None, counts) == 0
    assert list(counts) == [0, 0]
    assert lib.gft_densify_layout(None, 0, 0, 0, 2, *([None] * 6), 0.0, 0, 0, 0.0, 0.0, None, 0, *([None] * 8), counts) == 0
    assert lib.gft_densify_layout(None, 1 << 30, 1 << 30, 1 << 30, 2, *([None] * 6), 0.0, 0, 0, 0.0, 0.0, None, 0, *([None] * 8),
                                  counts) != 0
    assert "2^31" in _lib.last_error()
    assert lib.gft_rows_remap(None, 0, None, None, 0, None, None, 12) == 0
    assert lib.gft_rows_remap(None, 5, None, None, 0, None, None, 6) != 0
    assert "multiple of 4" in _lib.last_error()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _fresh_statistics(models, rnd, dev):
    """Statistics for the next round (the event zeroed them), the same on every model."""
    g = torch.Generator().manual_seed(7 + rnd)
    n = models[0]._xyz.shape[0]
    acc, den = (torch.rand((n, 1), generator=g) * 0.03).to(dev), torch.randint(0, 60, (n, 1), generator=g).float().to(dev)
    rad = (torch.rand(n, generator=g) * 30).to(dev)
    for m in models:
        m.xyz_gradient_accum, m.denom, m.max_radii2D = acc.clone(), den.clone(), rad.clone()


def _check_counts(res, P_before, masks, N, P_after):
    clone, split, _ = masks
    assert (res.P_before, res.P) == (P_before, P_after)
    assert res.cloned == int(clone.sum()) and res.split == int(split.sum())
    assert res.P == P_before + res.cloned + N * res.split - res.split - res.pruned and res.pruned >= 0
    assert res.source_row.shape == res.kind.shape == res.child.shape == (P_after,)
    kind = res.kind.cpu()
    assert int((kind == 1).sum()) <= res.cloned and int((kind == 2).sum()) <= N * res.split


def _composite(densify, pc, max_grad, min_opacity, extent, max_screen_size, N):
    """densify.densify_and_prune's body with the split's N handed through (the composite fixes it at 2)."""
    grads = pc.xyz_gradient_accum / pc.denom
    grads[grads.isnan()] = 0.0
    densify.densify_and_clone(pc, grads, max_grad, extent)
    densify.densify_and_split(pc, grads, max_grad, extent, N=N)
    prune_mask = (pc.get_opacity < min_opacity).squeeze()
    if max_screen_size:
        big_points_vs = pc.max_radii2D > max_screen_size
        big_points_ws = pc.get_scaling.max(dim=1).values > 0.05 * extent
        small_points_ws = pc.get_scaling.max(dim=1).values < 0.001 * extent
        prune_mask = torch.logical_or(torch.logical_or(torch.logical_or(prune_mask, big_points_vs), big_points_ws), small_points_ws)
    densify.prune_points(pc, prune_mask)


@pytest.mark.gpu
@pytest.mark.parametrize("max_screen_size", [20, None])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 4095, 4096, 4097, 20000, 100003])
def test_fused_matches_the_composite(P, max_screen_size):
    """Twins under the same torch generator state, two rounds with fresh statistics between them: every parameter, moment,
    step and statistic equal.  At one size a third twin runs the reference's own statements."""
    from gftorf_amd import densify
    dev = torch.device("cuda:0")
    a = densify_ref.EagerGaussians(P, dev, seed=5)             # densify_and_prune_fused
    b = densify_ref.EagerGaussians(P, dev, seed=5)             # densify.densify_and_prune
    c = densify_ref.EagerGaussians(P, dev, seed=5) if P == 4097 else None          # its own (the reference's) statements
    th = dict(max_grad=MAX_GRAD, extent=EXTENT, min_opacity=MIN_OPACITY)
    for rnd in range(2):
        n_before = b._xyz.shape[0]
        masks = L.selections(b, th)
        torch.manual_seed(100 + rnd)
        res = densify.densify_and_prune_fused(a, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size)
        torch.manual_seed(100 + rnd)
        densify.densify_and_prune(b, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size)
        L.assert_same_snapshot(a, b, (P, rnd))
        if c is not None:
            torch.manual_seed(100 + rnd)
            c.densify_and_prune(MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size)
            L.assert_same_snapshot(a, c, (P, rnd, "reference"))
        assert [g["name"] for g in a.optimizer.param_groups] == [g["name"] for g in b.optimizer.param_groups]
        assert a.optimizer.param_groups[0]["params"][0] is a._xyz
        assert len(a.optimizer.state) == len(b.optimizer.state)
        _check_counts(res, n_before, masks, 2, b._xyz.shape[0])
        _fresh_statistics([m for m in (a, b, c) if m is not None], rnd, dev)
    if P >= 4095:
        assert a._xyz.shape[0] != P


def _make_isotropic(m):
    """One scaling column (GaussianModel with isotropic=True), moments included."""
    grp = next(g for g in m.optimizer.param_groups if g["name"] == "scaling")
    old = grp["params"][0]
    st = m.optimizer.state.pop(old)
    new = torch.nn.Parameter(old.detach()[:, :1].contiguous().requires_grad_(True))
    st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][:, :1].contiguous(), st["exp_avg_sq"][:, :1].contiguous()
    grp["params"][0] = new
    m.optimizer.state[new] = st
    m._scaling, m.isotropic = new, True


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nothing_selected", "all_pruned", "no_size_rule", "denom_zero", "isotropic", "three_children"])
def test_degenerate_plans(case):
    from gftorf_amd import densify
    dev = torch.device("cuda:0")
    P = 4097
    a, b = densify_ref.EagerGaussians(P, dev, seed=9), densify_ref.EagerGaussians(P, dev, seed=9)
    max_grad, min_opacity, max_screen_size, N = MAX_GRAD, MIN_OPACITY, 20, 2
    if case == "nothing_selected":
        max_grad = 1e9
        for m in (a, b):
            m.denom.clamp_(min=1.0)                           # (a zero would make the mean gradient inf, which IS selected)
    if case == "all_pruned":
        min_opacity = 1.1
    if case == "no_size_rule":
        max_screen_size = None
    if case == "denom_zero":
        for m in (a, b):
            m.denom.zero_()
            m.xyz_gradient_accum[::3] = 0.0                   # 0 / 0: NaN -> 0; the others are inf and stay
    if case == "isotropic":
        _make_isotropic(a)
        _make_isotropic(b)
    if case == "three_children":
        N = 3
    th = dict(max_grad=max_grad, extent=EXTENT, min_opacity=min_opacity)
    masks = L.selections(b, th)
    torch.manual_seed(3)
    res = densify.densify_and_prune_fused(a, max_grad, min_opacity, EXTENT, max_screen_size, N=N)
    torch.manual_seed(3)
    _composite(densify, b, max_grad, min_opacity, EXTENT, max_screen_size, N)
    L.assert_same_snapshot(a, b, case)
    _check_counts(res, P, masks, N, b._xyz.shape[0])
    if case == "nothing_selected":
        assert res.cloned == res.split == 0 and int(res.kind.max()) == 0
    if case == "all_pruned":
        assert res.P == 0 and a._xyz.shape == (0, 3) and res.cloned > 0 and res.split > 0
    if case == "denom_zero":
        assert res.cloned + res.split == P - len(range(0, P, 3))
    if case == "isotropic":
        assert a._scaling.shape[1] == 1 and res.split > 0
    if case == "three_children":
        assert int((res.kind == 2).sum()) > 2 * res.split
    for grp in a.optimizer.param_groups:                       # the optimizer is still usable
        grp["params"][0].grad = torch.zeros_like(grp["params"][0])
    a.optimizer.step()


def _remap_call(n_out, row_map, src, extra, dst, row_bytes, src_rows=None):
    from gftorf_amd import _lib
    lib = _lib.load()
    dev = dst.device
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with _lib.on_device(dev):
        return lib.gft_rows_remap(_lib.raw_stream(dev), n_out, ptr(row_map), ptr(src), src.shape[0] if src_rows is None else src_rows,
                                  ptr(extra), ptr(dst), row_bytes)


def _remap_want(row_map, src, extra):
    """Indexing on the host."""
    rows = src.shape[0]
    both = torch.cat((src, extra, torch.zeros((1, src.shape[1]), dtype=src.dtype)))
    return both[torch.where(row_map < 0, torch.full_like(row_map, rows + extra.shape[0]), row_map).long()]


@pytest.mark.gpu
@pytest.mark.parametrize("row_bytes", [4, 12, 16, 60, 180, 192])
def test_rows_remap_against_host_indexing(row_bytes):
    """gft_rows_remap alone: rows of the source (repeated ones too), rows of `extra`, zero rows, in any order; the 16-byte
    and the 4-byte pieces; pointers off 16-byte alignment take the 4-byte pieces."""
    from gftorf_amd import _lib
    dev = torch.device("cuda:0")
    cols = row_bytes // 4
    g = torch.Generator().manual_seed(row_bytes)
    src_rows, extra_rows = 1000, 37
    src = torch.randint(-2**31, 2**31 - 1, (src_rows, cols), generator=g, dtype=torch.int32)
    extra = torch.randint(-2**31, 2**31 - 1, (extra_rows, cols), generator=g, dtype=torch.int32)
    src_d, extra_d = src.to(dev), extra.to(dev)
    for n_out in (0, 1, 65, 70001):
        row_map = torch.randint(-1, src_rows + extra_rows, (n_out,), generator=g, dtype=torch.int32)
        if n_out >= 65:
            row_map[:4] = torch.tensor([-1, src_rows - 1, src_rows, src_rows + extra_rows - 1], dtype=torch.int32)
            row_map[10:20] = 5                                                      # one source row ten times
        dst = torch.full((n_out, cols), 0x55555555, device=dev, dtype=torch.int32)
        _lib.check(_remap_call(n_out, row_map.to(dev), src_d, extra_d, dst, row_bytes))
        assert torch.equal(dst.cpu(), _remap_want(row_map, src, extra)), n_out
    # no extra rows given: a map entry past the source is a zero row; no source rows: everything comes from extra
    row_map = torch.tensor([0, src_rows, -1, 3], dtype=torch.int32)
    dst = torch.full((4, cols), 0x55555555, device=dev, dtype=torch.int32)
    _lib.check(_remap_call(4, row_map.to(dev), src_d, None, dst, row_bytes))
    assert torch.equal(dst.cpu(), torch.stack((src[0], torch.zeros_like(src[0]), torch.zeros_like(src[0]), src[3])))
    row_map = torch.tensor([2, -1, 0], dtype=torch.int32)
    dst = torch.full((3, cols), 0x55555555, device=dev, dtype=torch.int32)
    _lib.check(_remap_call(3, row_map.to(dev), None, extra_d, dst, row_bytes, src_rows=0))
    assert torch.equal(dst.cpu(), torch.stack((extra[2], torch.zeros_like(extra[2]), extra[0])))
    # every pointer in turn 4 bytes off a 16-byte boundary: the same result through the 4-byte pieces
    n_out = 4099
    row_map = torch.randint(-1, src_rows + extra_rows, (n_out,), generator=g, dtype=torch.int32)
    want = _remap_want(row_map, src, extra)
    off = lambda t: torch.cat((t.new_zeros(1), t.reshape(-1)))[1:].view(t.shape)
    for which in range(3):
        s, e = (off(src_d) if which == 0 else src_d), (off(extra_d) if which == 1 else extra_d)
        dst = off(torch.zeros((n_out, cols), device=dev, dtype=torch.int32)) if which == 2 else torch.zeros((n_out, cols), device=dev,
                                                                                                            dtype=torch.int32)
        assert [s, e, dst][which].data_ptr() % 16 == 4
        _lib.check(_remap_call(n_out, row_map.to(dev), s, e, dst, row_bytes))
        assert torch.equal(dst.cpu(), want), which


@pytest.mark.gpu
def test_rows_remap_refuses_rows_that_are_no_multiple_of_4_bytes():
    from gftorf_amd import _lib, densify
    dev = torch.device("cuda:0")
    row_map = torch.zeros(3, device=dev, dtype=torch.int32)
    src = torch.zeros((4, 6), device=dev, dtype=torch.uint8)
    assert _remap_call(3, row_map, src, None, torch.zeros((3, 6), device=dev, dtype=torch.uint8), 6) != 0
    assert "multiple of 4" in _lib.last_error()
    res = densify.DensifyResult(4, 3, source_row=row_map, map_state=row_map)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        res.remap(src, "parent")
    with pytest.raises(RuntimeError, match="4 rows"):
        res.remap(torch.zeros((5, 4), device=dev))
    with pytest.raises(ValueError, match="new_rows"):
        res.remap(torch.zeros((4, 4), device=dev), "copy")


@pytest.mark.gpu
@pytest.mark.parametrize("optimizer", ["torch", "fused", "capturable"])
def test_optimizer_continuity(optimizer):
    """One step() after a fused event, under a changed xyz rate, equals the composite-driven twin's step."""
    from gftorf_amd import FusedAdam, densify
    dev = torch.device("cuda:0")
    cls = {"torch": torch.optim.Adam, "fused": FusedAdam, "capturable": functools.partial(FusedAdam, capturable=True)}[optimizer]
    P = 4097
    a, b = densify_ref.EagerGaussians(P, dev, 5, optimizer_cls=cls), densify_ref.EagerGaussians(P, dev, 5, optimizer_cls=cls)
    L.assert_same_snapshot(a, b, "start")
    torch.manual_seed(21)
    res = densify.densify_and_prune_fused(a, MAX_GRAD, MIN_OPACITY, EXTENT)
    torch.manual_seed(21)
    densify.densify_and_prune(b, MAX_GRAD, MIN_OPACITY, EXTENT)
    assert res.cloned > 0 and res.split > 0 and res.P != P
    L.assert_same_snapshot(a, b, "event")
    moved_from = a._xyz.detach().clone()
    g = torch.Generator().manual_seed(4)
    grads = {grp["name"]: (torch.randn(grp["params"][0].shape, generator=g) * 1e-3).to(dev) for grp in a.optimizer.param_groups}
    for m in (a, b):
        for grp in m.optimizer.param_groups:
            grp["params"][0].grad = grads[grp["name"]].clone()
            if grp["name"] == "xyz":
                grp["lr"] = 3.7e-4
        if hasattr(m.optimizer, "refresh_lr"):
            m.optimizer.refresh_lr()
        m.optimizer.step()
    L.assert_same_snapshot(a, b, "step")
    assert float(a.optimizer.state[a._xyz]["step"]) == 2.0
    assert not torch.equal(a._xyz.detach(), moved_from)           # (the step moved something)


@pytest.mark.gpu
def test_motion_mask_and_side_tensors_stay_in_step():
    from gftorf_amd import densify
    from gftorf_amd.query import DeformQuery
    dev = torch.device("cuda:0")
    P = 20000
    a = L.DynamicGaussians(P, dev, seed=5)
    g = torch.Generator().manual_seed(2)
    seg = 0.5 + 0.01 * torch.randn((P, 3), generator=g)
    seg[::7, 0] = 0.5                                            # exactly on the threshold: static
    with torch.no_grad():
        a._features_seg_color.copy_(seg.to(dev))
    side = torch.randn((P, 5), generator=g).to(dev)             # a caller's own per-Gaussian tensors
    ids = torch.arange(P, dtype=torch.int32, device=dev)
    torch.manual_seed(8)
    res = densify.densify_and_prune_fused(a, MAX_GRAD, MIN_OPACITY, EXTENT)
    assert res.cloned > 0 and res.split > 0 and res.pruned > 0
    mask = a.get_motion_mask
    assert res.motion_mask.dtype == torch.bool and torch.equal(res.motion_mask, mask) and 0 < int(mask.sum()) < res.P
    q, fresh = res.deform_query(), DeformQuery(mask.contiguous())
    assert (q.n, q.P) == (fresh.n, fresh.P) == (int(mask.sum()), res.P)
    assert torch.equal(q.rank, fresh.rank) and torch.equal(q.count, fresh.count)
    for got, want in zip(q.inputs(a._xyz, EXTENT, [0.3]), fresh.inputs(a._xyz, EXTENT, [0.3])):
        assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(q.refresh().rank, fresh.rank)
    src, kind = res.source_row.cpu().long(), res.kind.cpu()
    assert torch.equal(res.remap(ids, "parent").cpu().long(), src)
    for t in (side, ids):
        want = t.cpu()[src]
        assert torch.equal(res.remap(t, "parent").cpu(), want)
        want[kind != 0] = 0
        assert torch.equal(res.remap(t, "zero").cpu(), want)
    # the kinds in their virtual order: originals, clones, children; sources increasing inside the first two
    k = kind.long()
    assert bool((k[1:] >= k[:-1]).all())
    for kd in (0, 1):
        s = src[kind == kd]
        assert bool((s[1:] > s[:-1]).all())
    child = res.child.cpu().long()
    assert bool((child[kind != 2] == -1).all()) and bool((child[kind == 2][1:] > child[kind == 2][:-1]).all())
