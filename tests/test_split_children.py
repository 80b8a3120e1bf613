"""The children of a densification event's split rows in one kernel (gft_split_children, gftorf_amd.densify.split_children,
the ``children="kernel"`` route of densify_and_prune_fused and densify_and_split).

The route has a contract of its own (include/gftorf_densify.h): the children's scaling and largest scaling are the torch
statements' bit for bit (they are left to torch: on the device this library's logf did not give torch.log's bits); their
positions are the rotation of the same samples by the same R, the three products summed as an ascending chain of fused
multiply-adds, held against float64 from the same float32 inputs to

    |got - exact| <= 16 eps (|s_0| + |s_1| + |s_2|) + 2 eps |exact|,    eps = 2^-23

(tests/split_children_ref.py derives it).  The reference's own route (torch.bmm) is checked against the same bound wherever
the kernel is, so a bound that is wrong shows as such.  Nothing asserts equality with torch.bmm.

CPU: the numpy restatement against the torch statements, the exported symbol, the argument errors, the keyword.  GPU: the
kernel against the torch statements and the restatement, the generator's consumption, twins through the fused event and the
composite, one optimizer step after the event."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import loop_densify as L
import split_children_ref as ref
from oracle import densify_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_GRAD, MIN_OPACITY, EXTENT = 0.0002, 0.005, 2.0
EPS = ref.EPS


def _ulps(a, b):
    """Distance in units of the last place between two float32 arrays of one sign pattern."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _torch_children(densify, xyz, rotation, scaling, z, N, scaling_cols=3):
    """densify_and_split's statements (scene/gaussian_model.py:577-585) on gathered rows, torch.normal replaced by what it
    does after its normal_(0, 1) so that the normals can be given: (new_xyz, new_scaling, child_max_scaling, R)."""
    stds = scaling.repeat(N, 1)
    samples = z.mul(stds).add(torch.zeros_like(z))
    R = densify._rotation_matrices(rotation)
    new_xyz = torch.bmm(R.repeat(N, 1, 1), samples.unsqueeze(-1)).squeeze(-1) + xyz.repeat(N, 1)
    new_scaling = torch.log(scaling[:, :scaling_cols].repeat(N, 1) / (0.8 * N))
    return new_xyz, new_scaling, torch.exp(new_scaling).max(dim=1).values, R


def _rows_inputs(S, seed):
    """Split rows' values that exercise the arithmetic: unnormalised quaternions of norm 1e-2 .. 10 with negative w among
    them, scalings around 0.02, one zero quaternion, one scaling of 1e-30 (S >= 3)."""
    g = torch.Generator().manual_seed(seed)
    rotation = torch.randn((S, 4), generator=g)
    rotation = rotation / rotation.norm(dim=1, keepdim=True).clamp_min(1e-6) * torch.pow(10.0, torch.rand((S, 1), generator=g) * 3 - 2)
    rotation[::2, 0] = -rotation[::2, 0].abs()
    scaling = torch.exp(torch.randn((S, 3), generator=g) * 0.7) * 0.02
    xyz = torch.randn((S, 3), generator=g)
    if S >= 3:
        rotation[S // 2] = 0.0
        scaling[S // 3] = 1e-30
    return xyz, rotation, scaling


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N,scaling_cols", [(1, 2, 3), (65, 1, 3), (4097, 2, 3), (257, 3, 1), (100003, 2, 3)])
def test_restatement_against_the_torch_statements(S, N, scaling_cols):
    """R bit for bit, the children's positions of both routes within the bound, the scalings within 2 ulp (numpy's log and
    exp against torch's).  The host's vectorised torch.sqrt is not correctly rounded (it is one ulp off numpy's for 26 of
    4097 of these norms), which the device's and the kernel's are: R is compared bit for bit with the restatement given
    the host torch's own square root, that root is held to one ulp of the correctly rounded one, and the positions of the
    restatement with the correctly rounded root are bounded like the others."""
    from gftorf_amd import densify
    xyz, rotation, scaling = _rows_inputs(S, seed=S)
    if scaling_cols == 1:
        scaling = scaling[:, :1].expand(S, 3).contiguous()
    z = torch.randn((N * S, 3), generator=torch.Generator().manual_seed(S + 1))
    z[::5, 1] = 0.0
    z[1::7] = 0.0
    t_xyz, t_scaling, t_max, t_R = _torch_children(densify, xyz, rotation, scaling, z, N, scaling_cols)
    n_xyz, n_scaling, n_max, n_R, n_s = ref.children(xyz.numpy(), rotation.numpy(), scaling.numpy(), z.numpy(), N, scaling_cols)
    host_sqrt = lambda a: torch.sqrt(torch.from_numpy(a)).numpy()
    h_R = ref.rotation_matrices(rotation.numpy(), sqrt=host_sqrt)
    nan = np.isnan(h_R)
    assert np.array_equal(nan, np.isnan(t_R.numpy())) and int(nan.sum()) == (9 if S >= 3 else 0)
    assert np.array_equal(h_R.view(np.int32)[~nan], t_R.numpy().view(np.int32)[~nan])
    sums = (rotation.numpy() * rotation.numpy()).sum(axis=1, dtype=np.float32)
    assert int(_ulps(host_sqrt(sums), np.sqrt(sums)).max()) <= 1
    same_root = host_sqrt(sums).view(np.int32) == np.sqrt(sums).view(np.int32)
    assert np.array_equal(n_R.view(np.int32)[same_root][~nan[same_root]], h_R.view(np.int32)[same_root][~nan[same_root]])
    assert not np.signbit(n_s[n_s == 0]).any()                    # the + 0 turned every -0 into +0
    args = (xyz.numpy(), rotation.numpy(), scaling.numpy(), z.numpy(), N)
    worst_n = ref.assert_positions(n_xyz, *args, "restatement")
    worst_t = ref.assert_positions(t_xyz.numpy(), *args, "torch.bmm")
    print("S %d N %d: worst error / bound: restatement %.3f, torch.bmm %.3f" % (S, N, worst_n, worst_t))
    assert n_scaling.shape == tuple(t_scaling.shape) == (N * S, scaling_cols) and n_max.shape == tuple(t_max.shape)
    assert int(_ulps(n_scaling, t_scaling.numpy()).max()) <= 2
    # exp turns one ulp of a logarithm l into |l| ulps, so the largest scalings are each held to the exp of their own route's
    # logarithms
    for new_scaling, child_max in ((n_scaling, n_max), (t_scaling.numpy(), t_max.numpy())):
        assert int(_ulps(child_max, np.exp(new_scaling.astype(np.float64)).max(axis=1).astype(np.float32)).max()) <= 2
    if S >= 3:
        assert np.isnan(n_xyz[S // 2]).all() and not np.isnan(np.delete(n_xyz[:S], S // 2, axis=0)).any()


def test_the_entry_point_is_exported_and_refuses_bad_arguments_without_a_device():
    from gftorf_amd import _lib, densify
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gftorf_densify.h")).read()
    assert "gft_split_children" in _lib.EXPORTS and hasattr(lib, "gft_split_children") and "gft_split_children(" in header
    assert lib.gft_abi_version() == 16 == _lib.ABI_VERSION
    assert callable(densify.split_children)
    none = [None] * 6
    assert lib.gft_split_children(None, 0, 0, 2, *none) == 0                                # S = 0: nothing to do
    assert lib.gft_split_children(None, 10, 0, 1, *none) == 0
    for P, S, N, text in ((10, 0, 0, "N 0"), (10, 4, 0, "N 0"), (10, 4, -1, "N -1"), (10, 11, 2, "S 11"), (10, -1, 2, "S -1"),
                          (10, 4, 2, "NULL"), (1 << 31, 1 << 30, 2, "2^31")):
        assert lib.gft_split_children(None, P, S, N, *none) != 0, (P, S, N)
        assert text in _lib.last_error(), (text, _lib.last_error())
    # one NULL among valid pointers is refused as well (no device is touched: the check comes first)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for hole in range(6):
        a = [p] * 6
        a[hole] = None
        assert lib.gft_split_children(None, 10, 1, 2, *a) != 0 and "NULL" in _lib.last_error(), hole


def test_the_keyword_is_checked_and_nothing_runs_on_the_cpu():
    from gftorf_amd import densify
    a = densify_ref.EagerGaussians(8, "cpu", 1)
    grads = torch.zeros((8, 1))
    for children in ("x", None, "Kernel"):
        with pytest.raises(ValueError, match="children"):
            densify.densify_and_prune_fused(a, MAX_GRAD, MIN_OPACITY, EXTENT, children=children)
        with pytest.raises(ValueError, match="children"):
            densify.densify_and_split(a, grads, MAX_GRAD, EXTENT, children=children)
    with pytest.raises(RuntimeError, match="HIP device only"):
        densify.densify_and_prune_fused(a, MAX_GRAD, MIN_OPACITY, EXTENT, children="kernel")
    with pytest.raises(RuntimeError, match="HIP device only"):
        densify.densify_and_split(a, grads, MAX_GRAD, EXTENT, children="kernel")
    with pytest.raises(RuntimeError, match="HIP device only"):
        densify.split_children(a, torch.zeros(2, dtype=torch.int32), 2)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
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


def _model_with_split_rows(S, dev, isotropic):
    """A model of P = 3 S + 5 rows and S scattered split rows that include rows 0 and P - 1, the split rows' values from
    _rows_inputs (zero quaternion, 1e-30 scaling)."""
    P = 3 * S + 5
    m = densify_ref.EagerGaussians(P, dev, seed=S + 1)
    g = torch.Generator().manual_seed(S)
    rows = torch.randperm(P - 2, generator=g)[:max(S - 2, 0)] + 1
    rows = torch.cat((rows, torch.tensor([P - 1, 0][:min(S, 2)], dtype=torch.long))).sort().values
    assert rows.numel() == S and rows.unique().numel() == S
    xyz, rotation, scaling = _rows_inputs(S, seed=S)
    with torch.no_grad():
        m._xyz[rows.to(dev)] = xyz.to(dev)
        m._rotation[rows.to(dev)] = rotation.to(dev)
        m._scaling[rows.to(dev)] = torch.log(scaling).to(dev)
    if isotropic:
        _make_isotropic(m)
    return m, rows.to(torch.int32).to(dev)


def _gathered(m, rows):
    """The split rows' values as the kernel reads them, on the host: xyz, rotation, activated scaling [S, 3]."""
    r = rows.long()
    scaling = m.get_scaling.detach()
    if scaling.shape[1] == 1:
        scaling = scaling.expand(-1, 3)
    return m._xyz.detach()[r].cpu().numpy(), m._rotation.detach()[r].cpu().numpy(), scaling[r].cpu().numpy()


def _check_children(got, want, gathered, z, N, cols, what):
    """got / want: (new_xyz, new_scaling, child_max_scaling) of split_children and of the torch statements; the entry
    point alone gives new_xyz only."""
    S = gathered[0].shape[0]
    assert tuple(got[0].shape) == tuple(want[0].shape) == (N * S, 3), what
    if len(got) > 1:
        assert tuple(got[1].shape) == tuple(want[1].shape) == (N * S, cols) and tuple(got[2].shape) == tuple(want[2].shape) == (N * S,), what
        assert torch.equal(got[1], want[1]), (what, "new_scaling")
        assert torch.equal(got[2], want[2]), (what, "child_max_scaling")
    if S == 0:
        return
    z = z.cpu().numpy()
    got_xyz = got[0].cpu().numpy()
    worst_k = ref.assert_positions(got_xyz, *gathered, z, N, (what, "kernel"))
    worst_t = ref.assert_positions(want[0].cpu().numpy(), *gathered, z, N, (what, "torch.bmm"))
    # against the restatement fed the kernel's inputs: R is no output, so a wrong row or a transposed R shows here
    n_xyz, _, _, R, s = ref.children(*gathered, z, N, cols)
    terms = np.abs(np.tile(R, (N, 1, 1)).astype(np.float64) * s[:, None, :].astype(np.float64)).sum(axis=2)
    nan = np.isnan(n_xyz)
    assert np.array_equal(np.isnan(got_xyz), nan), what
    with np.errstate(invalid="ignore"):
        close = np.abs(got_xyz.astype(np.float64) - n_xyz.astype(np.float64)) <= 2 * EPS * terms + EPS * np.abs(n_xyz.astype(np.float64))
    assert (close | nan).all(), (what, "restatement", int((~(close | nan)).sum()))
    same = float(((got_xyz == want[0].cpu().numpy()) | nan).mean())
    print("%s: worst error / bound: kernel %.3f, torch.bmm %.3f; elements equal to torch.bmm's %.4f" % (what, worst_k, worst_t, same))


@pytest.mark.gpu
@pytest.mark.parametrize("isotropic", [False, True])
@pytest.mark.parametrize("S", [0, 1, 63, 64, 65, 257, 4097])
def test_split_children_against_the_torch_statements(gpu, S, isotropic):
    from gftorf_amd import _lib, densify
    lib = _lib.load()
    m, rows = _model_with_split_rows(S, gpu, isotropic)
    cols = 1 if isotropic else 3
    gathered = _gathered(m, rows)
    for N in (1, 2, 3):
        # under the same seed: split_children draws what the reference's torch.normal draws
        torch.manual_seed(40 + N)
        got = densify.split_children(m, rows, S, N)
        state = torch.cuda.get_rng_state(gpu)
        torch.manual_seed(40 + N)
        want = densify._children_torch(m, lib, m.get_scaling, rows, S, N)
        assert torch.equal(torch.cuda.get_rng_state(gpu), state), (S, N)
        torch.manual_seed(40 + N)
        z = torch.randn((N * S, 3), device=gpu)
        _check_children(got, want, gathered, z, N, cols, ("seeded", S, N, cols))
        if S == 0:
            continue
        # the entry point alone on normals with exact zeros (and -0 products) among them
        z = z.clone()
        z[::5, 1] = 0.0
        z[1::7] = 0.0
        scaling3 = torch.as_tensor(gathered[2]).to(gpu)
        P = m._xyz.shape[0]
        full = m.get_scaling.detach().expand(P, 3).contiguous()
        out = (torch.full((N * S, 3), 7.0, device=gpu),)
        _lib.check(lib.gft_split_children(_lib.raw_stream(gpu), P, S, N, rows.data_ptr(), m._xyz.data_ptr(), m._rotation.data_ptr(),
                                          full.data_ptr(), z.data_ptr(), out[0].data_ptr()))
        want = _torch_children(densify, torch.as_tensor(gathered[0]).to(gpu), torch.as_tensor(gathered[1]).to(gpu), scaling3, z, N, cols)
        _check_children(out, want[:3], gathered, z, N, cols, ("zeros", S, N, cols))
        zero = (z == 0).all(dim=1).cpu().numpy()                   # a child whose normals are all zero sits on its parent
        keep = zero & ~np.isnan(out[0].cpu().numpy()).any(axis=1)
        assert (keep.any() or N * S < 2) and np.array_equal(out[0].cpu().numpy()[keep], np.tile(gathered[0], (N, 1))[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 193, 100003])
def test_randn_consumes_the_generator_as_the_reference_normal_does(gpu, n):
    """torch.normal(mean=zeros, std) is randn * std + 0 and leaves the device generator where randn leaves it."""
    std = (torch.rand((n, 3), generator=torch.Generator().manual_seed(n)) + 0.01).to(gpu)
    torch.manual_seed(n)
    a = torch.normal(mean=torch.zeros((n, 3), device=gpu), std=std)
    state_a = torch.cuda.get_rng_state(gpu)
    after_a = torch.randn((5,), device=gpu)
    torch.manual_seed(n)
    z = torch.randn((n, 3), device=gpu)
    state_b = torch.cuda.get_rng_state(gpu)
    after_b = torch.randn((5,), device=gpu)
    assert torch.equal(a, z * std + 0.0)
    assert torch.equal(state_a, state_b) and torch.equal(after_a, after_b)


def _composite(densify, pc, max_grad, min_opacity, extent, max_screen_size, N, children):
    """densify.densify_and_prune's body with the split's N and children handed through."""
    grads = pc.xyz_gradient_accum / pc.denom
    grads[grads.isnan()] = 0.0
    densify.densify_and_clone(pc, grads, max_grad, extent)
    densify.densify_and_split(pc, grads, max_grad, extent, N=N, children=children)
    prune_mask = (pc.get_opacity < min_opacity).squeeze()
    if max_screen_size:
        big_points_vs = pc.max_radii2D > max_screen_size
        big_points_ws = pc.get_scaling.max(dim=1).values > 0.05 * extent
        small_points_ws = pc.get_scaling.max(dim=1).values < 0.001 * extent
        prune_mask = torch.logical_or(torch.logical_or(torch.logical_or(prune_mask, big_points_vs), big_points_ws), small_points_ws)
    densify.prune_points(pc, prune_mask)


def _fresh_statistics(models, rnd, dev):
    g = torch.Generator().manual_seed(7 + rnd)
    n = models[0]._xyz.shape[0]
    acc, den = (torch.rand((n, 1), generator=g) * 0.03).to(dev), torch.randint(0, 60, (n, 1), generator=g).float().to(dev)
    rad = (torch.rand(n, generator=g) * 30).to(dev)
    for m in models:
        m.xyz_gradient_accum, m.denom, m.max_radii2D = acc.clone(), den.clone(), rad.clone()


def _before(m):
    """What the children are formed from, on the host: the model's snapshot and its activated scaling as the device gives it."""
    d = {k: v.clone() for k, v in m.snapshot().items()}
    d["get_scaling"] = m.get_scaling.detach().cpu()
    return d


def _children_inputs(before, res, N, seed, dev):
    """Per child that survived the event (rows of kind 2 of the new model): its parent's xyz, rotation and activated scaling
    [n, 3] from the model before the event, and its normals, drawn again under the event's seed."""
    kind = res.kind.cpu()
    src, child = res.source_row.cpu().long()[kind == 2], res.child.cpu().long()[kind == 2]
    torch.manual_seed(seed)
    z = torch.randn((N * res.split, 3), device=dev).cpu()[child]
    scaling = before["get_scaling"]
    if scaling.shape[1] == 1:
        scaling = scaling.expand(-1, 3)
    return kind, (before["_xyz"][src].numpy(), before["_rotation"][src].numpy(), scaling[src].numpy(), z.numpy(), 1)


def _assert_twins(a, b, kind, inputs, what):
    """Every snapshot key of the kernel-driven model `a` equals the torch-driven `b`'s but the children's xyz rows, which both
    hold within the bound."""
    sa, sb = a.snapshot(), b.snapshot()
    assert set(sa) == set(sb), (what, sorted(set(sa) ^ set(sb)))
    for k in sa:
        assert sa[k].shape == sb[k].shape, (what, k)
        if k != "_xyz":
            assert torch.equal(sa[k], sb[k]), (what, k)
    other = kind != 2
    assert torch.equal(sa["_xyz"][other], sb["_xyz"][other]), (what, "_xyz of the rows that are no children")
    worst_k = ref.assert_positions(sa["_xyz"][~other].numpy(), *inputs, (what, "kernel"))
    worst_t = ref.assert_positions(sb["_xyz"][~other].numpy(), *inputs, (what, "torch.bmm"))
    print("%s: %d children, worst error / bound: kernel %.3f, torch.bmm %.3f" % (what, int((~other).sum()), worst_k, worst_t))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["size_rule", "no_size_rule", "isotropic", "three_children"])
@pytest.mark.parametrize("P", [65, 4097, 20000])
def test_fused_event_with_kernel_children_against_the_composite(gpu, P, case):
    """Three twins under the same generator state, two rounds: `a` the fused event with the kernel's children, `b` the
    composite with the torch statements, `c` the composite with the kernel's children (equal to `a` in every bit).  Before
    the second round `a` and `c` take `b`'s xyz (teacher forcing): the children of the first round differ from `b`'s within
    the bound, and the second round compares rows that are no children bit for bit."""
    from gftorf_amd import densify
    models = [densify_ref.EagerGaussians(P, gpu, seed=5) for _ in range(3)]
    a, b, c = models
    max_screen_size = None if case == "no_size_rule" else 20
    N = 3 if case == "three_children" else 2
    if case == "isotropic":
        for m in models:
            _make_isotropic(m)
    for rnd in range(2):
        before = _before(b)
        n_before = b._xyz.shape[0]
        seed = 100 + rnd
        torch.manual_seed(seed)
        res = densify.densify_and_prune_fused(a, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size, N=N, children="kernel")
        state_a = torch.cuda.get_rng_state(gpu)
        torch.manual_seed(seed)
        _composite(densify, b, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size, N, "torch")
        state_b = torch.cuda.get_rng_state(gpu)
        torch.manual_seed(seed)
        _composite(densify, c, MAX_GRAD, MIN_OPACITY, EXTENT, max_screen_size, N, "kernel")
        assert torch.equal(state_a, state_b) and torch.equal(torch.cuda.get_rng_state(gpu), state_b), (P, case, rnd)
        L.assert_same_snapshot(a, c, (P, case, rnd, "fused and composite, both with the kernel's children"))
        assert (res.P_before, res.P) == (n_before, b._xyz.shape[0])
        kind, inputs = _children_inputs(before, res, N, seed, gpu)
        _assert_twins(a, b, kind, inputs, (P, case, rnd))
        assert [g["name"] for g in a.optimizer.param_groups] == [g["name"] for g in b.optimizer.param_groups]
        assert a.optimizer.param_groups[0]["params"][0] is a._xyz
        if P >= 4097:
            assert res.split > 0 and int((kind == 2).sum()) > 0
        if case == "three_children" and P >= 4097:
            assert int((kind == 2).sum()) > 2 * res.split
        with torch.no_grad():
            a._xyz.copy_(b._xyz)
            c._xyz.copy_(b._xyz)
        _fresh_statistics(models, rnd, gpu)


@pytest.mark.gpu
def test_optimizer_step_after_an_event_with_kernel_children(gpu):
    """One FusedAdam step after the event, under a changed xyz rate: every group but xyz equals the composite-driven twin's;
    so do the xyz rows that are no children.  A child has zero moments, so its first update is a function of its gradient
    alone, the same number d on both twins: d = lr * (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) with m = (1 - b1) g,
    v = (1 - b2) g^2 and t = 2 (the group took one step before the event).  The optimizer forms d in float32 within a few
    roundings (8 eps |d| allowed) and rounds the new position once: bound after = bound before + 8 eps |d| + eps |exact - d|."""
    from gftorf_amd import FusedAdam, densify
    P, seed, lr = 4097, 21, 3.7e-4
    a, b = densify_ref.EagerGaussians(P, gpu, 5, optimizer_cls=FusedAdam), densify_ref.EagerGaussians(P, gpu, 5, optimizer_cls=FusedAdam)
    before = _before(b)
    torch.manual_seed(seed)
    res = densify.densify_and_prune_fused(a, MAX_GRAD, MIN_OPACITY, EXTENT, children="kernel")
    torch.manual_seed(seed)
    densify.densify_and_prune(b, MAX_GRAD, MIN_OPACITY, EXTENT)
    assert res.cloned > 0 and res.split > 0 and res.P != P
    kind, inputs = _children_inputs(before, res, 2, seed, gpu)
    _assert_twins(a, b, kind, inputs, "event")
    g = torch.Generator().manual_seed(4)
    grads = {grp["name"]: (torch.randn(grp["params"][0].shape, generator=g) * 1e-3).to(gpu) for grp in a.optimizer.param_groups}
    for m in (a, b):
        for grp in m.optimizer.param_groups:
            grp["params"][0].grad = grads[grp["name"]].clone()
            if grp["name"] == "xyz":
                grp["lr"] = lr
        m.optimizer.refresh_lr()
        m.optimizer.step()
    sa, sb = a.snapshot(), b.snapshot()
    assert set(sa) == set(sb)
    other = kind != 2
    for k in sa:
        if k != "_xyz":
            assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), k
    assert torch.equal(sa["_xyz"][other], sb["_xyz"][other])
    assert float(a.optimizer.state[a._xyz]["step"]) == 2.0
    gx = grads["xyz"].cpu().numpy().astype(np.float64)[~other.numpy()]
    b1, b2, t = 0.9, 0.999, 2
    d = lr * ((1 - b1) * gx / (1 - b1 ** t)) / (np.sqrt((1 - b2) * gx * gx / (1 - b2 ** t)) + 1e-15)
    exact = ref.exact(*inputs) - d
    bound = ref.position_bound(inputs[2], inputs[3], 1, ref.exact(*inputs)) + 8 * EPS * np.abs(d) + EPS * np.abs(exact)
    for name, s in (("kernel", sa), ("torch.bmm", sb)):
        err = np.abs(s["_xyz"][~other].numpy().astype(np.float64) - exact)
        assert (err <= bound).all(), (name, float((err / bound).max()))
        print("step after the event, %s: worst error / bound %.3f" % (name, float((err / bound).max())))
