"""Deformation network on the inputs and parameters the reference gives it: world coordinates (signed, as large as the
scene, scene/gaussian_model.py:170-174), times that include 0 and 1 exactly and pass the last view (train.py:169-176),
and the reference's own initialisation (Xavier trunk, zero biases, heads N(0, 1e-5): utils/time_utils.py:85-101).
tests/test_deform.py draws everything from x in [0, 1)^3, t in [0, 1) and heads N(0, 0.05).

The input sets are oracle/deform_ref.domain_inputs.  x 2^f is exact in float32 and float64 alike, so deform_ref in
float64 on the float32 inputs is the reference of EVERY row, the rows beyond the fp16 planes included.  Bounds: FWD_TOL /
BWD_TOL of tests/test_deform.py or, where that is larger, four times the float32 numpy oracle's own distance from float64
(the rule of test_forward_against_oracle); the CPU test at the end keeps that yardstick inside the tolerances.

Where the fp16 walk's input guard sits: it takes an encoded value v while |16 v| <= 65504, i.e. |x| <= 4094.
`plane_edge_below` / `plane_edge_above` (|x| around 255.875 = 4094 / 16, and 300) are on both sides of 16 |x| = 4094 and
BOTH stay on the fp16 walk; `guard_edge_below` (|x| in [4090, 4094], 4094 itself included) is the last stretch the walk
keeps and `guard_edge_above` (one coordinate 4096: 16 * 4096 is no fp16) must leave it for the fp32-range walk.  Decided by
result only: a walk that kept 4096 would return NaN, a call that left too early would still be right.

The encoding's switch at |2^f x| = 2^15: `reduction_switch` and `time_switch` put arguments below it, on it and above it
(up to 2^9 * 128.1 = 65.6 k), so a wrong result of either path there shows -- a broken constant, fused multiply-add or
quadrant select of the encoding's own reduction, or a library path that is wrong.  The constant itself is a choice of
speed, not of accuracy: restated in numpy (float32 with fused multiply-adds) the three-constant reduction stays within
1.0e-7 of float64's sine and cosine up to 2^20 and leaves that only beyond 2^21 (3e-6 at 2^22, 2e-4 at 2^24).  2^21 at
octave 9 is |x| = 4096, beyond the fp16 walk's guard, and there the x column itself (|x| against a sine's 1) carries the
output's max-norm.  So a switch lowered, or raised to anything up to 2^20, changes no result beyond rounding, and no
comparison with float64 at these tolerances can tell; a switch taken out altogether is not seen either, for the same
reason.  What is pinned is that both paths are right where the reference's scenes put their arguments."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import deform_modes
from oracle import deform_ref

FWD_TOL = 3e-6      # as tests/test_deform.py
BWD_TOL = 2e-5
KINDS = ("random", "init")
HEAD_STDS = (5e-2, 1e-3, 1e-5, 1e-6, 1e-7)
EXACT_ROWS = 4      # deform_ref.domain_inputs puts the rows with exact coordinates and times first

# (input set, t_multires, n): every set at the reference's 10 octaves of t, `time_switch` at 16 (2^15 t reaches the
# encoding's switch at t = 1), one set at the class default 6, one forward case of 65 points (one point past a tile)
FWD_CASES = [("signed_unit", 10, 333), ("signed_unit", 6, 333), ("room", 10, 333), ("room", 10, 65), ("far", 10, 333),
             ("reduction_switch", 10, 333), ("time_switch", 16, 333), ("plane_edge_below", 10, 333), ("plane_edge_above", 10, 333),
             ("guard_edge_below", 10, 333), ("guard_edge_above", 10, 333)]
BWD_CASES = [c for c in FWD_CASES if c[2] == 333]


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-30))


def _params(kind, seed, tm, head_std=None):
    if kind == "random":
        return deform_ref.random_params(seed, t_multires=tm)
    return deform_ref.reference_init_params(seed, tm) if head_std is None else deform_ref.reference_init_params(seed, tm, head_std)


def _net_of(params, dev, tm):
    from gftorf_amd.deform import DeformNetwork
    net = DeformNetwork(D=8, W=256, xyz_multires=10, t_multires=tm, sh_degree=3)
    net.load_state_dict({k: torch.tensor(v) for k, v in params.items()})
    return net.to(dev)


def _on_device(x, t, shared_t, dev):
    xt = torch.tensor(x, device=dev)
    tt = torch.tensor(t[:1], device=dev).expand(x.shape[0], -1) if shared_t else torch.tensor(t, device=dev)   # gaussian_model.py:171
    return xt, tt


def _check_forward(tag, out, ref, o32, n):
    """d_xyz and d_sh of one device forward against float64; prints the figures before it asserts."""
    d_xyz, d_rot, d_sh, d_sh_p = out
    assert d_xyz.shape == (n, 3) and d_sh.shape == (n, 16, 3) and d_rot.shape == (n, 4) and d_sh_p.shape == (n, 16, 2)
    assert not d_rot.any() and not d_sh_p.any()
    got = (d_xyz.detach().cpu().numpy(), d_sh.detach().cpu().numpy())
    errs = [_rel(got[0], ref[0]), _rel(got[1], ref[2])]
    orac = [_rel(o32[0], ref[0]), _rel(o32[2], ref[2])]
    print("FWD %s: device d_xyz %.3g d_sh %.3g | float32 oracle %.3g %.3g" % (tag, errs[0], errs[1], orac[0], orac[1]))
    for e, o, name in zip(errs, orac, ("d_xyz", "d_sh")):
        assert np.isfinite(e) and e < max(FWD_TOL, 4 * o), (tag, name, e, o)
    return max(errs)


def _check_grads(tag, grads, ref, o32):
    """Parameter gradients of one device backward against float64 (24 tensors; `rot` and `a` get none)."""
    assert sorted(grads) == sorted(k for k, v in ref.items() if v is not None) and len(grads) == 24
    errs = {k: _rel(g.cpu().numpy(), ref[k]) for k, g in grads.items()}
    orac = {k: _rel(o32[k], ref[k]) for k in grads}
    worst = max(errs, key=errs.get)
    print("BWD %s: device worst %.3g (%s; float32 oracle there %.3g) | float32 oracle worst %.3g"
          % (tag, errs[worst], worst, orac[worst], max(orac.values())))
    for k in errs:
        assert grads[k].shape == ref[k].shape
        assert np.isfinite(errs[k]) and errs[k] < max(BWD_TOL, 4 * orac[k]), (tag, k, errs[k], orac[k])


def _step(net, xt, tt, gx, gs):
    net.zero_grad(set_to_none=True)
    d_xyz, _, d_sh, _ = net(xt, tt)
    torch.autograd.backward([d_xyz, d_sh], [gx, gs])
    return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


def _far_from_a_relu_edge(params, name, n, seed):
    """n + n / 8 points of the set, the n furthest from a ReLU edge kept (a pre-activation within rounding of zero may
    switch differently in two arithmetics and moves the gradient by a finite amount); one point in nine is the cap.  The
    rows with exact values (the first EXACT_ROWS of every set) and the edited row are never among the dropped ones, as in
    make_golden.world_inputs; the margin asserted is that of every kept row, theirs included."""
    x, t, shared_t = deform_ref.domain_inputs(name, n + n // 8, seed)
    margin = deform_ref.relu_margin(params, x, t)
    rank = margin.copy()
    rank[:EXACT_ROWS] = np.inf
    if name in deform_ref.EDITED:
        rank[(x == deform_ref.EDITED[name]).any(axis=1)] = np.inf
    keep = np.sort(np.argsort(-rank)[:n])
    assert np.array_equal(keep[:EXACT_ROWS], np.arange(EXACT_ROWS)) and margin[keep].min() > 1e-6
    x0, t0 = x[:EXACT_ROWS].copy(), t[:EXACT_ROWS].copy()
    x, t = x[keep], t[keep]
    assert np.array_equal(x[:EXACT_ROWS].view(np.uint32), x0.view(np.uint32)) and np.array_equal(t[:EXACT_ROWS], t0)
    if name in deform_ref.EDITED:
        assert (x == deform_ref.EDITED[name]).sum() == 1          # the edited row is among the kept ones
    return x, t, shared_t


# ---------------------------------------------------------------------------------------------
# 1. forward against float64
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,tm,n", FWD_CASES)
def test_forward_against_float64(name, tm, n, kind):
    dev = torch.device("cuda:0")
    params = _params(kind, 41, tm)
    net = _net_of(params, dev, tm)
    x, t, shared_t = deform_ref.domain_inputs(name, n, 300 + n)
    ref = deform_ref.forward(params, x, t, dtype=np.float64)
    o32 = deform_ref.forward(params, x, t)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[2]).all()
    xt, tt = _on_device(x, t, shared_t, dev)
    with torch.no_grad():
        inference = net(xt, tt)
    saving = net(xt, tt)
    tag = "%s tm=%d n=%d %s" % (name, tm, n, kind)
    _check_forward(tag + " inference", inference, ref, o32, n)
    _check_forward(tag + " saving", saving, ref, o32, n)
    assert torch.equal(inference[0], saving[0]) and torch.equal(inference[2], saving[2])   # saving activations changes no result


# ---------------------------------------------------------------------------------------------
# 2. backward against float64: dense, blocking row selection, rows counted on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,tm,n", BWD_CASES)
def test_backward_against_float64(name, tm, n, kind):
    dev = torch.device("cuda:0")
    params = _params(kind, 42, tm)
    x, t, shared_t = _far_from_a_relu_edge(params, name, n, 400 + n)
    rng = np.random.default_rng(n)
    g_dxyz, g_dsh = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 16, 3)).astype(np.float32)
    # 30 % of the rows with a gradient: the rows with exact values (_far_from_a_relu_edge keeps them first) and the edited
    # one among them
    rows = rng.random(n) < 0.3
    rows[:EXACT_ROWS] = True
    if name in deform_ref.EDITED:
        rows |= (x == deform_ref.EDITED[name]).any(axis=1)
    k = int(rows.sum())
    assert 0.25 * n < k < 0.4 * n
    s_dxyz, s_dsh = g_dxyz * rows[:, None], g_dsh * rows[:, None, None]
    ref_all = deform_ref.backward(params, x, t, g_dxyz, g_dsh, dtype=np.float64)
    o32_all = deform_ref.backward(params, x, t, g_dxyz, g_dsh)
    ref_rows = deform_ref.backward(params, x, t, s_dxyz, s_dsh, dtype=np.float64)
    o32_rows = deform_ref.backward(params, x, t, s_dxyz, s_dsh)
    xt, tt = _on_device(x, t, shared_t, dev)
    up = lambda a, b: (torch.tensor(a, device=dev), torch.tensor(b, device=dev))
    tag = "%s tm=%d %s" % (name, tm, kind)
    net = _net_of(params, dev, tm)
    with deform_modes(sparse_backward=False, device_row_count=False) as D:
        dense = _step(net, xt, tt, *up(g_dxyz, g_dsh))
        assert D.last_backward_stats == {"points": n, "points_processed": n, "recomputed": False}
    _check_grads(tag + " dense", dense, ref_all, o32_all)
    # the blocking selection: a forward that keeps nothing, the count read by the host, the k rows recomputed
    net = _net_of(params, dev, tm)
    with deform_modes(sparse_backward=True, device_row_count=False, lazy_save=True, _SPARSE_MAX_FRACTION=2.0, _SPARSE_MIN_POINTS=0) as D:
        net._save_state = {"fraction": 0.0}
        blocking = _step(net, xt, tt, *up(s_dxyz, s_dsh))
        assert D.last_backward_stats == {"points": n, "points_processed": k, "recomputed": True}
    _check_grads(tag + " blocking rows", blocking, ref_rows, o32_rows)
    # the rows counted on the device: xyz and t are encoded again by a second forward over the rows that count
    net = _net_of(params, dev, tm)
    with deform_modes(sparse_backward=True, device_row_count=True, lazy_save=True, _SPARSE_MIN_POINTS=0) as D:
        counted = _step(net, xt, tt, *up(s_dxyz, s_dsh))
        st = dict(D.last_backward_stats)
        assert st["recomputed"] and int(st["rows_on_device"].item()) == k
    _check_grads(tag + " device rows", counted, ref_rows, o32_rows)
    for q in blocking:
        assert torch.equal(counted[q], blocking[q]), q            # the same kernels on the same compacted rows


# ---------------------------------------------------------------------------------------------
# 3. both sides of the planes' edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(deform_ref.EDITED))
def test_one_coordinate_beyond_an_edge_leaves_the_other_rows_alone(name):
    """`room` with one coordinate of one row at 300 (inside the planes) or 4096 (beyond them: the whole call is redone by
    the fp32-range walk): every other row is what the unedited call gives, within FWD_TOL, and the edited row itself is
    right against float64 (test_forward_against_float64 has it among its rows; here it is looked at alone)."""
    dev = torch.device("cuda:0")
    n = 333
    for kind in KINDS:
        params = _params(kind, 43, 10)
        net = _net_of(params, dev, 10)
        x, t, _ = deform_ref.domain_inputs(name, n, 77)
        x0, t0, _ = deform_ref.domain_inputs("room", n, 77)
        row = n // 2
        assert x[row, 1] == deform_ref.EDITED[name] and np.array_equal(np.delete(x, row, 0), np.delete(x0, row, 0)) and np.array_equal(t, t0)
        with torch.no_grad():
            a = net(torch.tensor(x, device=dev), torch.tensor(t, device=dev))
            b = net(torch.tensor(x0, device=dev), torch.tensor(t0, device=dev))
        others = np.arange(n) != row
        for i in (0, 2):
            assert _rel(a[i].cpu().numpy()[others], b[i].cpu().numpy()[others]) < FWD_TOL, (name, kind, i)
        ref = deform_ref.forward(params, x[row:row + 1], t[row:row + 1], dtype=np.float64)
        full = deform_ref.forward(params, x, t, dtype=np.float64)
        for i in (0, 2):    # (of the batch's max-norm, as everywhere)
            err = float(np.abs(a[i].cpu().numpy()[row].astype(np.float64) - ref[i][0]).max() / np.abs(full[i]).max())
            print("EDGE %s %s output %d: edited row %.3g" % (name, kind, i, err))
            assert err < FWD_TOL, (name, kind, i, err)


# ---------------------------------------------------------------------------------------------
# 4. head magnitudes from the suite's 0.05 down to 1e-7, and a head that is exactly zero
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _sweep_points():
    """`room`, 1500 points far from a ReLU edge of the trunk (the heads have no ReLU: one selection for every head_std)."""
    params = deform_ref.reference_init_params(44, 10)
    x, t, _ = _far_from_a_relu_edge(params, "room", 1500, 9)
    rng = np.random.default_rng(10)
    return x, t, rng.normal(size=(1500, 3)).astype(np.float32), rng.normal(size=(1500, 16, 3)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("head_std", HEAD_STDS)
def test_head_magnitude_sweep(head_std):
    """The reference starts its heads at N(0, 1e-5) and they stay small for the first iterations.  The bounds are of the
    output's (the gradient's) max-norm, so they ask the same at every magnitude: a weight plane that keeps fewer digits of
    a small head shows here."""
    dev = torch.device("cuda:0")
    n = 1500
    params = _params("init", 44, 10, head_std)
    x, t, g_dxyz, g_dsh = _sweep_points()
    net = _net_of(params, dev, 10)
    xt, tt = torch.tensor(x, device=dev), torch.tensor(t, device=dev)
    tag = "room n=%d head_std=%g" % (n, head_std)
    ref = deform_ref.forward(params, x, t, dtype=np.float64)
    o32 = deform_ref.forward(params, x, t)
    with torch.no_grad():
        _check_forward(tag + " inference", net(xt, tt), ref, o32, n)
    _check_forward(tag + " saving", net(xt, tt), ref, o32, n)
    with deform_modes(sparse_backward=False, device_row_count=False):
        grads = _step(net, xt, tt, torch.tensor(g_dxyz, device=dev), torch.tensor(g_dsh, device=dev))
    _check_grads(tag + " dense", grads, deform_ref.backward(params, x, t, g_dxyz, g_dsh, dtype=np.float64),
                 deform_ref.backward(params, x, t, g_dxyz, g_dsh))


@pytest.mark.gpu
@pytest.mark.parametrize("zeroed", ["g", "all"])
def test_a_head_of_zero_weights_gives_its_bias_and_no_trunk_gradient(zeroed):
    """A weight matrix that is exactly zero: its outputs are its bias bit for bit, and with an upstream gradient on its
    outputs alone every trunk gradient is exactly zero (its own weight and bias gradients are not)."""
    dev = torch.device("cuda:0")
    n = 333
    params = _params("init", 45, 10)
    rng = np.random.default_rng(46)
    heads = ("g",) if zeroed == "g" else deform_ref.HEADS
    for h in deform_ref.HEADS:
        params[h + ".bias"] = rng.normal(0.0, 0.3, params[h + ".bias"].shape).astype(np.float32)
    for h in heads:
        params[h + ".weight"][:] = 0.0
    x, t, _ = deform_ref.domain_inputs("room", n, 47)
    net = _net_of(params, dev, 10)
    xt, tt = torch.tensor(x, device=dev), torch.tensor(t, device=dev)
    with torch.no_grad():
        inference = net(xt, tt)
    d_xyz, _, d_sh, _ = net(xt, tt)
    for out in ((inference[0], inference[2]), (d_xyz.detach(), d_sh.detach())):
        o_xyz, o_sh = out[0].cpu().numpy(), out[1].cpu().numpy()
        for h in heads:
            got = o_xyz if h == "xyz_warp" else o_sh[:, :, "rgb".index(h)]
            assert np.array_equal(got.view(np.uint32), np.broadcast_to(params[h + ".bias"], got.shape).view(np.uint32)), h
    # the heads that are not zero are still right
    ref = deform_ref.forward(params, x, t, dtype=np.float64)
    assert _rel(d_sh.detach().cpu().numpy(), ref[2]) < FWD_TOL and _rel(d_xyz.detach().cpu().numpy(), ref[0]) < FWD_TOL
    g_dxyz = torch.tensor(rng.normal(size=(n, 3)).astype(np.float32), device=dev)
    g_dsh = torch.tensor(rng.normal(size=(n, 16, 3)).astype(np.float32), device=dev)
    if zeroed == "g":
        g_dxyz.zero_()
        g_dsh[:, :, 0] = 0
        g_dsh[:, :, 2] = 0
    net.zero_grad(set_to_none=True)
    with deform_modes(sparse_backward=False, device_row_count=False):
        torch.autograd.backward([d_xyz, d_sh], [g_dxyz, g_dsh])
    grads = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    assert len(grads) == 24
    for k, g in grads.items():
        if k.startswith("linear."):
            assert not g.any(), k
    for h in heads:
        assert grads[h + ".weight"].any() and grads[h + ".bias"].any()
    gref = deform_ref.backward(params, x, t, g_dxyz.cpu().numpy(), g_dsh.cpu().numpy(), dtype=np.float64)
    for h in heads:
        assert _rel(grads[h + ".weight"].cpu().numpy(), gref[h + ".weight"]) < BWD_TOL, h
        assert _rel(grads[h + ".bias"].cpu().numpy(), gref[h + ".bias"]) < BWD_TOL, h


# ---------------------------------------------------------------------------------------------
# 5. golden vectors of the reference's own module on world-space inputs at its own initialisation
# ---------------------------------------------------------------------------------------------
GOLDEN_WORLD = os.path.join(os.path.dirname(__file__), "golden", "deform_world.npz")


def test_oracle_matches_reference_module_on_world_inputs():
    g = np.load(GOLDEN_WORLD)
    tm = int(g["kwargs"][3])
    assert tm == 10 and g["x"].shape == (48, 3) and np.abs(g["x"]).max() > 128 and g["x"].min() < -128
    assert {0.0, 1.0} <= set(g["t"][:, 0].tolist()) and g["t"].max() > 1 and g["t"].min() < 0
    params = deform_ref.reference_init_params(int(g["seed"]), tm)
    d_xyz, d_rot, d_sh, d_sh_p = deform_ref.forward(params, g["x"], g["t"])
    assert d_xyz.shape == g["d_xyz"].shape and d_sh.shape == g["d_sh"].shape == (48, 16, 3)
    assert _rel(d_xyz, g["d_xyz"]) < 2e-6 and _rel(d_sh, g["d_sh"]) < 2e-6
    assert d_rot.shape == g["d_rot"].shape and not d_rot.any() and not g["d_rot"].any()
    assert d_sh_p.shape == g["d_sh_p"].shape and not d_sh_p.any() and not g["d_sh_p"].any()
    grads = deform_ref.backward(params, g["x"], g["t"], g["g_dxyz"], g["g_dsh"])
    assert sorted(n for n, v in grads.items() if v is None) == sorted(g["grad_none"].tolist())
    seen = 0
    for key in g.files:
        if key.startswith("grad:"):
            assert _rel(grads[key[5:]], g[key]) < 5e-6, key
            seen += 1
        elif key.startswith("grad_s:"):
            assert _rel(grads[key[7:]][::8, ::4], g[key]) < 5e-6, key
            seen += 1
    assert seen == 2 * 8 + 2 * 4


@pytest.mark.gpu
def test_device_matches_reference_module_on_world_inputs():
    dev = torch.device("cuda:0")
    g = np.load(GOLDEN_WORLD)
    tm = int(g["kwargs"][3])
    net = _net_of(deform_ref.reference_init_params(int(g["seed"]), tm), dev, tm)
    xt, tt = torch.tensor(g["x"], device=dev), torch.tensor(g["t"], device=dev)
    with torch.no_grad():
        inference = net(xt, tt)
    d_xyz, d_rot, d_sh, d_sh_p = net(xt, tt)
    for a, b in ((inference[0], inference[2]), (d_xyz.detach(), d_sh.detach())):
        e_xyz, e_sh = _rel(a.cpu().numpy(), g["d_xyz"]), _rel(b.cpu().numpy(), g["d_sh"])
        print("GOLDEN world: d_xyz %.3g d_sh %.3g" % (e_xyz, e_sh))
        assert e_xyz < FWD_TOL and e_sh < FWD_TOL
    assert d_rot.shape == g["d_rot"].shape and not d_rot.any()
    assert d_sh_p.shape == g["d_sh_p"].shape and not d_sh_p.any()
    ((d_xyz * torch.tensor(g["g_dxyz"], device=dev)).sum() + (d_sh * torch.tensor(g["g_dsh"], device=dev)).sum()).backward()
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert sorted(k for k, v in grads.items() if v is None) == sorted(g["grad_none"].tolist())
    for key in g.files:
        if key.startswith("grad:"):
            assert _rel(grads[key[5:]].cpu().numpy(), g[key]) < BWD_TOL, key
        elif key.startswith("grad_s:"):
            assert _rel(grads[key[7:]].cpu().numpy()[::8, ::4], g[key]) < BWD_TOL, key


# ---------------------------------------------------------------------------------------------
# 6. the bf16 walks on the same inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bf16_walks_on_the_same_inputs():
    """GFT_DEFORM_FP16X2=0 GFT_DEFORM_BWD_FP16=0: forward and backward on three bf16 planes (what runs when a value does not
    fit the fp16 planes) over tests 1, 2 and 4, in one child process."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x",
                        "-k", "forward_against_float64 or backward_against_float64 or head_magnitude_sweep"],
                       env=dict(os.environ, GFT_DEFORM_FP16X2="0", GFT_DEFORM_BWD_FP16="0"), cwd=root, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout


# ---------------------------------------------------------------------------------------------
# 7. a point's result does not depend on the batch it is in
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_batch_independence_on_large_coordinates(kind):
    dev = torch.device("cuda:0")
    params = _params(kind, 48, 10)
    net = _net_of(params, dev, 10)
    xa, ta, _ = deform_ref.domain_inputs("far", 333, 1)
    xb, tb, _ = deform_ref.domain_inputs("reduction_switch", 333, 2)
    x = torch.tensor(np.concatenate([xa, xb]), device=dev)
    t = torch.tensor(np.concatenate([ta, tb]), device=dev)
    n = x.shape[0]
    with torch.no_grad():
        whole = net(x, t)
    assert torch.isfinite(whole[0]).all() and torch.isfinite(whole[2]).all()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(dev)
    for idx in (perm[:n // 2], perm[n // 2:]):
        with torch.no_grad():
            part = net(x[idx], t[idx])
        assert torch.equal(part[0], whole[0][idx]) and torch.equal(part[2], whole[2][idx])


# ---------------------------------------------------------------------------------------------
# CPU: the float32 numpy oracle stays inside the tolerances on these inputs (the GPU bounds lean on it)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", deform_ref.DOMAIN_SETS)
def test_float32_oracle_close_to_float64_on_every_input_set(name, kind):
    tm = 16 if name == "time_switch" else 10
    n = 333
    params = _params(kind, 42, tm)
    x, t, _ = _far_from_a_relu_edge(params, name, n, 400 + n)
    a, b = deform_ref.forward(params, x, t), deform_ref.forward(params, x, t, dtype=np.float64)
    assert _rel(a[0], b[0]) < FWD_TOL and _rel(a[2], b[2]) < FWD_TOL
    rng = np.random.default_rng(n)
    g_dxyz, g_dsh = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 16, 3)).astype(np.float32)
    ga, gb = deform_ref.backward(params, x, t, g_dxyz, g_dsh), deform_ref.backward(params, x, t, g_dxyz, g_dsh, dtype=np.float64)
    for k, v in gb.items():
        if v is not None:
            assert _rel(ga[k], v) < BWD_TOL, k


def test_input_sets_hold_what_they_are_named_for():
    sets = {name: deform_ref.domain_inputs(name, 333, 5) for name in deform_ref.DOMAIN_SETS}
    x, t, _ = sets["signed_unit"]
    assert x.min() < -0.9 and x.max() > 0.9 and np.signbit(x[1]).all() and not x[0].any() and t[0] == 0 and t[1] == 1
    x, t, _ = sets["room"]
    assert x.min() < -7 and x.max() > 7 and np.allclose(t[2:4, 0], [-0.04, 1.04])
    x, t, shared_t = sets["far"]
    assert shared_t and np.abs(x).max() > 55 and 512 * np.abs(x).max() < 32768 and (t == t[0]).all()
    x, t, _ = sets["reduction_switch"]
    a = np.abs(x.astype(np.float64))
    assert ((np.abs(a - 64) <= 0.1001) | (np.abs(a - 128) <= 0.1001)).all() and (x < 0).any() and (x > 0).any()
    assert ((512 * a < 32768).any() and (512 * a > 32768).any() and (256 * a < 32768).any() and (256 * a[a > 100] > 32768).any())
    assert all(v in x for v in (64.0, -64.0, 128.0, -128.0))
    x, t, _ = sets["time_switch"]
    assert sorted(set(t[:, 0].tolist())) == [0.0, float(np.float32(1 - 2.0 ** -16)), 1.0, float(np.float32(1.04))]
    x, t, _ = sets["plane_edge_below"]
    assert (np.abs(x) >= 255).all() and (16 * np.abs(x.astype(np.float64)) < 4094).all() and (x < 0).any() and (x > 0).any()
    x, t, _ = sets["guard_edge_below"]
    assert (16 * np.abs(x.astype(np.float64)) <= 65504).all() and (np.abs(x) >= 4090).all() and 4094.0 in x and -4094.0 in x
    for name, v in deform_ref.EDITED.items():
        x, t, _ = sets[name]
        assert (x == v).sum() == 1 and np.array_equal(t, sets["room"][1])
    assert 16 * deform_ref.EDITED["plane_edge_above"] <= 65504 < 16 * deform_ref.EDITED["guard_edge_above"]
