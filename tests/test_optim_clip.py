"""Gradient-norm clipping (reference train.py:468, `torch.nn.utils.clip_grad_norm_(deform.parameters(), max_norm=1.0)`):
`gftorf_amd.clip_grad_norm_`, `FusedAdam.step(max_grad_norm=...)`, and the row-masked step of the capturable optimizer.
torch is the reference throughout: the statement that is replaced is a torch call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch


# ---- without a GPU ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


def test_drop_in_rejects_cpu_gradients_and_other_norms():
    import gftorf_amd
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="HIP device only"):
        gftorf_amd.clip_grad_norm_([p], 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gftorf_amd.clip_grad_norm_(p, 1.0)                    # a single tensor, as torch takes it
    with pytest.raises(NotImplementedError):
        gftorf_amd.clip_grad_norm_([p], 1.0, norm_type=1)
    with pytest.raises(NotImplementedError):
        gftorf_amd.clip_grad_norm_([p], 1.0, norm_type=float("inf"))
    q = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    got, want = gftorf_amd.clip_grad_norm_(q, 1.0), torch.nn.utils.clip_grad_norm_(q, 1.0)
    assert got.shape == want.shape == () and got.dtype == want.dtype and float(got) == float(want) == 0.0


def test_no_gradient_at_all_does_not_load_the_library(monkeypatch):
    import gftorf_amd
    from gftorf_amd import _lib

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", boom)
    assert float(gftorf_amd.clip_grad_norm_([torch.nn.Parameter(torch.zeros(3))], 1.0)) == 0.0
    assert float(gftorf_amd.clip_grad_norm_([], 1.0)) == 0.0


def test_new_entry_points_report_argument_errors_and_take_empty_tables(lib):
    from gftorf_amd import _lib
    tab = (_lib.AdamTensor * 1)()
    ptrs, ns = (C.c_void_p * 1)(), (C.c_int64 * 1)(4)
    dev = C.c_void_p(256)        # stands for a device pointer: no call below gets as far as a launch
    # name -> (arguments with `count` as a hole, the same with the host tables NULL).  gft_adam_step is one function: its four
    # argument shapes (dense / rows x learning rates in the table / on the device, each with a grad_scale) are named after it
    adam = lambda rows, mask, dev_rates: lambda n, t: (
        None, n, tab if t else None, rows, mask, ptrs if dev_rates and t else None, ptrs if dev_rates and t else None,
        dev if dev_rates else None, 0.9, 0.999, 1e-8, 0.0, dev)
    calls = {
        "gft_grad_norm": lambda n, t: (None, n, ptrs if t else None, ns if t else None, 1.0, dev, 64, dev),
        "gft_grad_scale": lambda n, t: (None, n, ptrs if t else None, ns if t else None, dev),
        "gft_adam_step dense host": adam(0, None, False),
        "gft_adam_step rows host": adam(5, dev, False),
        "gft_adam_step dense device": adam(0, None, True),
        "gft_adam_step rows device": adam(5, dev, True),
    }
    for what, args in calls.items():
        name = what.split()[0]
        fn = getattr(lib, name)
        assert fn(*args(-1, True)) != 0, what
        assert (name + ":") in _lib.last_error() and "count < 0" in _lib.last_error(), (what, _lib.last_error())
        assert fn(*args(1, False)) != 0, what
        assert (name + ":") in _lib.last_error() and "NULL" in _lib.last_error(), (what, _lib.last_error())
    # nothing to do: 0, and no device is touched (this test runs without one).  gft_grad_norm with an `out` has {0, 1} to
    # write, so "nothing to do" is count == 0 with out == NULL
    for what, args in calls.items():
        a = list(args(0, True))
        if what == "gft_grad_norm":
            a[-1] = None
        assert getattr(lib, what.split()[0])(*a) == 0, what
    # the per-span checks come before any launch as well
    bad = (C.c_int64 * 1)(-4)
    assert lib.gft_grad_norm(None, 1, ptrs, bad, 1.0, dev, 64, dev) != 0 and "gft_grad_norm: span 0 has n < 0" in _lib.last_error()
    assert lib.gft_grad_norm(None, 1, ptrs, ns, 1.0, dev, 64, dev) != 0 and "NULL pointer" in _lib.last_error()
    odd = (C.c_void_p * 1)(258)
    assert lib.gft_grad_scale(None, 1, odd, ns, dev) != 0 and "4-byte aligned" in _lib.last_error()
    ok = (C.c_void_p * 1)(260)
    assert lib.gft_grad_norm(None, 1, ok, ns, 1.0, dev, 0, dev) != 0 and "scratch" in _lib.last_error()
    assert lib.gft_grad_norm(None, 1, ok, ns, 1.0, dev, 64, None) != 0 and "out is NULL" in _lib.last_error()
    assert lib.gft_adam_step(None, 1, tab, 0, dev, ptrs, ptrs, dev, 0.9, 0.999, 1e-8, 0.0, None) != 0
    assert "gft_adam_step:" in _lib.last_error() and "rows must be > 0" in _lib.last_error()
    # what one function for all of them can be handed that the eight could not: rows without a mask, half of the device rates
    assert lib.gft_adam_step(None, 1, tab, 5, None, None, None, None, 0.9, 0.999, 1e-8, 0.0, None) != 0
    assert "gft_adam_step:" in _lib.last_error() and "row_mask" in _lib.last_error()
    assert lib.gft_adam_step(None, 1, tab, 0, None, ptrs, None, dev, 0.9, 0.999, 1e-8, 0.0, None) != 0
    assert "gft_adam_step:" in _lib.last_error() and "NULL" in _lib.last_error()
    # the size query: host only, one double per workgroup of 4096 elements and at most one more per span
    q = lib.gft_grad_norm_scratch_bytes
    assert q(0, 0) == 8 and q(-1, 0) == 0 and q(0, -1) == 0
    assert q(516915, 24) == 8 * (516915 // 4096 + 24 + 1) and q(10 ** 10, 3) >= 8 * (10 ** 10 // 4096)


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
def groups(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=g).to(dev))
    # shapes of the reference's parameter groups (xyz, f_dc, f_rest, opacity, scaling, rotation, an odd one)
    ps = [mk(1001, 3), mk(1001, 1, 3), mk(1001, 15, 3), mk(1001, 1), mk(1001, 3), mk(1001, 4), mk(7)]
    lrs = [1.6e-4, 2.5e-3, 1.25e-4, 0.05, 5e-3, 1e-3, 0.0]
    return [{"params": [p], "lr": lr, "name": str(i)} for i, (p, lr) in enumerate(zip(ps, lrs))]


def network_shapes():
    """The 24 tensors of DeformNetwork(xyz_multires=10, t_multires=10) that receive a gradient (rot and a get none)."""
    widths = [84, 256, 256, 256, 256, 340, 256, 256]
    shapes = []
    for w in widths:
        shapes += [(256, w), (256,)]
    for rows in (3, 16, 16, 16):
        shapes += [(rows, 256), (rows,)]
    assert len(shapes) == 24 and sum(int(np.prod(s)) for s in shapes) == 516915
    return shapes


SIZES_B = [0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1025, 2049]
KINDS = ["network", "sizes", "odd_views", "backward"]


def _with_grads(grads):
    ps = []
    for g in grads:
        p = torch.nn.Parameter(torch.empty(g.shape, device=g.device))
        p.grad = g
        ps.append(p)
    return ps


def make_set(kind, dev, seed=0):
    """Parameters with gradients of unit scale (the tests scale them to a norm of their choice)."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    if kind == "network":
        return _with_grads([rnd(*s) for s in network_shapes()])
    if kind == "sizes":
        sizes = SIZES_B + SIZES_B + SIZES_B[:11]             # 45 spans: two launches of the 40-entry table
        assert len(sizes) == 45
        return _with_grads([rnd(n) for n in sizes])
    if kind == "odd_views":
        two, buf, buf2 = rnd(2), rnd(1040), rnd(64)
        grads = [two[1:2], buf[3:1033], rnd(5), buf2[2:4], buf2[9:16]]
        assert [g.data_ptr() % 16 for g in grads] == [4, 12, 0, 8, 4]
        return _with_grads(grads)
    # the gradients an actual backward of the network leaves: consecutive views of one flat buffer
    import gftorf_amd
    torch.manual_seed(seed)
    net = gftorf_amd.reference_network().to(dev)
    x, t = rnd(500, 3), torch.rand(500, 1, generator=gen).to(dev)
    d_xyz, _, d_sh, _ = net(x, t, zeros_as_scalars=True)
    (d_xyz.sum() + d_sh.sum()).backward()
    ps = [p for p in net.parameters() if p.grad is not None]
    assert len(ps) == 24 and sum(p.numel() for p in ps) == 516915
    assert len({p.grad.untyped_storage().data_ptr() for p in ps}) == 1
    return ps


def whole(g):
    """The gradient's whole allocation as a flat tensor (what lies around a view must stay as it was)."""
    return torch.as_strided(g, (g.untyped_storage().nbytes() // 4,), (1,), 0)


def fresh_copy(ps):
    """New parameters whose gradients are copies placed exactly as the originals: every allocation is copied whole, and views keep
    their offsets, so the copy has the same 16-byte phases (and the same neighbours)."""
    copies, out = {}, []
    for p in ps:
        g = p.grad
        key = g.untyped_storage().data_ptr()
        if key not in copies:
            copies[key] = whole(g).clone()
        q = torch.nn.Parameter(torch.empty(p.shape, device=p.device))
        q.grad = torch.as_strided(copies[key], g.shape, g.stride(), g.storage_offset())
        assert q.grad.data_ptr() % 16 == g.data_ptr() % 16
        out.append(q)
    return out


def norm64(ps):
    tot = torch.zeros((), dtype=torch.float64, device=ps[0].grad.device)
    for p in ps:
        tot += (p.grad.double() ** 2).sum()
    return float(tot.sqrt())


def scale_set(ps, target):
    k = target / norm64(ps)
    seen = set()
    for p in ps:
        key = p.grad.untyped_storage().data_ptr()
        if key not in seen:
            seen.add(key)
            whole(p.grad).mul_(k)
    return ps


def bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("target", [0.3, 1.0, 40.0])
@pytest.mark.parametrize("kind", KINDS)
def test_norm_scaled_gradients_and_determinism(kind, target, gpu):
    """The drop-in against float64 and against torch's own function on the same device gradients: the norm within four times
    torch's error (at least 8 fp32 ulps: a lane adds at most 22 squares in fp32, everything above in double), the gradients
    equal to g * c bit for bit with c formed by torch from the returned norm, and the same bits from a second call."""
    import gftorf_amd
    ps = scale_set(make_set(kind, gpu), target)
    ref = norm64(ps)
    before = [p.grad.clone() for p in ps]
    around = {p.grad.untyped_storage().data_ptr(): whole(p.grad).clone() for p in ps}
    twin, other = fresh_copy(ps), fresh_copy(ps)
    err_torch = abs(float(torch.nn.utils.clip_grad_norm_(twin, 1.0).double()) - ref)
    got = gftorf_amd.clip_grad_norm_(ps, 1.0)
    assert got.shape == () and got.dtype == torch.float32 and got.device == gpu
    err = abs(float(got.double()) - ref)
    ulp = float(np.spacing(np.float32(ref)))
    bound = max(4 * err_torch, 8 * ulp)
    print("clip norm %-9s target %-5g: ours %.3g (%.2f ulp), torch %.3g (%.2f ulp), ratio to the bound %.3f"
          % (kind, target, err, err / ulp, err_torch, err_torch / ulp, err / bound))
    assert err <= bound, (err, err_torch, ulp)
    c = torch.clamp(1.0 / (got + 1e-6), max=1.0)
    assert c.dtype == torch.float32
    clamped = float(got) + 1e-6 < 1.0
    assert clamped == (float(c) == 1.0) and (target < 0.9) == clamped
    for p, g0 in zip(ps, before):
        assert torch.equal(bits(p.grad), bits(g0 * c)), tuple(p.shape)
        if clamped:
            assert torch.equal(bits(p.grad), bits(g0))
    # what lies around the views is as it was (the elements of the views themselves are compared above)
    for p in ps:
        w, w0 = whole(p.grad), around[p.grad.untyped_storage().data_ptr()]
        inside = torch.zeros_like(w, dtype=torch.bool)
        for q in ps:
            if q.grad.untyped_storage().data_ptr() == p.grad.untyped_storage().data_ptr():
                inside[q.grad.storage_offset():q.grad.storage_offset() + q.grad.numel()] = True
        assert torch.equal(bits(w[~inside]), bits(w0[~inside]))
    again = gftorf_amd.clip_grad_norm_(other, 1.0)
    assert torch.equal(bits(got), bits(again))
    for p, q in zip(ps, other):
        assert torch.equal(bits(p.grad), bits(q.grad))


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_values_follow_torch(bad, gpu):
    import gftorf_amd
    ps = scale_set(make_set("sizes", gpu, seed=4), 40.0)
    assert ps[16].grad.numel() == 2049
    ps[16].grad[100] = bad
    twin, third = fresh_copy(ps), fresh_copy(ps)
    want = torch.nn.utils.clip_grad_norm_(twin, 1.0)
    got = gftorf_amd.clip_grad_norm_(ps, 1.0)
    assert bool(torch.isnan(got)) == bool(torch.isnan(want)) and bool(torch.isinf(got)) == bool(torch.isinf(want))
    assert bool(torch.isnan(got)) or bool(torch.isinf(got))
    for p, q in zip(ps, twin):
        for f in (torch.isnan, torch.isinf, lambda t: t == 0):
            assert torch.equal(f(p.grad), f(q.grad))
    keep = [p.grad.clone() for p in third]
    with pytest.raises(RuntimeError, match="non-finite"):
        gftorf_amd.clip_grad_norm_(third, 1.0, error_if_nonfinite=True)
    for p, g0 in zip(third, keep):                        # torch raises before it scales
        assert torch.equal(bits(p.grad), bits(g0))
    # finite gradients pass the check
    fine = scale_set(make_set("odd_views", gpu), 3.0)
    assert abs(float(gftorf_amd.clip_grad_norm_(fine, 1.0, error_if_nonfinite=True)) - 3.0) < 1e-5


def _twins(dev, n, wd=0.0, cls=None, seed=0, **kw):
    from gftorf_amd import FusedAdam
    return [(cls or FusedAdam)(groups(dev, seed=seed), lr=0.0, eps=1e-15, weight_decay=wd, **kw) for _ in range(n)]


def _params(opt):
    return [p for g in opt.param_groups for p in g["params"]]


def _assert_same_state(a, b, what=""):
    for ga, gb in zip(a.param_groups, b.param_groups):
        pa, pb = ga["params"][0], gb["params"][0]
        assert (pa in a.state) == (pb in b.state)
        assert torch.equal(bits(pa), bits(pb)), "param of group %s %s" % (ga["name"], what)
        if pa in a.state:
            sa, sb = a.state[pa], b.state[pb]
            assert float(sa["step"]) == float(sb["step"]), ga["name"]
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(bits(sa[k]), bits(sb[k])), "%s of group %s %s" % (k, ga["name"], what)


# (one list, so that the cases with the rates in the call keep the names they had before there was a `capturable`)
CLIP_STEP_CASES = [pytest.param(wd, frac, cap, id="%s-%s%s" % (wd, frac, "-capturable" if cap else ""))
                   for wd in (0.0, 0.01) for frac in (None, 0.14, 1.0) for cap in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("wd,frac,capturable", CLIP_STEP_CASES)
def test_fused_step_equals_clip_then_step(wd, frac, capturable, gpu):
    """`step(max_grad_norm=1.0)` against `clip_grad_norm_(all parameters, 1.0); step()`: parameters, both moments and step counts
    bit for bit, `.grad` untouched, `last_grad_norm` the drop-in's norm -- dense and with a visibility mask, with the learning
    rates and step counts in the call and on the device (capturable: every step here is an eager one, the first included)."""
    import gftorf_amd
    a, b = _twins(gpu, 2, wd, capturable=capturable)
    vis = None if frac is None else (torch.rand(1001, generator=torch.Generator().manual_seed(99)) < frac).to(gpu)
    gen = torch.Generator().manual_seed(123)
    assert b.last_grad_norm is None
    for it in range(4):
        for ga, gb in zip(a.param_groups, b.param_groups):
            pa, pb = ga["params"][0], gb["params"][0]
            if it == 2 and ga["name"] == "3":
                pa.grad = pb.grad = None                    # a parameter without gradient is left out of norm and step
            else:
                pa.grad = torch.randn(pa.shape, generator=gen).to(gpu) * (10.0 ** (it - 2))
                pb.grad = pa.grad.clone()
        keep = [None if p.grad is None else p.grad.clone() for p in _params(b)]
        n_a = gftorf_amd.clip_grad_norm_(_params(a), 1.0)
        a.step(visibility=vis)
        b.step(visibility=vis if it % 2 == 0 or vis is None else vis.to(torch.uint8), max_grad_norm=1.0)
        assert b.last_grad_norm.shape == () and b.last_grad_norm.device == gpu
        assert torch.equal(bits(b.last_grad_norm), bits(n_a)), it
        for p, g0 in zip(_params(b), keep):
            assert (p.grad is None) == (g0 is None)
            if g0 is not None:
                assert torch.equal(bits(p.grad), bits(g0))
        _assert_same_state(a, b, "step %d" % it)
    # the norms went from below max_norm to far above it
    assert float(n_a) > 100.0


@pytest.mark.gpu
def test_fused_clip_takes_an_odd_gradient_view_once(gpu):
    """A gradient the step copies for alignment (element 1 of a two-float tensor) enters the norm as that copy."""
    import gftorf_amd
    from gftorf_amd import FusedAdam
    p = torch.nn.Parameter(torch.tensor([0.5], device=gpu))
    q = torch.nn.Parameter(torch.tensor([0.5], device=gpu))
    for cap in (False, True):
        a, b = FusedAdam([p], lr=1e-2, capturable=cap), FusedAdam([q], lr=1e-2, capturable=cap)
        for _ in range(2):
            two = torch.tensor([9.0, 4.0], device=gpu)
            p.grad, q.grad = two[1:2], torch.tensor([4.0], device=gpu)
            assert p.grad.data_ptr() % 16 == 4
            a.step(max_grad_norm=1.0)
            gftorf_amd.clip_grad_norm_([q], 1.0)
            b.step()
            assert float(a.last_grad_norm) == 4.0 and two.tolist() == [9.0, 4.0]
            assert torch.equal(bits(p), bits(q))


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fused_clip_vs_torch_clip_and_adam(wd, gpu):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU in fp32 (as test_fused_adam_vs_torch_adam compares), with
    that test's tolerance; rtol grows by twice the relative difference of the two norms, since the second moment sees the
    coefficient squared."""
    (got,) = _twins(gpu, 1, wd)
    (ref,) = _twins("cpu", 1, wd, cls=torch.optim.Adam)
    gen = torch.Generator().manual_seed(123)
    delta = 0.0
    for it in range(4):
        for gr, gg in zip(ref.param_groups, got.param_groups):
            pr, pg = gr["params"][0], gg["params"][0]
            pr.grad = torch.randn(pr.shape, generator=gen) * (10.0 ** (it - 2))
            pg.grad = pr.grad.to(gpu)
        n_ref = float(torch.nn.utils.clip_grad_norm_(_params(ref), 1.0))
        ref.step()
        got.step(max_grad_norm=1.0)
        delta = max(delta, abs(float(got.last_grad_norm) - n_ref) / n_ref)
    print("fused clip vs torch: largest relative difference of the norms %.3g" % delta)
    assert delta < 1e-5
    for gr, gg in zip(ref.param_groups, got.param_groups):
        pr, pg = gr["params"][0], gg["params"][0]
        sr, sg = ref.state[pr], got.state[pg]
        assert float(sr["step"]) == float(sg["step"]) == 4.0
        for name, a, b in (("param", pr, pg), ("exp_avg", sr["exp_avg"], sg["exp_avg"]), ("exp_avg_sq", sr["exp_avg_sq"], sg["exp_avg_sq"])):
            ref_np = a.detach().numpy()
            np.testing.assert_allclose(b.detach().cpu().numpy(), ref_np, rtol=3e-6 + 2 * delta, atol=3e-7 * float(np.abs(ref_np).max()),
                                       err_msg="%s of group %s" % (name, gr["name"]))


@pytest.mark.gpu
def test_no_host_sync(gpu):
    import gftorf_amd
    ps = scale_set(make_set("network", gpu), 40.0)
    (cap,) = _twins(gpu, 1, capturable=True)
    vis = torch.ones(1001, dtype=torch.bool, device=gpu)

    def both():
        n = gftorf_amd.clip_grad_norm_(ps, 1.0)
        cap.step(max_grad_norm=1.0)
        cap.step(visibility=vis, max_grad_norm=1.0)
        return n
    for p in _params(cap):
        p.grad = torch.ones_like(p)
    both()                                              # warm: buffers and optimizer state exist
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        n = both()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert float(n) > 0 and float(cap.last_grad_norm) > 0


def _capture(fn):
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph, out


@pytest.mark.gpu
def test_captured_clip_follows_new_gradients_and_learning_rates(gpu, monkeypatch):
    """`cap.step(max_grad_norm=1.0)` captured and replayed on new gradient values, norms alternating below and above
    max_norm, under a moving learning rate: equal to an eager non-capturable twin's `step(max_grad_norm=1.0)` bit for bit.
    Then the drop-in alone, captured."""
    import gftorf_amd
    gen = torch.Generator().manual_seed(7)
    eager, cap = _twins(gpu, 1, seed=3)[0], _twins(gpu, 1, seed=3, capturable=True)[0]
    for opt in (eager, cap):
        for g in opt.param_groups:
            g["base_lr"] = g["lr"]
            g["params"][0].grad = torch.zeros_like(g["params"][0])
    numel = sum(p.numel() for p in _params(eager))
    # 59 066 values of deviation s have a norm of about 243 s
    scale = lambda it: (0.5 if it % 2 else 3.0) / numel ** 0.5
    grads = [[torch.randn(p.shape, generator=gen).to(gpu) * scale(it) for p in _params(eager)] for it in range(6)]

    def load(opt, it):
        for g, gr in zip(opt.param_groups, grads[it]):
            g["params"][0].grad.copy_(gr)
            g["lr"] = g["base_lr"] * (0.9 ** it)
    load(eager, 0), load(cap, 0)
    eager.step(max_grad_norm=1.0), cap.step(max_grad_norm=1.0)          # the state is created outside the graph
    assert torch.equal(bits(eager.last_grad_norm), bits(cap.last_grad_norm))
    load(cap, 1)
    graph, _ = _capture(lambda: cap.step(max_grad_norm=1.0))
    norms = []
    for it in range(1, 6):
        load(eager, it)
        eager.step(max_grad_norm=1.0)
        load(cap, it)
        cap.refresh_lr()
        graph.replay()
        assert torch.equal(bits(eager.last_grad_norm), bits(cap.last_grad_norm)), it
        norms.append(float(cap.last_grad_norm))
    torch.cuda.synchronize()
    assert [n > 1.0 for n in norms] == [False, True, False, True, False], norms
    for ge, gc, gr in zip(eager.param_groups, cap.param_groups, grads[5]):
        pe, pc = ge["params"][0], gc["params"][0]
        assert float(eager.state[pe]["step"]) == float(cap.state[pc]["step"]) == 6.0
        assert torch.equal(bits(pe), bits(pc)), ge["name"]
        assert torch.equal(bits(eager.state[pe]["exp_avg_sq"]), bits(cap.state[pc]["exp_avg_sq"]))
        assert torch.equal(bits(pc.grad), bits(gr))                      # the fused form leaves .grad as it was
    # ---- the drop-in alone
    ps = scale_set(make_set("odd_views", gpu), 0.5)
    gftorf_amd.clip_grad_norm_(ps, 1.0)
    graph, n = _capture(lambda: gftorf_amd.clip_grad_norm_(ps, 1.0))
    for target in (5.0, 0.25, 40.0):
        scale_set(ps, target)
        before = [p.grad.clone() for p in ps]
        graph.replay()
        assert abs(float(n) - target) < 1e-5 * target
        c = torch.clamp(1.0 / (n + 1e-6), max=1.0)
        assert (float(c) == 1.0) == (target < 1.0)
        for p, g0 in zip(ps, before):
            assert torch.equal(bits(p.grad), bits(g0 * c))
    # error_if_nonfinite reads the norm: refused while a graph is captured (before anything is launched)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(NotImplementedError):
        gftorf_amd.clip_grad_norm_(ps, 1.0, error_if_nonfinite=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
def test_captured_step_on_visible_rows(dtype, gpu):
    """`FusedAdam(capturable=True).step(visibility=mask)`: one eager call, then the call captured; every replay follows the
    mask's contents of that replay.  Rows of the mask take exactly the dense capturable step, the other rows keep parameter
    and moments, the 7-element parameter takes the dense step, and every step count advances."""
    dense, rows = _twins(gpu, 2, seed=3, capturable=True)
    mask = torch.zeros(1001, dtype=dtype, device=gpu)
    ggen, mgen = torch.Generator().manual_seed(5), torch.Generator().manual_seed(99)
    for opt in (dense, rows):
        for p in _params(opt):
            p.grad = torch.zeros_like(p)
    graph = None
    for it, frac in enumerate((0.5, 0.0, 0.14, 1.0, 0.14)):
        mask.copy_((torch.rand(1001, generator=mgen) < frac).to(gpu))
        sel_rows = mask != 0
        assert 0 < int(sel_rows.sum()) < 1001 if 0.0 < frac < 1.0 else int(sel_rows.sum()) == 1001 * int(frac)
        for pd, pr in zip(_params(dense), _params(rows)):
            pr.grad.copy_(torch.randn(pr.shape, generator=ggen).to(gpu))
            pd.grad.copy_(pr.grad)
            # the dense optimizer starts every step from the row-wise one's state: one step is compared at a time
            pd.data.copy_(pr.data)
            if pr in rows.state:
                for k in ("step", "exp_avg", "exp_avg_sq"):
                    dense.state[pd][k].copy_(rows.state[pr][k])
        old = [(p.detach().clone(),
                rows.state[p]["exp_avg"].clone() if p in rows.state else torch.zeros_like(p),
                rows.state[p]["exp_avg_sq"].clone() if p in rows.state else torch.zeros_like(p)) for p in _params(rows)]
        dense.step()
        if it == 0:
            rows.step(visibility=mask)                   # eager, on the capturable optimizer: the state is created here
            graph, _ = _capture(lambda: rows.step(visibility=mask))
        else:
            graph.replay()
        for (p0, m0, v0), gd, gr in zip(old, dense.param_groups, rows.param_groups):
            pd, pr = gd["params"][0], gr["params"][0]
            sd, sr = dense.state[pd], rows.state[pr]
            assert sr["step"].is_cuda and float(sd["step"]) == float(sr["step"]) == it + 1, gr["name"]
            if pr.shape[0] == 1001:
                sel = sel_rows.view(-1, *([1] * (pr.dim() - 1)))
                want = (torch.where(sel, pd.detach(), p0), torch.where(sel, sd["exp_avg"], m0), torch.where(sel, sd["exp_avg_sq"], v0))
            else:
                want = (pd.detach(), sd["exp_avg"], sd["exp_avg_sq"])
                assert not torch.equal(sr["exp_avg"], m0)                 # the odd one moved
            for name, w, g in zip(("param", "exp_avg", "exp_avg_sq"), want, (pr.detach(), sr["exp_avg"], sr["exp_avg_sq"])):
                assert torch.equal(bits(w), bits(g)), "%s of group %s, step %d (%.2f of the rows)" % (name, gr["name"], it, frac)
            if pr.shape[0] == 1001 and gr["lr"] > 0 and frac > 0:
                assert not torch.equal(pr.detach(), p0), gr["name"]                 # the selected rows did move
