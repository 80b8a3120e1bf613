"""FusedAdam (optimizer part) against torch.optim.Adam, the optimizer the
reference uses (scene/gaussian_model.py:274)."""
import functools

import numpy as np
import pytest
import torch


def groups(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=g).to(dev))
    # shapes of the reference's parameter groups (xyz, f_dc, f_rest, opacity, scaling, rotation, an odd one)
    ps = [mk(1001, 3), mk(1001, 1, 3), mk(1001, 15, 3), mk(1001, 1), mk(1001, 3), mk(1001, 4), mk(7)]
    lrs = [1.6e-4, 2.5e-3, 1.25e-4, 0.05, 5e-3, 1e-3, 0.0]
    return [{"params": [p], "lr": lr, "name": str(i)} for i, (p, lr) in enumerate(zip(ps, lrs))]


def run(opt_cls, dev, steps=5, wd=0.0, **kw):
    gs = groups(dev)
    opt = opt_cls(gs, lr=0.0, eps=1e-15, weight_decay=wd, **kw)
    gen = torch.Generator().manual_seed(123)
    for it in range(steps):
        for grp in opt.param_groups:
            p = grp["params"][0]
            if it == 2 and grp["name"] == "3":
                p.grad = None                       # a parameter without gradient is skipped
            else:
                p.grad = torch.randn(p.shape, generator=gen).to(dev) * (10.0 ** (it - 2))
        opt.step()
    return opt


def test_reference_optimizer_is_deterministic_on_cpu():
    a, b = run(torch.optim.Adam, "cpu"), run(torch.optim.Adam, "cpu")
    for ga, gb in zip(a.param_groups, b.param_groups):
        assert torch.equal(ga["params"][0], gb["params"][0])


def test_fused_adam_rejects_cpu_and_unsupported_modes():
    from gftorf_amd import FusedAdam
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="HIP device only"):
        FusedAdam([p]).step()
    with pytest.raises(NotImplementedError):
        FusedAdam([p], amsgrad=True)


@pytest.mark.gpu
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_fused_adam_vs_torch_adam(wd, gpu):
    from gftorf_amd import FusedAdam
    ref = run(torch.optim.Adam, "cpu", wd=wd)
    got = run(FusedAdam, gpu, wd=wd)
    for gr, gg in zip(ref.param_groups, got.param_groups):
        pr, pg = gr["params"][0], gg["params"][0]
        sr, sg = ref.state[pr], got.state[pg]
        assert float(sr["step"]) == float(sg["step"])
        for name, a, b in (("param", pr, pg), ("exp_avg", sr["exp_avg"], sg["exp_avg"]),
                           ("exp_avg_sq", sr["exp_avg_sq"], sg["exp_avg_sq"])):
            ref_np = a.detach().numpy()
            # one rounding per operation may differ (fused multiply-adds on either side); parameters
            # near zero are the difference of larger updates, hence the absolute term
            np.testing.assert_allclose(b.detach().cpu().numpy(), ref_np, rtol=3e-6, atol=3e-7 * float(np.abs(ref_np).max()),
                                       err_msg="%s of group %s" % (name, gr["name"]))


@pytest.mark.gpu
def test_fused_adam_state_is_torch_compatible(gpu):
    """The reference's densification edits optimizer.state in place and reloads state_dicts."""
    from gftorf_amd import FusedAdam
    opt = run(FusedAdam, gpu, steps=2)
    sd = opt.state_dict()
    other = torch.optim.Adam(groups(gpu), lr=0.0, eps=1e-15)
    other.load_state_dict(sd)
    assert set(other.state[other.param_groups[0]["params"][0]].keys()) == {"step", "exp_avg", "exp_avg_sq"}


@pytest.mark.gpu
@pytest.mark.parametrize("frac", [0.0, 0.14, 1.0])
def test_step_on_visible_rows_only(frac, gpu):
    """Opt-in `step(visibility=mask)` (sparse Adam on visible Gaussians): rows of the mask take exactly
    the dense step (bit for bit), the other rows keep parameter and moments; parameters that are not per-Gaussian (the
    odd 7-element one) take the dense step."""
    from gftorf_amd import FusedAdam
    gen = torch.Generator().manual_seed(99)
    vis = (torch.rand(1001, generator=gen) < frac).to(gpu)
    dense, rows = FusedAdam(groups(gpu), lr=0.0, eps=1e-15), FusedAdam(groups(gpu), lr=0.0, eps=1e-15)
    ggen = torch.Generator().manual_seed(5)
    for it in range(4):
        for gd, gr in zip(dense.param_groups, rows.param_groups):
            pd, pr = gd["params"][0], gr["params"][0]
            pd.grad = torch.randn(pd.shape, generator=ggen).to(gpu)
            pr.grad = pd.grad.clone()
            # the dense optimizer starts every step from the row-wise one's state: one step is compared at a time
            pd.data.copy_(pr.data)
            if pr in rows.state:
                if pd not in dense.state:
                    dense.state[pd] = {"step": rows.state[pr]["step"].clone(), "exp_avg": rows.state[pr]["exp_avg"].clone(),
                                       "exp_avg_sq": rows.state[pr]["exp_avg_sq"].clone()}
                for k in ("step", "exp_avg", "exp_avg_sq"):
                    dense.state[pd][k].copy_(rows.state[pr][k])
        old = [(g["params"][0].detach().clone(),
                rows.state[g["params"][0]]["exp_avg"].clone() if g["params"][0] in rows.state else None,
                rows.state[g["params"][0]]["exp_avg_sq"].clone() if g["params"][0] in rows.state else None) for g in rows.param_groups]
        dense.step()
        rows.step(visibility=vis if it % 2 == 0 else vis.to(torch.uint8))
        for (p0, m0, v0), gd, gr in zip(old, dense.param_groups, rows.param_groups):
            pd, pr = gd["params"][0], gr["params"][0]
            sd, sr = dense.state[pd], rows.state[pr]
            assert float(sd["step"]) == float(sr["step"]) == it + 1
            m0 = torch.zeros_like(p0) if m0 is None else m0
            v0 = torch.zeros_like(p0) if v0 is None else v0
            if pr.shape[0] == 1001:
                sel = vis.view(-1, *([1] * (pr.dim() - 1)))
                want = (torch.where(sel, pd.detach(), p0), torch.where(sel, sd["exp_avg"], m0), torch.where(sel, sd["exp_avg_sq"], v0))
            else:
                want = (pd.detach(), sd["exp_avg"], sd["exp_avg_sq"])
            for name, w, g in zip(("param", "exp_avg", "exp_avg_sq"), want, (pr.detach(), sr["exp_avg"], sr["exp_avg_sq"])):
                assert torch.equal(w, g), "%s of group %s, step %d" % (name, gr["name"], it)
    with pytest.raises(RuntimeError, match="visibility"):
        rows.step(visibility=torch.zeros(1001, device=gpu))


@pytest.mark.gpu
def test_gradient_view_at_an_odd_offset_and_row_params(gpu):
    """The rasterizer returns the dc_offset gradient as element 1 of a two-float tensor (api.py: `g["offsets"][1:2]`): a
    contiguous view 4 bytes into its allocation, which autograd may adopt as `.grad`.  The step copies such a gradient
    instead of rejecting the whole table, and step counters only advance with a step that was taken.  `row_params` names
    the tensors a visibility mask applies to."""
    from gftorf_amd import FusedAdam
    p = torch.nn.Parameter(torch.tensor([0.5], device=gpu))
    q = torch.nn.Parameter(torch.tensor([0.5], device=gpu))
    two = torch.tensor([9.0, 0.25], device=gpu)
    p.grad = two[1:2]
    q.grad = torch.tensor([0.25], device=gpu)
    assert p.grad.data_ptr() % 16 == 4
    a, b = FusedAdam([p], lr=1e-2), FusedAdam([q], lr=1e-2)
    for _ in range(3):
        a.step()
        b.step()
    assert torch.equal(p.detach(), q.detach()) and float(a.state[p]["step"]) == 3.0
    # a 7-row weight is not a per-Gaussian tensor although a 7-entry mask fits it: named row parameters only
    w = torch.nn.Parameter(torch.ones(7, 3, device=gpu))
    x = torch.nn.Parameter(torch.ones(7, 3, device=gpu))
    w.grad, x.grad = torch.ones_like(w), torch.ones_like(x)
    opt = FusedAdam([w, x], lr=1e-2)
    vis = torch.tensor([1, 0, 0, 0, 0, 0, 1], dtype=torch.bool, device=gpu)
    opt.step(visibility=vis, row_params=[x])
    assert (w.detach() != 1.0).all()                                  # dense step
    assert (x.detach()[1:6] == 1.0).all() and (x.detach()[0] != 1.0).all()


@pytest.mark.gpu
def test_capturable_adam_equals_the_eager_one_and_replays(gpu):
    """FusedAdam(capturable=True): step counts and learning rates on the device.  Eager steps equal the non-capturable ones
    bit for bit (the bias corrections are the same doubles rounded once); a step captured in a graph and replayed follows
    the learning rates the scheduler writes between replays (refresh_lr) and new gradient VALUES in the static tensors."""
    from gftorf_amd import FusedAdam
    ref = run(FusedAdam, gpu, steps=5)
    got = run(FusedAdam, gpu, steps=5, capturable=True)
    for gr, gg in zip(ref.param_groups, got.param_groups):
        pr, pg = gr["params"][0], gg["params"][0]
        sr, sg = ref.state[pr], got.state[pg]
        assert sg["step"].is_cuda and float(sr["step"]) == float(sg["step"])
        for name, a, b in (("param", pr, pg), ("exp_avg", sr["exp_avg"], sg["exp_avg"]), ("exp_avg_sq", sr["exp_avg_sq"], sg["exp_avg_sq"])):
            assert torch.equal(a, b), "%s of group %s" % (name, gr["name"])
    # ---- under a graph: static gradient tensors, learning rates that move between replays
    gen = torch.Generator().manual_seed(7)
    sched = lambda it, base: base * (0.9 ** it)

    def make(capturable):
        gs = groups(gpu, seed=3)
        opt = FusedAdam(gs, lr=0.0, eps=1e-15, capturable=capturable)
        for g in opt.param_groups:
            g["base_lr"] = g["lr"]
            g["params"][0].grad = torch.zeros_like(g["params"][0])
        return opt
    eager, cap = make(False), make(True)
    grads = [[torch.randn(g["params"][0].shape, generator=gen).to(gpu) for g in eager.param_groups] for _ in range(6)]

    def load(opt, it):
        for g, gr in zip(opt.param_groups, grads[it]):
            g["params"][0].grad.copy_(gr)
            g["lr"] = sched(it, g["base_lr"])
    load(eager, 0), load(cap, 0)
    eager.step(), cap.step()                          # the state is created outside the graph
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        load(cap, 1)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            cap.step()
    torch.cuda.current_stream().wait_stream(side)
    # (the capture itself ran nothing: iteration 1 is the first replay)
    for it in range(1, 6):
        load(eager, it)
        eager.step()
        load(cap, it)
        cap.refresh_lr()
        graph.replay()
    torch.cuda.synchronize()
    for ge, gc in zip(eager.param_groups, cap.param_groups):
        pe, pc = ge["params"][0], gc["params"][0]
        assert float(eager.state[pe]["step"]) == float(cap.state[pc]["step"]) == 6.0
        assert torch.equal(pe, pc), ge["name"]
        assert torch.equal(eager.state[pe]["exp_avg_sq"], cap.state[pc]["exp_avg_sq"])


# ---- a table that crosses GFT_ADAM_MAX_TENSORS (40): 43 one-tensor groups, every one with its own learning rate, so a tensor
# that reads another one's factors, or a second launch that starts at the wrong entry, gives wrong values ------------------------
WIDE_SIZES = [0, 1, 3, 4, 5, 7, 8, 255, 256, 257, 1025, 2053]      # empty; tails of 1..3; 2053 floats = 513 16-byte groups: two
                                                                    # workgroups of the dense kernel (256 threads x 2 groups)
WIDE_ROWS = 37
WIDE_ROW_FLOATS = {5: 1, 17: 3, 29: 4, 41: 45}      # entry of the table -> floats per row of the per-row tensor there (entry 41 is
                                                    # in the second launch; 37 x 45 floats = 416 groups: two workgroups of the
                                                    # row kernel, 256 groups each)


def wide_groups(dev):
    gen = torch.Generator().manual_seed(11)
    out, dense = [], 0
    for i in range(43):
        if i in WIDE_ROW_FLOATS:
            shape = (WIDE_ROWS, WIDE_ROW_FLOATS[i])
        else:
            shape = (WIDE_SIZES[dense % len(WIDE_SIZES)],)
            dense += 1
        out.append({"params": [torch.nn.Parameter(torch.randn(*shape, generator=gen).to(dev))], "lr": 1e-3 * (1 + i), "name": str(i)})
    assert dense == 39
    return out


def wide_grads(it):
    gen = torch.Generator().manual_seed(100 + it)
    return [torch.randn(g["params"][0].shape, generator=gen) for g in wide_groups("cpu")]


def wide_steps(opt, dev, **kw):
    for it in range(3):
        for grp, g in zip(opt.param_groups, wide_grads(it)):
            grp["params"][0].grad = g.to(dev)
        opt.step(**kw)
    return opt


@functools.lru_cache(maxsize=None)
def wide_reference():
    """torch.optim.Adam on the CPU in fp32 (it steps the empty parameter too and advances its count); computed once, read only."""
    return wide_steps(torch.optim.Adam(wide_groups("cpu"), lr=0.0, eps=1e-15), "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("capturable", [False, True])
def test_table_longer_than_one_launch(capturable, gpu):
    """43 tensors in one bucket: two launches (40 + 3), the second with its own tick and its own slice of the factors.  Dense:
    three steps against torch.optim.Adam under the tolerance of test_fused_adam_vs_torch_adam, step counts equal, the empty
    tensor's included.  With a visibility mask over the four per-row tensors: selected rows equal the dense twin's step bit
    for bit, the other rows keep parameter and moments (as test_step_on_visible_rows_only asserts it), everything else takes
    the dense step."""
    from gftorf_amd import FusedAdam
    ref = wide_reference()
    got = wide_steps(FusedAdam(wide_groups(gpu), lr=0.0, eps=1e-15, capturable=capturable), gpu)
    assert len(got.param_groups) == 43
    for gr, gg in zip(ref.param_groups, got.param_groups):
        pr, pg = gr["params"][0], gg["params"][0]
        sr, sg = ref.state[pr], got.state[pg]
        assert float(sr["step"]) == float(sg["step"]) == 3.0, gr["name"]
        assert sg["step"].is_cuda == capturable
        for name, a, b in (("param", pr, pg), ("exp_avg", sr["exp_avg"], sg["exp_avg"]), ("exp_avg_sq", sr["exp_avg_sq"], sg["exp_avg_sq"])):
            ref_np = a.detach().numpy()
            assert b.shape == a.shape
            if ref_np.size:
                np.testing.assert_allclose(b.detach().cpu().numpy(), ref_np, rtol=3e-6, atol=3e-7 * float(np.abs(ref_np).max()),
                                           err_msg="%s of group %s" % (name, gr["name"]))
    # ---- the row-masked step: the four per-row tensors in one launch, the other 39 in another
    vis = (torch.rand(WIDE_ROWS, generator=torch.Generator().manual_seed(99)) < 0.5).to(gpu)
    assert 0 < int(vis.sum()) < WIDE_ROWS
    dense, rows = (FusedAdam(wide_groups(gpu), lr=0.0, eps=1e-15, capturable=capturable) for _ in range(2))
    row_params = [rows.param_groups[i]["params"][0] for i in WIDE_ROW_FLOATS]
    for it in range(3):
        for gd, gr, g in zip(dense.param_groups, rows.param_groups, wide_grads(it)):
            pd, pr = gd["params"][0], gr["params"][0]
            pd.grad = g.to(gpu)
            pr.grad = pd.grad.clone()
            # the dense optimizer starts every step from the row-wise one's state: one step is compared at a time
            pd.data.copy_(pr.data)
            if pr in rows.state:
                for k in ("step", "exp_avg", "exp_avg_sq"):
                    dense.state[pd][k].copy_(rows.state[pr][k])
        old = [(p.detach().clone(),
                rows.state[p]["exp_avg"].clone() if p in rows.state else torch.zeros_like(p),
                rows.state[p]["exp_avg_sq"].clone() if p in rows.state else torch.zeros_like(p))
               for p in (g["params"][0] for g in rows.param_groups)]
        dense.step()
        rows.step(visibility=vis, row_params=row_params)
        for i, ((p0, m0, v0), gd, gr) in enumerate(zip(old, dense.param_groups, rows.param_groups)):
            pd, pr = gd["params"][0], gr["params"][0]
            sd, sr = dense.state[pd], rows.state[pr]
            assert float(sd["step"]) == float(sr["step"]) == it + 1, gr["name"]
            if i in WIDE_ROW_FLOATS:
                sel = vis.view(-1, 1)
                want = (torch.where(sel, pd.detach(), p0), torch.where(sel, sd["exp_avg"], m0), torch.where(sel, sd["exp_avg_sq"], v0))
                assert not torch.equal(pr.detach(), p0) and torch.equal(pr.detach()[~vis], p0[~vis])
            else:
                want = (pd.detach(), sd["exp_avg"], sd["exp_avg_sq"])
            for name, w, g in zip(("param", "exp_avg", "exp_avg_sq"), want, (pr.detach(), sr["exp_avg"], sr["exp_avg_sq"])):
                assert torch.equal(w.view(torch.int32), g.view(torch.int32)), "%s of group %s, step %d" % (name, gr["name"], it)


# ---- densification re-keys the parameters: the reference replaces each nn.Parameter and hands the SAME state dict to the new
# tensor (scene/gaussian_model.py:456-540; gftorf_amd.densify does the same) --------------------------------------------------
PER_GAUSSIAN = [str(i) for i in range(6)]      # groups() names of the six [1001, ...] tensors; "6" is the odd one


def _new_rows(seed=21, rows=37):
    g = torch.Generator().manual_seed(seed)
    shapes = [(3,), (1, 3), (15, 3), (1,), (3,), (4,)]
    ext = {name: torch.randn((rows,) + s, generator=g) for name, s in zip(PER_GAUSSIAN, shapes)}
    keep = torch.rand(1001 + rows, generator=g) < 0.8
    return ext, keep


def _densify(opt, dev, ext, keep):
    """37 rows appended, then a seeded mask of rows kept: every per-Gaussian parameter is replaced twice."""
    from gftorf_amd import densify
    densify.cat_tensors_to_optimizer(opt, {k: v.to(dev) for k, v in ext.items()}, skip=("6",))
    densify.prune_optimizer(opt, keep.to(dev), skip=("6",))


def _densify_by_hand(opt, ext, keep):
    """The same surgery on a torch.optim.Adam, written out (gaussian_model.py:473-492 and 516-537)."""
    for group in opt.param_groups:
        if group["name"] not in ext:
            continue
        p = group["params"][0]
        state = opt.state.pop(p)
        new_p = torch.nn.Parameter(torch.cat((p.detach(), ext[group["name"]]), dim=0)[keep].clone())
        for k in ("exp_avg", "exp_avg_sq"):
            state[k] = torch.cat((state[k], torch.zeros_like(ext[group["name"]])), dim=0)[keep].clone()
        group["params"][0] = new_p
        opt.state[new_p] = state


def _rekey(opt, group):
    """A parameter replaced the way the densification replaces it: new tensor, same state dict."""
    p = group["params"][0]
    new_p = torch.nn.Parameter(p.detach().clone())
    state = opt.state.pop(p)
    group["params"][0] = new_p
    opt.state[new_p] = state
    return new_p


@pytest.mark.gpu
def test_capturable_adam_follows_the_schedule_after_densification(gpu):
    """Two eager steps, the densification's surgery on the optimizer, one eager step, the step captured, five replays under
    a moving learning rate: the capturable optimizer equals the eager one bit for bit and torch.optim.Adam (CPU, the same
    surgery by hand) to rounding.  The re-keyed parameters keep their state dict, so their slot in the device buffers has to
    be known from the state: refresh_lr() must reach them."""
    from gftorf_amd import FusedAdam
    ext, keep = _new_rows()
    gen = torch.Generator().manual_seed(7)

    def make(cls, dev, **kw):
        opt = cls(groups(dev, seed=3), lr=0.0, eps=1e-15, **kw)
        for g in opt.param_groups:
            g["base_lr"] = g["lr"]
        return opt
    # eager, captured, eager with the learning rate held at its capture-time value (the guard), torch on the CPU
    eager, cap, held = make(FusedAdam, gpu), make(FusedAdam, gpu, capturable=True), make(FusedAdam, gpu)
    cpu = make(torch.optim.Adam, "cpu")
    opts = [(eager, gpu), (cap, gpu), (held, gpu), (cpu, "cpu")]

    def draw():
        return [torch.randn(g["params"][0].shape, generator=gen) for g in eager.param_groups]

    def load(opt, dev, grads, lr_of):
        for g, gr in zip(opt.param_groups, grads):
            p = g["params"][0]
            if p.grad is None:
                p.grad = torch.zeros_like(p)            # (static gradient tensors: the graph reads these)
            p.grad.copy_(gr.to(dev))
            g["lr"] = lr_of(g["base_lr"])
    for _ in range(2):
        grads = draw()
        for opt, dev in opts:
            load(opt, dev, grads, lambda base: base)
            opt.step()
    for opt, dev in opts[:3]:
        _densify(opt, dev, ext, keep)
    _densify_by_hand(cpu, ext, keep)
    rows = int(keep.sum())
    assert all(g["params"][0].shape[0] == (rows if g["name"] != "6" else 7) for opt, _ in opts for g in opt.param_groups)
    grads = draw()
    for opt, dev in opts:
        load(opt, dev, grads, lambda base: base)
        opt.step()                                       # adopts the state outside the graph
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            cap.step()
    torch.cuda.current_stream().wait_stream(side)
    for it in range(1, 6):
        grads = draw()
        for opt, dev in ((eager, gpu), (cpu, "cpu")):
            load(opt, dev, grads, lambda base: base * 0.9 ** it)
            opt.step()
        load(held, gpu, grads, lambda base: base)
        held.step()
        load(cap, gpu, grads, lambda base: base * 0.9 ** it)
        cap.refresh_lr()
        graph.replay()
    torch.cuda.synchronize()
    for ge, gc, gh, gt in zip(eager.param_groups, cap.param_groups, held.param_groups, cpu.param_groups):
        pe, pc, ph, pt = (g["params"][0] for g in (ge, gc, gh, gt))
        se, sc, st = eager.state[pe], cap.state[pc], cpu.state[pt]
        assert float(se["step"]) == float(sc["step"]) == float(st["step"]) == 8.0, ge["name"]
        for name, a, b, t in (("param", pe, pc, pt), ("exp_avg", se["exp_avg"], sc["exp_avg"], st["exp_avg"]),
                              ("exp_avg_sq", se["exp_avg_sq"], sc["exp_avg_sq"], st["exp_avg_sq"])):
            assert torch.equal(a, b), "%s of group %s" % (name, ge["name"])
            ref_np = t.detach().numpy()
            np.testing.assert_allclose(b.detach().cpu().numpy(), ref_np, rtol=3e-6, atol=3e-7 * float(np.abs(ref_np).max()),
                                       err_msg="%s of group %s" % (name, ge["name"]))
        # the guard: the schedule moved the result (a replay that kept the capture-time rate would equal `held`)
        if ge["base_lr"] > 0:
            assert not torch.equal(ph, pc), ge["name"]
            assert float((ph.detach() - pc.detach()).abs().max()) > 1e-3 * ge["base_lr"], ge["name"]


@pytest.mark.gpu
def test_capturable_adam_never_hands_out_the_slot_of_a_rekeyed_parameter(gpu):
    """Eight slots.  Seven tensors step and all are re-keyed (they keep their state, so their slots); the odd one then leaves
    the optimizer -- its slot is the only dead one -- and two groups are added: the ninth tensor to ask for a slot forces the
    reclaim, which must find that dead slot and none of the re-keyed parameters'.  One more tensor does not fit."""
    from gftorf_amd import FusedAdam, densify
    opt = FusedAdam(groups(gpu), lr=1e-3, eps=1e-15, capturable=True)
    opt._SLOTS = 8
    ext, keep = _new_rows()

    def step():
        for g in opt.param_groups:
            p = g["params"][0]
            p.grad = torch.ones_like(p)
        opt.step()
    step()
    _densify(opt, gpu, ext, keep)
    _rekey(opt, opt.param_groups[6])
    buf = opt._buffers(gpu)
    assert buf["step"].numel() == 8 and buf["used"] == 7
    gone = opt.param_groups.pop(6)["params"][0]
    gone_ptr = opt.state.pop(gone)["step"].data_ptr()
    taken = {}
    for i in range(2):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(5 + i, device=gpu))], "lr": 1e-3, "name": "new%d" % i})
    for _ in range(3):
        step()
    for g in opt.param_groups:
        st = opt.state[g["params"][0]]["step"]
        assert st.data_ptr() not in taken, (g["name"], taken[st.data_ptr()])
        taken[st.data_ptr()] = g["name"]
        assert float(st) == (3.0 if g["name"].startswith("new") else 4.0), g["name"]
    assert len(taken) == 8 and taken[gone_ptr] == "new1"
    opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3, device=gpu))], "lr": 1e-3, "name": "one too many"})
    with pytest.raises(RuntimeError, match="more than 8 parameter tensors"):
        step()


@pytest.mark.gpu
def test_refresh_lr_reaches_exactly_the_slot_of_a_rekeyed_parameter(gpu):
    """After the densification re-keyed the parameters, a changed learning rate of one group changes that parameter's entry of
    the pinned buffer a captured step copies from, and no other (read on the host: no replay needed)."""
    from gftorf_amd import FusedAdam
    opt = FusedAdam(groups(gpu), lr=0.0, eps=1e-15, capturable=True)
    for g in opt.param_groups:
        p = g["params"][0]
        p.grad = torch.ones_like(p)
    opt.step()
    ext, keep = _new_rows()
    _densify(opt, gpu, ext, keep)
    _rekey(opt, opt.param_groups[6])
    buf = opt._buffers(gpu)
    lr_host = buf["lr_host"]
    opt.refresh_lr()
    assert lr_host[:7].tolist() == [g["lr"] for g in opt.param_groups] and not lr_host[7:].any()
    for i, g in enumerate(opt.param_groups):
        slot = (opt.state[g["params"][0]]["step"].data_ptr() - buf["step"].data_ptr()) // 4
        assert slot == i                                  # (slots were given out in this order by the first step)
        before = lr_host.clone()
        g["lr"] = 0.125 + i
        opt.refresh_lr()
        assert torch.nonzero(lr_host != before)[:, 0].tolist() == [slot], g["name"]
        assert float(lr_host[slot]) == 0.125 + i
