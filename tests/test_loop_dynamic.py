"""The DYNAMIC training loop across fused densification events: the deformation network's queries (DeformQuery.plan /
query_dmlp), assemble_parameters under a motion mask, the colour + ToF rasterizer call, an L1 loss, backward,
add_densification_stats, FusedAdam on the Gaussians and torch.optim.Adam on the network (train.py:164-178, 441-449,
468-474) run through the product for 26 iterations from small_scene(P=1500, 96x64), about 35 % of the Gaussians dynamic,
while four events change the model: `densify_and_prune_fused` without and with a screen-size rule (the new mask and its
DeformQuery taken from the DensifyResult), `reset_opacity(apply_mask=get_motion_mask)` and a `prune_points` of every dynamic
Gaussian, after which n = 0 and three more iterations go through the same code.  Every event changes P or the dynamic row
count n and with it what is kept from call to call: the rasterizer's pools and schedules, FusedAdam's slots, every captured
graph, the network's `_save_state` (sized by the rows of the last call), the capacity of the backward over the rows that
count (K * n), the rank tensor a DensifyResult hands to DeformQuery.from_rank.

TEACHER FORCING, as in tests/test_loop_densify.py: one trajectory, the product's; each checked step is compared with an
independent reference evaluated on the product's own state just before it -- the network's float64 oracle on a snapshot of
the weights, the eager assembly with the mask and the oracle's offsets, the C oracle of the rasterizer, its gradients pushed
back through CPU autograd and through the network's written-out adjoint.

Schedules: "ftorf" alternates an integer frame (K = 1) with a frame between two (K = 2, the lerp of train.py:176), d_sh
unused; "torf" is query_dmlp with d_sh and gradients into the r / g / b heads.  Modes: "eager" and "graph" (two eager
iterations per shape, then one whole-iteration capture; the times and the coefficients are device tensors rewritten before
every replay.  A graph holds one K, so a replay on an integer frame of "ftorf" is the K = 2 query under the coefficients
(1, 0): the zero coefficient's block is neither read nor given a gradient).

Two things are set up so that the loop reaches the code it is about at 500-2000 network rows: `deform._SPARSE_MIN_POINTS`
is lowered to 1 for the test (a real run has 10^5 rows and is above the product's 8192 throughout), so the eager backward
counts its rows on the device and a captured one runs over the rows that count; and the phase whose statistics take
`apply_mask=get_motion_mask` renders the dynamic region alone, as train.py:446-447 does -- the reference's masked branch
(gaussian_model.py:652-654) is only defined when every visible Gaussian is inside the mask.

The SH degree is the constant 3 here (_Loop's `degrees`); tests/test_loop_sh_degree.py runs the "torf" loop while it rises.

With no dynamic row the query does not run the network: its parameters get no gradient and its optimizer takes no step
(gftorf_amd/query.py).

The network's gradient is discontinuous where a pre-activation crosses zero; about one of the 10^6 units of a step lies
within 1e-6 of it and then moves a bias gradient by 3e-3 .. 8e-3 of its max-norm, whichever arithmetic decides.  Where a step
misses the bound, network_reference takes such units on the side the product is closer to and nothing else.

Observed maxima on an MI355X over both modes and both schedules (the test prints them per checked step and per run):
d_xyz blocks, combination and d_sh 1.1e-6 of the max-norm (bound 3e-6); colour / phasor mae 8.8e-8 / 6.1e-8 (1e-5);
Gaussian gradients and ssp 5.8e-5 (1e-3); network gradients 1e-6 .. 1e-5 on most steps, 7e-4 .. 1.8e-3 where a ReLU edge
below the bound is in play (2e-3), K = 1 and K = 2 alike; statistics, event snapshots, masks and ranks bit for bit.

CPU tests: composed_reference_dynamic under an all-false mask against composed_reference; its assembly against a per-row
loop; the model's mask property on rows exactly on the threshold; the frame schedule; the network oracle's ReLU edges."""
import types

import numpy as np
import pytest
import torch

from oracle import assemble_ref, deform_ref, densify_ref
from tests import helpers, loop_densify as L

EVENTS = {6: "densify", 12: "reset_dynamic", 17: "densify_screen", 23: "prune_dynamic"}          # after this iteration: the event
ITERATIONS = 26
EAGER_FIRST = 2           # graph mode: iterations of a shape that run eagerly before it is captured
TOTAL_VIEWS = 45          # frames 0..44: the integer frames are the multiples of 4
EXTENT = 3.7              # scene_extent; its fp32 reciprocal is inexact (tests/test_query.py)
NET_LR = 1e-4             # tests/test_train_step.py
FWD_TOL = 3e-6            # tests/test_deform.py::test_forward_against_oracle, of the max-norm
NET_TOL = 2e-3            # tests/test_train_step.py: the network's gradients through rasterizer and assembly
RELU_EDGE = 1e-6          # tests/test_deform.py: a pre-activation nearer to zero than this may switch the other way in fp32
# the phase after each event: the regions rendered and whether the statistics take the motion mask (train.py:444-449)
PHASES = {"start": (("static", "dynamic"), False), "densify": (("dynamic",), True), "reset_dynamic": (("static", "dynamic"), False),
          "densify_screen": (("static", "dynamic"), False), "prune_dynamic": (("static", "dynamic"), False)}
API_FLAGS = ("no_host_read", "_GRADS_REUSE", "_GRADS_CHECK", "_ACC_REUSE", "_TILE_HINTS", "_TILE_HINTS_PER_CAMERA", "_CELL_SCHED",
             "_FWD_ORDER", "_force_cell_sched", "_force_whole_lists", "_DETERMINISTIC", "keep_last_buffers")
RGB = tuple(h + s for h in ("r", "g", "b") for s in (".weight", ".bias"))
NEVER = tuple(h + s for h in deform_ref.UNUSED for s in (".weight", ".bias"))


def frame_of(it):
    """The frame of iteration `it`: even iterations sit on an integer frame, odd ones 1-3 frames past one."""
    base = 4 * ((it // 2) % (TOTAL_VIEWS // 4))
    return base if it % 2 == 0 else base + 1 + (it // 2) % 3


def schedule_of(schedule, it, K=None):
    """(times, combine) of iteration `it`: "ftorf" from query.ftorf_schedule (with `K` = 2 an integer frame is widened to the
    next integer frame under a zero coefficient: what a graph captured with two times replays); "torf": one time, no matrix."""
    from gftorf_amd import ftorf_schedule
    if schedule == "torf":
        return [((it * 7) % TOTAL_VIEWS) / (TOTAL_VIEWS - 1)], None
    times, combine, names = ftorf_schedule(frame_of(it), TOTAL_VIEWS)
    assert names == ("d_xyz",)
    if K == 2 and len(times) == 1:
        times, combine = times + [(frame_of(it) + 4) / (TOTAL_VIEWS - 1)], [[1.0, 0.0]]
    return times, combine


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def _cpu_case(P, seed=7):
    scene = helpers.small_scene(P=P, W=48, H=32, seed=seed)
    pc = L.make_model(scene["gaussians"], "cpu", cls=L.DynamicGaussians, optimizer_cls=torch.optim.Adam)
    raw = {n: getattr(pc, L.ATTR[n]).detach() for n in L.NAMES}
    rng = np.random.default_rng(seed)
    up_c, up_p = ((rng.normal(size=scene["grads"][k].shape) * 1e-3).astype(np.float32) for k in ("color", "phasor"))
    return scene, raw, up_c, up_p, rng


def test_all_false_mask_is_the_static_reference(oracle):
    scene, raw, up_c, up_p, _ = _cpu_case(200)
    f0, g0 = L.composed_reference(oracle, scene, raw, up_c, up_p)
    f1, g1 = L.composed_reference_dynamic(oracle, scene, raw, torch.zeros(200, dtype=torch.bool), np.zeros((0, 3), np.float32),
                                          np.zeros((0, 16, 3), np.float32), up_c, up_p)
    assert int((np.asarray(f0.radii) > 0).sum()) > 50 and np.abs(g0["xyz"]).max() > 0
    for k in ("color", "phasor"):
        np.testing.assert_array_equal(f1[k], f0[k])
    np.testing.assert_array_equal(np.asarray(f1.radii), np.asarray(f0.radii))
    assert set(g1) == set(g0) | {"d_xyz", "d_sh"} and g1["d_xyz"].shape == (0, 3)
    for k in g0:
        np.testing.assert_array_equal(g1[k], g0[k], err_msg=k)


@pytest.mark.parametrize("regions", [("static", "dynamic"), ("dynamic",)])
def test_dynamic_assembly_matches_the_per_row_loop(regions):
    """dynamic_inputs (the eager statements over pc.get_*) against gaussian_renderer/__init__.py:91-105 one Gaussian and one
    coefficient at a time in float64 (assemble_ref.parameters_loops): what is copied or added once agrees to a float32
    rounding of the sum, the activations to a few float32 roundings; and the offsets' gradient is the dynamic rows'."""
    P = 60
    scene, raw, _, _, rng = _cpu_case(P)
    mask = rng.random(P) < 0.4
    mask[:2] = (True, False)
    n = int(mask.sum())
    d_xyz, d_sh = rng.normal(0, 0.05, (n, 3)).astype(np.float32), rng.normal(0, 0.05, (n, 16, 3)).astype(np.float32)
    a, cl = L.dynamic_inputs(raw, mask, d_xyz, d_sh, regions)
    r64 = {k: v.numpy().astype(np.float64) for k, v in raw.items()}
    want = assemble_ref.parameters_loops(r64["xyz"], np.zeros((P, 3)), r64["opacity"], r64["scaling"], r64["rotation"], r64["f_dc_color"],
                                         r64["f_rest_color"], r64["phase_f_dc"], r64["phase_f_rest"], r64["amp_f_dc"], r64["amp_f_rest"],
                                         mask, d_xyz.astype(np.float64), 0.0, d_sh.astype(np.float64), 0.0, regions)
    for got, ref, name in zip(a, want, ("means3D", "means2D", "opacity", "scales", "rotations", "shs", "shs_p")):
        np.testing.assert_allclose(got.detach().numpy(), ref, rtol=4 * 2.0 ** -24, atol=1e-30, err_msg=name)
        if regions == ("dynamic",):
            assert not got.detach().numpy()[~mask].any(), name
    assert np.abs(a[0].detach().numpy()[mask] - raw["xyz"].numpy()[mask]).max() > 0.01          # the offsets are in
    w = torch.tensor(rng.normal(size=(P, 3)).astype(np.float32))
    ws = torch.tensor(rng.normal(size=(P, 16, 3)).astype(np.float32))
    ((a[0] * w).sum() + (a[5] * ws).sum()).backward()
    assert torch.equal(cl["d_xyz"].grad, w[torch.tensor(mask)]) and torch.equal(cl["d_sh"].grad, ws[torch.tensor(mask)])
    assert torch.equal(cl["xyz"].grad[torch.tensor(mask)], w[torch.tensor(mask)])
    assert bool((cl["xyz"].grad[torch.tensor(~mask)] == (w[torch.tensor(~mask)] if "static" in regions else 0)).all())


def test_motion_mask_property_on_the_threshold_rows():
    P, rows = 1500, (3, 40, 41, 700)
    scene = helpers.small_scene(P=P, W=48, H=32, seed=7)
    pc = L.make_model(scene["gaussians"], "cpu", cls=L.DynamicGaussians, optimizer_cls=torch.optim.Adam)
    assert not pc.get_motion_mask.any()                                       # a scene's model starts static
    seg = L.seg_colors(P, on_threshold=rows)
    with torch.no_grad():
        pc._features_seg_color.copy_(seg)
    mask = pc.get_motion_mask
    assert mask.dtype == torch.bool and mask.shape == (P,) and not mask.requires_grad and pc._features_seg_color.requires_grad
    assert torch.equal(mask, pc._features_seg_color[:, 0] > 0.5)              # scene/gaussian_model.py:160-161
    assert bool((seg[list(rows), 0] == 0.5).all()) and not mask[list(rows)].any()
    assert 0.3 * P < int(mask.sum()) < 0.4 * P
    assert isinstance(pc.twin(), L.DynamicGaussians) and torch.equal(pc.twin().get_motion_mask, mask)


def test_frames_alternate_between_one_and_two_times():
    for it in range(1, ITERATIONS + 1):
        times, combine = schedule_of("ftorf", it)
        assert len(times) == (1 if it % 2 == 0 else 2) and len(combine) == 1 and len(combine[0]) == len(times)
        assert all(0.0 <= t <= 1.0 for t in times) and sum(combine[0]) == pytest.approx(1.0) and min(combine[0]) > 0
        t2, c2 = schedule_of("ftorf", it, K=2)
        assert len(t2) == 2 and t2[0] == times[0] and (c2 == combine if it % 2 else c2 == [[1.0, 0.0]])
        (t,), none = schedule_of("torf", it)
        assert none is None and 0.0 <= t <= 1.0
    assert len({schedule_of("torf", it)[0][0] for it in range(1, ITERATIONS + 1)}) == ITERATIONS


def test_a_relu_edge_is_one_points_term_of_every_sum():
    """What network_reference relies on: the adjoint with one unit's ReLU taken on its other side differs from the adjoint as
    it stands by that point's own term, and relu_edges finds exactly the units relu_margin speaks of."""
    params = deform_ref.random_params(31, head_std=0.01)
    rng = np.random.default_rng(2)
    x, t = rng.random((40, 3)).astype(np.float32), rng.random((40, 1)).astype(np.float32)
    g_dxyz, g_dsh = rng.normal(size=(40, 3)), rng.normal(size=(40, 16, 3))
    eps = 2e-4
    edges = deform_ref.relu_edges(params, x, t, eps)
    margin = deform_ref.relu_margin(params, x, t)
    assert edges and {r for _, r, _ in edges} == set(np.nonzero(margin < eps)[0].tolist())
    assert not deform_ref.relu_edges(params, x, t, margin.min())
    base = deform_ref.backward(params, x, t, g_dxyz, g_dsh, dtype=np.float64)
    i, r, u = edges[0]
    flipped = deform_ref.backward(params, x, t, g_dxyz, g_dsh, dtype=np.float64, flip=[(i, r, u)])
    one = lambda flip: deform_ref.backward(params, x[r:r + 1], t[r:r + 1], g_dxyz[r:r + 1], g_dsh[r:r + 1], dtype=np.float64, flip=flip)
    there, here = one([(i, 0, u)]), one([])
    assert np.abs(flipped["linear.%d.bias" % i] - base["linear.%d.bias" % i]).max() > 0
    for k, v in base.items():
        if v is None:
            assert flipped[k] is None
        else:
            np.testing.assert_allclose(flipped[k], v + there[k] - here[k], rtol=0, atol=1e-12 * max(1.0, np.abs(v).max()), err_msg=k)
            if k.startswith("linear.") and int(k.split(".")[1]) > i:
                np.testing.assert_array_equal(flipped[k], v, err_msg=k)           # layers behind the unit do not see it
    got = {k: v for k, v in flipped.items() if v is not None}
    assert max(L.rel(got[k], base[k]) for k in got) >= NET_TOL                   # one unit of one point in forty: a miss
    ref, flips = network_reference(params, x, t, g_dxyz, g_dsh, got, eps)
    assert flips == [(i, r, u)] and all(L.rel(got[k], ref[k]) < 1e-9 for k in got)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def network_state(net, opt):
    """L.optimizer_state's form for the network: parameter name -> dict(param, exp_avg, exp_avg_sq, step), on the CPU."""
    out = {}
    for name, p in net.named_parameters():
        st = opt.state.get(p, None)
        has = st is not None and "exp_avg" in st
        out[name] = dict(param=p.detach().cpu().clone(), exp_avg=st["exp_avg"].cpu().clone() if has else None,
                         exp_avg_sq=st["exp_avg_sq"].cpu().clone() if has else None, step=float(st["step"]) if has else None)
    return out


def network_reference(params, X, T, g_dxyz, g_dsh, got, eps=RELU_EDGE):
    """The float64 adjoint of the network under the upstream gradients `g_dxyz` / `g_dsh`.  The gradient is discontinuous
    where a pre-activation crosses zero, and a unit within rounding of zero may fall on either side in another arithmetic
    (tests/test_deform.py chooses its points away from such edges; a training loop cannot).  So where the product's
    gradients `got` miss the bound, each unit within `eps` of zero is tried on its other side -- a point is one term of
    every sum, so that point's adjoint alone gives the difference -- and kept there if the product is closer to that side.
    Returns (gradients, the units taken on the other side); every other unit of every point is held to the float64 adjoint."""
    ref = deform_ref.backward(params, X, T, g_dxyz, g_dsh, dtype=np.float64)
    worst = lambda o: max(L.rel(got[k], o[k]) for k in got)
    flips = []
    if worst(ref) >= NET_TOL:
        for i, r, u in deform_ref.relu_edges(params, X, T, eps):
            one = lambda flip: deform_ref.backward(params, X[r:r + 1], T[r:r + 1], g_dxyz[r:r + 1], g_dsh[r:r + 1], dtype=np.float64, flip=flip)
            there, here = one(((i, 0, u),)), one(())
            other = {k: None if v is None else v + there[k] - here[k] for k, v in ref.items()}
            if worst(other) < worst(ref):
                ref, flips = other, flips + [(i, r, u)]
    return ref, flips


class _Loop:
    """The loop of one mode and schedule: model, network, optimizers, target, the iteration (eager or captured per shape and
    SH degree), the events, the checks.  `degrees`: iteration -> active SH degree (oneupSHdegree's schedule, train.py); None:
    3 throughout."""

    def __init__(self, mode, schedule, dev, oracle, degrees=None):
        from gftorf_amd import DeformQuery, FusedAdam, reference_network
        self.mode, self.schedule, self.dev, self.oracle = mode, schedule, dev, oracle
        self.scene = helpers.small_scene(P=1500, W=96, H=64, seed=33)
        self.degrees = degrees if degrees is not None else (lambda it: self.scene["cfg"]["D"])
        self.D, self.rasts = self.scene["cfg"]["D"], {}
        g = self.scene["gaussians"]
        t32 = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
        with torch.no_grad():            # the target: a render of the unperturbed, undeformed scene
            out = self.render(t32(g["means3D"]), torch.zeros((1500, 3), device=dev), t32(g["opacities"]).reshape(1500, 1),
                              t32(g["shs"]), t32(g["shs_p"]), t32(g["scales"]), t32(g["rotations"]))
            self.target = dict(color=out[0].clone(), phasor=out[1].clone())
        self.target_np = {k: v.cpu().numpy() for k, v in self.target.items()}
        self.pc = pc = L.make_model(g, dev, FusedAdam, cls=L.DynamicGaussians, capturable=(mode == "graph"))
        with torch.no_grad():
            pc._features_seg_color.copy_(L.seg_colors(1500).to(dev))
        self.params0 = deform_ref.random_params(31, head_std=0.01)
        self.net = reference_network()
        self.net.load_state_dict({k: torch.tensor(v) for k, v in self.params0.items()})
        self.net = self.net.to(dev)
        self.opt_net = torch.optim.Adam(self.net.parameters(), lr=NET_LR, eps=1e-15, capturable=(mode == "graph"))
        pc.scene_extent, pc.deform_model = EXTENT, types.SimpleNamespace(deform=self.net)          # what query_dmlp reads
        self.it, self.net_steps, self.phase = 0, 0, "start"
        self.maxima = {}
        self.new_shape(DeformQuery(pc.get_motion_mask.contiguous()))

    def rasterizer(self, D):
        """One GaussianRasterizer per degree, its settings carrying that degree."""
        from gftorf_amd import GaussianRasterizer
        if D not in self.rasts:
            self.rasts[D] = GaussianRasterizer(raster_settings=helpers.gpu_settings(self.scene, self.dev, sh_degree=D))
        return self.rasts[D]

    def render(self, m3, m2, op, shs, shp, sc, ro):
        return self.rasterizer(self.D)(means3D=m3, means2D=m2, opacities=op, shs=shs, shs_p=shp, scales=sc, rotations=ro,
                                       phase_offset=self.scene["phase_offset"], dc_offset=self.scene["dc_offset"])

    def new_shape(self, q):
        """After an event: the query of the new mask; nothing else of the old shape is kept -- the graphs (one per degree),
        their static tensors, the screen-space leaf.  `in_shape` counts the iterations of the shape at the degree in use."""
        self.q, self.mask = q, q.motion_mask
        self.P, self.n = self.pc._xyz.shape[0], q.n
        assert q.P == self.P
        self.ssp = torch.zeros((self.P, 3), device=self.dev, requires_grad=True)
        self.in_shape, self.graphs = 0, {}
        K = 2 if self.schedule == "ftorf" else 1
        self.times_dev = torch.zeros((K,), device=self.dev)
        self.combine_dev = torch.zeros((1, K), device=self.dev)

    def expected_net_grads(self):
        if self.n == 0:
            return set()
        return set(self.params0) - set(NEVER) - (set(RGB) if self.schedule == "ftorf" else set())

    def body(self, times, combine):
        """The device work of one iteration; what the checks read is copied before the gradients are dropped -- inside a
        capture into tensors of the graph's pool, which every replay rewrites."""
        from gftorf_amd import assemble_parameters, deform, densify, query_dmlp
        pc, ssp, net = self.pc, self.ssp, self.net
        regions, masked_stats = PHASES[self.phase]
        ssp.grad = None
        if self.schedule == "ftorf":
            (d_xyz,), d_sh = self.q.plan(net, pc._xyz, pc.scene_extent, times, combine)
            assert d_sh is None
            d_rot, d_sh, d_sh_p = 0.0, 0.0, 0.0
        else:
            d_xyz, d_rot, d_sh, d_sh_p = query_dmlp(pc, times, plan=self.q)
        m3, m2, op, sc, ro, shs, shp = assemble_parameters(
            pc._xyz, ssp, pc._opacity, pc._scaling, pc._rotation, pc._features_dc_color, pc._features_rest_color,
            pc._features_dc_phase, pc._features_rest_phase, pc._features_dc_amp, pc._features_rest_amp, self.mask,
            d_xyz, d_rot, d_sh, d_sh_p, render_regions=regions)
        out = self.render(m3, m2, op, shs, shp, sc, ro)
        color, phasor, pixels, radii = out[0], out[1], out[8], out[10]
        loss = (color - self.target["color"]).abs().mean() + (phasor - self.target["phasor"]).abs().mean() * 0.5
        loss.backward()
        with torch.no_grad():
            kept = dict(recomputed=bool(deform.last_backward_stats["recomputed"]) and self.n > 0,
                        color=color.detach().clone(), phasor=phasor.detach().clone(), pixels=pixels.detach().clone(),
                        radii=radii.clone(), ssp=ssp.grad.clone(), loss=loss.detach().clone(), d_xyz=d_xyz.detach().clone(),
                        d_sh=d_sh.detach().clone() if isinstance(d_sh, torch.Tensor) else None,
                        grads={n: getattr(pc, L.ATTR[n]).grad.clone() for n in L.NAMES if getattr(pc, L.ATTR[n]).grad is not None},
                        net_grads={n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
            densify.add_densification_stats(pc.xyz_gradient_accum, pc.denom, pc.max_radii2D, ssp.grad, radii > 0, pixels, radii,
                                            apply_mask=self.mask if masked_stats else None)
            pc.optimizer.step()
            self.opt_net.step()
            pc.optimizer.zero_grad(set_to_none=True)
            self.opt_net.zero_grad(set_to_none=True)
        ssp.grad = None
        return kept

    def iteration(self, checked):
        pc = self.pc
        self.next_degree()
        self.it += 1
        for grp in pc.optimizer.param_groups:                                  # gaussian_model.py:294-310
            if grp["name"] == "xyz":
                grp["lr"] = L.xyz_lr(self.it)
        lrs = {g["name"]: g["lr"] for g in pc.optimizer.param_groups}
        replay = self.mode == "graph" and self.in_shape >= EAGER_FIRST
        times, combine = schedule_of(self.schedule, self.it, K=2 if replay else None)
        t_dev = torch.tensor(times, dtype=torch.float32, device=self.dev)
        before, net_before = L.optimizer_state(pc), network_state(self.net, self.opt_net)          # clones, outside the graph
        stats = [t.cpu().clone() for t in (pc.xyz_gradient_accum, pc.denom, pc.max_radii2D)]
        probe = self.probe(times, t_dev if replay else times) if checked else None
        if not replay:
            kept = self.body(times if self.schedule == "ftorf" else times[0], combine)
        else:
            if self.D not in self.graphs:
                # torch's recipe for a whole-iteration capture: eager iterations first, no gradient tensor alive
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    static = self.body(self.times_dev, self.combine_dev if combine is not None else None)
                self.graphs[self.D] = (graph, static)      # (the capture ran nothing: this iteration is the first replay)
            self.times_dev.copy_(t_dev)
            if combine is not None:
                self.combine_dev.copy_(torch.tensor(combine, dtype=torch.float32, device=self.dev))
            pc.optimizer.refresh_lr()
            graph, kept = self.graphs[self.D]
            graph.replay()
        self.in_shape += 1
        torch.cuda.synchronize()
        what = "iteration %d (P = %d, n = %d, K = %d, D = %d, %s %s%s)" % (self.it, self.P, self.n, len(times), self.D, self.schedule,
                                                                          self.mode, ", replay" if replay else "")
        after = L.optimizer_state(pc)
        L.assert_adam_step(before, kept["grads"], lrs, after, what)
        assert set(kept["grads"]) == set(L.NAMES) - {"f_seg_color"}, what
        assert np.isfinite(float(kept["loss"])), what
        # the network: exactly the expected parameters have a gradient, and its Adam step is the CPU twin's
        net_grads = {k: v.cpu() for k, v in kept["net_grads"].items()}
        assert set(net_grads) == self.expected_net_grads(), (what, sorted(set(net_grads) ^ self.expected_net_grads()))
        net_after = network_state(self.net, self.opt_net)
        L.assert_adam_step(net_before, net_grads, {k: NET_LR for k in net_before}, net_after, what + " network")
        self.net_steps += self.n > 0
        self.every_iteration(before, kept, after, net_grads, net_after, what)
        if checked:
            self.check(before, net_before, stats, probe, kept, times, combine, what)
        return replay

    def next_degree(self):
        """The degree of the next iteration (oneupSHdegree): a degree step begins a new phase of the shape -- `in_shape` starts
        again; the shape stays, and so do the graphs of its earlier degrees.  Returns the degree."""
        D = self.degrees(self.it + 1)
        if D != self.D:
            self.D, self.in_shape = D, 0
        return D

    def every_iteration(self, before, kept, after, net_grads, net_after, what):
        """Further checks of every iteration (tests/test_loop_sh_degree.py)."""

    def checked_step(self, before, kept, f, ref, what):
        """Further checks of a checked step (from the state `before`) against the composed reference's forward `f` and
        gradients `ref`."""

    def probe(self, times, times_arg):
        """Before a checked step, on the weights the step will use: the query's inputs and the K d_xyz blocks themselves (the
        iteration only sees their combination)."""
        pc = self.pc
        x, t = self.q.inputs(pc._xyz, pc.scene_extent, times_arg)
        with torch.no_grad():
            blocks, _ = self.q.plan(self.net, pc._xyz, pc.scene_extent, times_arg)
            want_x = (pc._xyz.detach() / pc.scene_extent)[pc.get_motion_mask].repeat(len(times), 1)       # get_xyz_normalized[mask]
            want_t = torch.tensor(times, dtype=torch.float32, device=self.dev).repeat_interleave(self.n)
        assert x.shape == want_x.shape and torch.equal(x, want_x) and t.shape == want_t.shape and torch.equal(t, want_t)
        assert len(blocks) == len(times) and all(b.shape == (self.n, 3) for b in blocks)
        return dict(x=x.cpu().numpy(), t=t.cpu().numpy(), blocks=[b.cpu().numpy() for b in blocks])

    def note(self, key, value):
        self.maxima[key] = max(self.maxima.get(key, 0.0), float(value))

    def check(self, before, net_before, stats, probe, kept, times, combine, what):
        K, n = len(times), self.n
        regions, masked_stats = PHASES[self.phase]
        mask = self.mask.cpu()
        params = {k: v["param"].numpy() for k, v in net_before.items()}
        coeff = [1.0] if combine is None else combine[0]
        torf = self.schedule == "torf"
        # ---- the network's outputs against its float64 oracle on the weights before the step
        X, T = probe["x"], probe["t"].reshape(-1, 1)
        o_dxyz, _, o_dsh, _ = deform_ref.forward(params, X, T, dtype=np.float64)
        o_blocks = o_dxyz.reshape(K, n, 3)
        o_comb = sum(c * b for c, b in zip(coeff, o_blocks))
        o_sh = o_dsh[:n] if torf else None
        if n:
            for k in range(K):
                self.note("d_xyz block", L.rel(probe["blocks"][k], o_blocks[k]))
                assert L.rel(probe["blocks"][k], o_blocks[k]) < FWD_TOL, (what, k, L.rel(probe["blocks"][k], o_blocks[k]))
            e_comb = L.rel(kept["d_xyz"].cpu().numpy(), o_comb)
            self.note("d_xyz", e_comb)
            assert e_comb < FWD_TOL, (what, e_comb)
            if torf:
                e_sh = L.rel(kept["d_sh"].cpu().numpy(), o_sh)
                self.note("d_sh", e_sh)
                assert e_sh < FWD_TOL, (what, e_sh)
            assert np.abs(kept["d_xyz"].cpu().numpy()).max() > 0, what
        else:
            assert kept["d_xyz"].shape == (0, 3) and (kept["d_sh"] is None or kept["d_sh"].shape == (0, 16, 3)), what
        # ---- render and Gaussian gradients against the composed reference
        color, phasor = kept["color"].cpu().numpy(), kept["phasor"].cpu().numpy()
        up_c = L.l1_upstream(color, self.target_np["color"], 1.0)
        up_p = L.l1_upstream(phasor, self.target_np["phasor"], 0.5)
        scene = dict(self.scene, cfg=dict(self.scene["cfg"], D=self.D))          # (cfg["D"]: what helpers.run_oracle hands the oracle)
        f, ref = L.composed_reference_dynamic(self.oracle, scene, {k: before[k]["param"] for k in L.NAMES}, mask, o_comb, o_sh,
                                              up_c, up_p, regions)
        mae_c = float(np.abs(color - f["color"]).mean())
        mae_p = float(np.abs(phasor - f["phasor"]).mean()) / max(1.0, float(np.abs(f["phasor"]).max()))
        rels = {k: L.rel(kept["grads"][k].cpu().numpy(), ref[k]) for k in kept["grads"]}
        rels["ssp"] = L.rel(kept["ssp"].cpu().numpy(), ref["ssp"])
        assert mae_c < 1e-5 and mae_p < 1e-5, (what, mae_c, mae_p)
        visible = kept["radii"].cpu().numpy() > 0
        assert np.array_equal(visible, np.asarray(f.radii) > 0), what
        for k, v in rels.items():
            assert v < 1e-3, (what, k, v)
        assert int(visible.sum()) > 100 and np.abs(ref["xyz"]).max() > 0, what
        assert n == 0 or int((visible & mask.numpy()).sum()) >= 30, what
        self.checked_step(before, kept, f, ref, what)
        # ---- the network's gradients: the oracle's gradient on its offsets, through the coefficients and the written-out adjoint
        net_rels = {}
        if n:
            g_dxyz = np.concatenate([c * ref["d_xyz"].astype(np.float64) for c in coeff])
            g_dsh = np.zeros((K * n, 16, 3))
            if torf:
                g_dsh[:n] = ref["d_sh"]
            got = {name: kept["net_grads"][name].cpu().numpy() for name in self.expected_net_grads()}
            o_net, flips = network_reference(params, X, T, g_dxyz, g_dsh, got)
            net_rels = {name: L.rel(got[name], o_net[name]) for name in sorted(got)}
            assert all(o_net[name] is None for name in NEVER)
            assert any(kept["net_grads"]["linear.%d.weight" % i].any() for i in range(deform_ref.D)), what
        print("%s: colour mae %.3g, phasor mae %.3g, gradients %s, network %.3g (%s; %s%s)"
              % (what, mae_c, mae_p, {k: float("%.3g" % v) for k, v in rels.items()}, max(net_rels.values(), default=0.0),
                 max(net_rels, key=net_rels.get, default="-"), "rows recomputed" if kept["recomputed"] else "saved activations",
                 "; ReLU edges taken on the other side: %s" % (flips,) if n and flips else ""))
        self.note("colour mae", mae_c), self.note("phasor mae", mae_p)
        self.note("gaussian gradients", max(rels.values())), self.note("network gradients K=%d" % K, max(net_rels.values(), default=0.0))
        for name, v in net_rels.items():
            assert v < NET_TOL, (what, name, v)
        # ---- the statistics, bit for bit
        acc, den, mr = stats
        densify_ref.add_densification_stats_eager(acc, den, mr, kept["ssp"].cpu(), (kept["radii"] > 0).cpu(), kept["pixels"].cpu(),
                                                  kept["radii"].cpu(), apply_mask=mask if masked_stats else None)
        pc = self.pc
        for name, got, want in (("xyz_gradient_accum", pc.xyz_gradient_accum, acc), ("denom", pc.denom, den), ("max_radii2D", pc.max_radii2D, mr)):
            assert torch.equal(got.cpu(), want), (what, name)

    def event(self, kind):
        """The product's function on the model, the reference's statements on a twin made just before, same generator state:
        the snapshots agree key for key, bit for bit; the mask, the handed-over query and the network across the event."""
        from gftorf_amd import DeformQuery, densify
        pc = self.pc
        tw = pc.twin()
        L.assert_same_snapshot(pc, tw, "twin before " + kind)
        net_before = network_state(self.net, self.opt_net)
        mask0 = pc.get_motion_mask.clone()
        P0, n0, seed, what = self.P, self.n, 1000 + self.it, "%s after iteration %d" % (kind, self.it)
        assert int(mask0.sum()) == n0, what
        if kind in ("densify", "densify_screen"):
            th = L.thresholds(pc)
            clone, split, _ = L.selections(pc, th)
            size = 20 if kind == "densify_screen" else None
            torch.manual_seed(seed)
            tw.densify_and_prune(th["max_grad"], th["min_opacity"], th["extent"], size)
            torch.manual_seed(seed)
            res = densify.densify_and_prune_fused(pc, th["max_grad"], th["min_opacity"], th["extent"], size)
            mask1 = pc.get_motion_mask
            P1, n1 = pc._xyz.shape[0], int(mask1.sum())
            assert (res.P_before, res.P) == (P0, P1) and res.cloned == int(clone.sum()) and res.split == int(split.sum()), what
            assert res.cloned >= 1 and res.split >= 1 and res.pruned >= 1, (what, res.cloned, res.split, res.pruned)
            assert P1 != P0 and n1 != n0 and 0 < n1 < P1, (what, P0, P1, n0, n1)
            assert res.motion_mask.dtype == torch.bool and torch.equal(res.motion_mask, mask1), what
            q, fresh = res.deform_query(), DeformQuery(mask1.contiguous())
            assert (q.n, q.P) == (fresh.n, fresh.P) == (n1, P1), what
            assert torch.equal(q.rank, fresh.rank) and torch.equal(q.count, fresh.count), what
            # every kept row, clone and child is what its source row was: dynamic parents have dynamic children, static static
            src, new = res.source_row.long(), res.kind != 0
            assert torch.equal(mask1, mask0[src]), what
            if kind == "densify":         # (its statistics are those of both regions: both classes were cloned and split)
                for kd in (1, 2):
                    of_kind = mask0[src[res.kind == kd]]
                    assert bool(of_kind.any()) and not bool(of_kind.all()), (what, kd)
            assert torch.equal(mask1[new], mask0[src[new]]) and int(new.sum()) >= 2, what
        elif kind == "reset_dynamic":
            step = float(pc.optimizer.state[pc._opacity]["step"])
            tw.reset_opacity(tw.get_motion_mask)                                        # train.py:459
            pc.reset_opacity(pc.get_motion_mask)
            st = pc.optimizer.state[pc._opacity]
            assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(st["step"]) == step == float(self.it), what
            assert float(pc.get_opacity.detach()[mask0].max()) <= 0.01 * (1 + 1e-5) < float(pc.get_opacity.detach()[~mask0].max()), what
            q = DeformQuery(pc.get_motion_mask.contiguous())
            assert (q.n, q.P) == (n0, P0) and torch.equal(pc.get_motion_mask, mask0), what
        elif kind == "prune_dynamic":
            tw.prune_points(tw.get_motion_mask)
            densify.prune_points(pc, pc.get_motion_mask)
            q = DeformQuery(pc.get_motion_mask.contiguous())
            assert pc._xyz.shape[0] == P0 - n0 and q.n == 0 and not pc.get_motion_mask.any() and n0 > 0, what
        L.assert_same_snapshot(pc, tw, what)
        assert [g["name"] for g in pc.optimizer.param_groups] == L.NAMES + ["phase_offset"]
        for g in pc.optimizer.param_groups[:-1]:
            assert g["params"][0] is getattr(pc, L.ATTR[g["name"]]), (what, g["name"])
        net_after = network_state(self.net, self.opt_net)                                # the network: untouched by the event
        for name, s in net_before.items():
            for k in ("param", "exp_avg", "exp_avg_sq"):
                assert (s[k] is None) == (net_after[name][k] is None) and (s[k] is None or torch.equal(s[k], net_after[name][k])), (what, name, k)
            assert s["step"] == net_after[name]["step"], (what, name)
        print("%s: P %d -> %d, n %d -> %d" % (what, P0, pc._xyz.shape[0], n0, q.n))
        self.phase = kind
        self.new_shape(q)
        return kind


def _run(mode, schedule, dev, oracle):
    from gftorf_amd import api
    loop = _Loop(mode, schedule, dev, oracle)
    last_event, shapes = "start", [(loop.P, loop.n)]
    n_checked = 3 if mode == "graph" else 2              # graph: two eager iterations and the first replay of the shape
    replays = {}
    while loop.it < ITERATIONS:
        checked = loop.in_shape < n_checked
        if loop.iteration(checked) and checked:
            replays[last_event] = replays.get(last_event, 0) + 1
        if loop.it in EVENTS:
            last_event = loop.event(EVENTS[loop.it])
            shapes.append((loop.P, loop.n))
    torch.cuda.synchronize()
    print("shapes (P, n):", shapes)
    print("observed maxima (%s, %s): %s" % (schedule, mode, {k: float("%.3g" % v) for k, v in sorted(loop.maxima.items())}))
    # both densifications change P and n, the reset keeps both, the last event leaves the static Gaussians
    assert len(shapes) == 5 and shapes[0][0] == 1500 and shapes[2] == shapes[1] and shapes[4] == (shapes[3][0] - shapes[3][1], 0), shapes
    assert len({s[0] for s in shapes[:4]}) == 3 and max(s[0] for s in shapes) <= 4000 and 2 * max(s[1] for s in shapes) <= 2500, shapes
    # every group that learns has taken every step, re-keyed or not; the network the steps that had a dynamic row
    for g in loop.pc.optimizer.param_groups:
        st = loop.pc.optimizer.state.get(g["params"][0], None)
        if g["name"] in ("f_seg_color", "phase_offset"):
            assert not st, g["name"]
        else:
            assert float(st["step"]) == float(ITERATIONS), (g["name"], float(st["step"]))
    assert loop.net_steps == EVENTS_AT["prune_dynamic"]
    for name, s in network_state(loop.net, loop.opt_net).items():
        learns = name not in NEVER and not (schedule == "ftorf" and name in RGB)
        assert s["step"] == (float(loop.net_steps) if learns else None), (name, s["step"])
    # operator state: bounded; no frame that was queued without a host read outgrew its binning buffer
    assert len(api.state.grad_pool) <= 8 and len(api.state.acc_pool) <= 8 and len(api.state.status) <= api.state.MAX_SHAPES
    assert not any(x["overflow"] or x["overflows"] for x in api.enqueue_status())
    if mode == "graph":           # a checked replay after every event, the one that left no dynamic row included
        assert all(replays.get(k, 0) >= 1 for k in ["start"] + list(EVENTS.values())), replays


EVENTS_AT = {kind: it for it, kind in EVENTS.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["ftorf", "torf"])
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_dynamic_loop_across_fused_densification(mode, schedule, oracle, gpu):
    from gftorf_amd import api, deform as D
    flags = {k: getattr(api, k) for k in API_FLAGS}
    rows_from = D._SPARSE_MIN_POINTS
    api.state.reset()
    try:
        D._SPARSE_MIN_POINTS = 1          # the row-counting backward at this test's 500-2000 rows (the module's docstring)
        _run(mode, schedule, gpu, oracle)
    finally:
        D._SPARSE_MIN_POINTS = rows_from
        for k, v in flags.items():
            setattr(api, k, v)
        api.state.reset()
