"""The training step ACROSS densification, pruning and an opacity reset (train.py:441-461): the reference's loop shape --
assemble_parameters over the model's own tensors, the colour + ToF rasterizer call, an L1 loss, backward, the densification
statistics, FusedAdam under a learning rate that moves every iteration -- run through the product for 38 iterations on a
1500-Gaussian scene (a dense and a sparse one, SCENES) while five events change the model and at last bring the number of
Gaussians back to its first value.  Every
event invalidates what the package keeps from one call to the next (api.state's size hints, status blocks, kept gradient
tensors and accumulators, plans; FusedAdam's state handed to a new nn.Parameter; in the capturable mode the step slots, the
pinned learning rates and every captured graph), and the return to P = 1500 hands kept buffers whose invariant is "every
unmarked row is zero" to another set of Gaussians.

TEACHER FORCING: there is one trajectory, the product's.  Each checked step is compared with an independent reference
evaluated on the product's own state just before that step (Adam turns rounding noise into whole steps and a threshold
turns it into another P: two free-running trajectories cannot be compared tightly enough to see a stale buffer).

Every Gaussian is static here; the deformation network and a motion mask that densification keeps in step are carried through
the same kind of loop by tests/test_loop_dynamic.py; the SH degree schedule (here the constant 3, _Loop's `degrees`) by
tests/test_loop_sh_degree.py.  Not covered: the length of a real run (38 iterations, not 7 000).

CPU tests: the restated reset_opacity / replace_tensor_to_optimizer against a per-row loop, the twin copy, the thresholds."""
import numpy as np
import pytest
import torch

from oracle import densify_ref
from tests import helpers, loop_densify as L

EVENTS = {8: "densify", 14: "densify_screen", 20: "reset", 26: "prune", 32: "return"}     # after this iteration: the event
ITERATIONS = 38
EVENTS_AT = {kind: it for it, kind in EVENTS.items()}
EAGER_FIRST = 2           # graph mode: iterations of a shape that run eagerly before it is captured
# The Gaussians are spread over `spread` times the image (tests/helpers.small_scene).  "dense": nearly all of the 1500 are
# blended, so a kept set of gradient tensors is written in full from its third backward on (api._DENSE_SHARE).  "sparse": one
# in five is, every reused set is rewritten row by row, and the set kept for P = 1500 meets OTHER rows when P comes back.
SCENES = {"dense": 1.05, "sparse": 3.0}
API_FLAGS = ("no_host_read", "_GRADS_REUSE", "_GRADS_CHECK", "_ACC_REUSE", "_TILE_HINTS", "_TILE_HINTS_PER_CAMERA", "_CELL_SCHED",
             "_FWD_ORDER", "_force_cell_sched", "_force_whole_lists", "_DETERMINISTIC", "keep_last_buffers")


# ---- CPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_reset_opacity_restatement_matches_the_loop(masked):
    pc = densify_ref.EagerGaussians(257, "cpu", seed=11)
    before = pc.twin()
    apply = (torch.rand(257, generator=torch.Generator().manual_seed(5)) < 0.4) if masked else None
    old_params = {g["name"]: g["params"][0] for g in pc.optimizer.param_groups}
    old_state = pc.optimizer.state[pc._opacity]
    pc.reset_opacity(apply)
    want, wrote = densify_ref.reset_opacity_loops(before._opacity.detach().numpy(), None if apply is None else apply.numpy())
    got = pc._opacity.detach().numpy()
    assert wrote.sum() == (257 if apply is None else int(apply.sum())) and 0 < wrote.sum()
    np.testing.assert_array_equal(got[~wrote], before._opacity.detach().numpy()[~wrote])        # rows outside the mask keep their bits
    np.testing.assert_allclose(got[wrote], want[wrote], rtol=2e-6)                              # (float32 sigmoid / log against float64)
    assert (1.0 / (1.0 + np.exp(-got[wrote].astype(np.float64))) <= 0.01 * (1 + 1e-6)).all()
    lowered = (before.get_opacity.detach().numpy()[:, 0] > 0.0101) & wrote
    assert lowered.any() and (got[lowered, 0] < before._opacity.detach().numpy()[lowered, 0]).all()
    # the optimizer: the group holds the new leaf, the SAME state dict with zeroed moments and the count it had
    grp = [g for g in pc.optimizer.param_groups if g["name"] == "opacity"][0]
    assert grp["params"][0] is pc._opacity and pc._opacity.is_leaf and pc._opacity.requires_grad
    assert pc._opacity is not old_params["opacity"] and old_params["opacity"] not in pc.optimizer.state
    st = pc.optimizer.state[pc._opacity]
    assert st is old_state and float(st["step"]) == 1.0
    assert st["exp_avg"].shape == pc._opacity.shape and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    # every other group: the same parameter object, its state untouched
    sa, sb = pc.snapshot(), before.snapshot()
    for g in pc.optimizer.param_groups:
        if g["name"] != "opacity":
            assert g["params"][0] is old_params[g["name"]]
    for k in sa:
        if k not in ("_opacity", "m:opacity", "v:opacity"):
            assert torch.equal(sa[k], sb[k]), k
    for g in pc.optimizer.param_groups:              # and the optimizer still steps
        g["params"][0].grad = torch.ones_like(g["params"][0])
    pc.optimizer.step()
    assert float(pc.optimizer.state[pc._opacity]["step"]) == 2.0


def test_twin_copy_preserves_step_and_moments():
    pc = densify_ref.EagerGaussians(64, "cpu", seed=2)
    for _ in range(2):
        for g in pc.optimizer.param_groups[:5]:         # the other groups stay at step 1
            g["params"][0].grad = torch.full_like(g["params"][0], 0.25)
        pc.optimizer.step()
        pc.optimizer.zero_grad(set_to_none=True)
    tw = pc.twin()
    L.assert_same_snapshot(pc, tw, "twin")
    snap = pc.snapshot()
    assert float(snap["step:xyz"]) == 3.0 and float(snap["step:rotation"]) == 1.0 and snap["m:xyz"].abs().sum() > 0
    assert [g["lr"] for g in tw.optimizer.param_groups] == [g["lr"] for g in pc.optimizer.param_groups]
    for ga, gb in zip(pc.optimizer.param_groups[:-1], tw.optimizer.param_groups[:-1]):
        pa, pb = ga["params"][0], gb["params"][0]
        assert pa.data_ptr() != pb.data_ptr() and getattr(tw, L.ATTR[ga["name"]]) is pb
        if pa in pc.optimizer.state and "exp_avg" in pc.optimizer.state[pa]:
            for k in ("step", "exp_avg", "exp_avg_sq"):
                assert pc.optimizer.state[pa][k].data_ptr() != tw.optimizer.state[pb][k].data_ptr(), k
    # a model of a scene: no state yet, and the twin has none either; the activations give the scene back
    sc = helpers.small_scene(P=50, W=32, H=32, seed=1)
    m = densify_ref.EagerGaussians.from_scene(sc["gaussians"], "cpu", lrs=L.LRS)
    assert len(m.optimizer.state) == 0 and len(m.twin().optimizer.state) == 0
    np.testing.assert_allclose(m.get_opacity.detach().numpy(), sc["gaussians"]["opacities"].reshape(50, 1), rtol=1e-5)
    np.testing.assert_allclose(m.get_scaling.detach().numpy(), sc["gaussians"]["scales"], rtol=1e-6)
    assert [g["lr"] for g in m.optimizer.param_groups][:-1] == [L.LRS[n] for n in L.NAMES]
    # tw steps on: pc does not move
    for g in tw.optimizer.param_groups:
        g["params"][0].grad = torch.ones_like(g["params"][0])
    tw.optimizer.step()
    after = pc.snapshot()
    assert all(torch.equal(after[k], snap[k]) for k in snap)
    assert float(tw.snapshot()["step:xyz"]) == 4.0


def test_thresholds_select_rows_in_every_branch():
    pc = densify_ref.EagerGaussians(500, "cpu", seed=9)            # random statistics, some rows never seen (denom 0)
    assert (pc.denom == 0).any()
    th = L.thresholds(pc)
    clone, split, prune = L.selections(pc, th)
    assert clone.any() and split.any() and prune.any() and not (clone & split).any()
    assert np.isfinite(list(th.values())).all() and th["max_grad"] > 0
    torch.manual_seed(1)
    pc.densify_and_prune(th["max_grad"], th["min_opacity"], th["extent"], None)
    P1 = pc._xyz.shape[0]
    pruned = 500 + int(clone.sum()) + int(split.sum()) - P1          # clones appended, every split row replaced by two
    assert pruned >= 1 and P1 != 500
    assert L.xyz_lr(0) == pytest.approx(L.LRS["xyz"]) and L.xyz_lr(40) == pytest.approx(L.LRS["xyz"] * 0.01)
    assert all(L.xyz_lr(i + 1) < 0.9 * L.xyz_lr(i) for i in range(40))


# ---- GPU -------------------------------------------------------------------------------------------------------------------
class _Loop:
    """The loop of one mode: model, optimizer, target, the iteration (eager or captured per shape and SH degree), the events,
    the checks.  `degrees`: iteration -> active SH degree (oneupSHdegree's schedule, train.py); None: 3 throughout."""

    def __init__(self, mode, dev, oracle, spread, degrees=None):
        from gftorf_amd import FusedAdam
        self.mode, self.dev, self.oracle, self.sparse = mode, dev, oracle, spread > 2.0
        self.scene = helpers.small_scene(P=1500, W=96, H=64, seed=33, spread=spread)
        self.degrees = degrees if degrees is not None else (lambda it: self.scene["cfg"]["D"])
        self.D, self.rasts = self.scene["cfg"]["D"], {}
        self.frames = []                 # every rasterizer call: dict(P, D, captured, R = num_rendered, backward, reused, rows_only)
        g = self.scene["gaussians"]
        t32 = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
        with torch.no_grad():            # the target: a render of the unperturbed scene (at the full degree)
            out = self.render(t32(g["means3D"]), torch.zeros((1500, 3), device=dev), t32(g["opacities"]).reshape(1500, 1),
                              t32(g["shs"]), t32(g["shs_p"]), t32(g["scales"]), t32(g["rotations"]))
            self.target = dict(color=out[0].clone(), phasor=out[1].clone())
        self.target_np = {k: v.cpu().numpy() for k, v in self.target.items()}
        self.pc = L.make_model(g, dev, FusedAdam, capturable=(mode == "graph"))
        self.it = 0
        self.new_shape()

    def rasterizer(self, D):
        """One GaussianRasterizer per degree, its settings carrying that degree (and its own tensors: kept for the run)."""
        from gftorf_amd import GaussianRasterizer
        if D not in self.rasts:
            self.rasts[D] = GaussianRasterizer(raster_settings=helpers.gpu_settings(self.scene, self.dev, sh_degree=D))
        return self.rasts[D]

    def scene_at(self, D):
        """The scene as the composed reference takes it at degree `D` (cfg["D"] is what helpers.run_oracle hands the oracle)."""
        return dict(self.scene, cfg=dict(self.scene["cfg"], D=D))

    def render(self, m3, m2, op, shs, shp, sc, ro):
        from gftorf_amd import api
        out = self.rasterizer(self.D)(means3D=m3, means2D=m2, opacities=op, shs=shs, shs_p=shp, scales=sc, rotations=ro,
                                      phase_offset=self.scene["phase_offset"], dc_offset=self.scene["dc_offset"])
        self.frames.append(dict(P=m3.shape[0], D=self.D, captured=torch.cuda.is_current_stream_capturing(), R=api.last_call_stats["num_rendered"],
                                backward=torch.is_grad_enabled(), reused=api.last_call_stats.get("grads_reused"),
                                rows_only=api.last_call_stats.get("grads_rows_only")))
        return out

    def new_shape(self):
        """After an event: nothing of the old shape is kept -- the graphs (one per degree), their static tensors, the
        screen-space leaf.  `in_shape` counts the iterations of the shape at the degree in use."""
        self.P = self.pc._xyz.shape[0]
        self.ssp = torch.zeros((self.P, 3), device=self.dev, requires_grad=True)
        self.mask = torch.zeros((self.P,), dtype=torch.bool, device=self.dev)        # no motion mask: every Gaussian is static
        self.in_shape, self.graphs = 0, {}

    def body(self):
        """The device work of one iteration (train.py:164-231, 441-449, 468-474); what the checks read is copied before the
        gradients are dropped -- inside a capture into tensors of the graph's pool, which every replay rewrites."""
        from gftorf_amd import assemble_parameters, densify
        pc, ssp = self.pc, self.ssp
        ssp.grad = None
        m3, m2, op, sc, ro, shs, shp = assemble_parameters(
            pc._xyz, ssp, pc._opacity, pc._scaling, pc._rotation, pc._features_dc_color, pc._features_rest_color,
            pc._features_dc_phase, pc._features_rest_phase, pc._features_dc_amp, pc._features_rest_amp, self.mask,
            0.0, 0.0, 0.0, 0.0, render_regions=("static",))
        out = self.render(m3, m2, op, shs, shp, sc, ro)
        color, phasor, pixels, radii = out[0], out[1], out[8], out[10]
        loss = (color - self.target["color"]).abs().mean() + (phasor - self.target["phasor"]).abs().mean() * 0.5
        loss.backward()
        with torch.no_grad():
            kept = dict(color=color.detach().clone(), phasor=phasor.detach().clone(), pixels=pixels.detach().clone(),
                        radii=radii.clone(), ssp=ssp.grad.clone(), loss=loss.detach().clone(),
                        grads={n: getattr(pc, L.ATTR[n]).grad.clone() for n in L.NAMES if getattr(pc, L.ATTR[n]).grad is not None})
            densify.add_densification_stats(pc.xyz_gradient_accum, pc.denom, pc.max_radii2D, ssp.grad, radii > 0, pixels, radii)
            pc.optimizer.step()
            pc.optimizer.zero_grad(set_to_none=True)
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
        before = L.optimizer_state(pc)                                          # clones, outside the graph
        stats = [t.cpu().clone() for t in (pc.xyz_gradient_accum, pc.denom, pc.max_radii2D)]
        replay = self.mode == "graph" and self.in_shape >= EAGER_FIRST
        if not replay:
            kept = self.body()
        else:
            if self.D not in self.graphs:
                # torch's recipe for a whole-iteration capture: eager iterations first, no gradient tensor alive
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    static = self.body()
                self.graphs[self.D] = (graph, static)      # (the capture ran nothing: this iteration is the first replay)
            pc.optimizer.refresh_lr()
            graph, kept = self.graphs[self.D]
            graph.replay()
        self.in_shape += 1
        torch.cuda.synchronize()
        what = "iteration %d (P = %d, D = %d, %s%s)" % (self.it, self.P, self.D, self.mode, ", replay" if replay else "")
        after = L.optimizer_state(pc)
        L.assert_adam_step(before, kept["grads"], lrs, after, what)             # every iteration
        assert set(kept["grads"]) == set(L.NAMES) - {"f_seg_color"}, what
        assert np.isfinite(float(kept["loss"])), what
        self.every_iteration(before, kept, after, what)
        if checked:
            self.check_render(before, kept, what)
            self.check_stats(stats, kept, what)
        return replay

    def next_degree(self):
        """The degree of the next iteration (oneupSHdegree): a degree step begins a new phase of the shape -- `in_shape` starts
        again; the shape stays, and so do the graphs of its earlier degrees.  Returns the degree."""
        D = self.degrees(self.it + 1)
        if D != self.D:
            self.D, self.in_shape = D, 0
        return D

    def every_iteration(self, before, kept, after, what):
        """Further checks of every iteration (tests/test_loop_sh_degree.py)."""

    def checked_step(self, before, kept, f, ref, what):
        """Further checks of a checked step (from the state `before`) against the composed reference's forward `f` and
        gradients `ref`."""

    def check_render(self, before, kept, what):
        color, phasor = kept["color"].cpu().numpy(), kept["phasor"].cpu().numpy()
        up_c = L.l1_upstream(color, self.target_np["color"], 1.0)
        up_p = L.l1_upstream(phasor, self.target_np["phasor"], 0.5)
        f, ref = L.composed_reference(self.oracle, self.scene_at(self.D), {n: before[n]["param"] for n in L.NAMES}, up_c, up_p)
        mae_c = float(np.abs(color - f["color"]).mean())
        # (the phasor planes are amplitudes, not bounded by one: the colour's bound in units of the largest reference value)
        mae_p = float(np.abs(phasor - f["phasor"]).mean()) / max(1.0, float(np.abs(f["phasor"]).max()))
        rels = {n: L.rel(kept["grads"][n].cpu().numpy(), ref[n]) for n in kept["grads"]}
        rels["ssp"] = L.rel(kept["ssp"].cpu().numpy(), ref["ssp"])
        print("%s: colour mae %.3g, phasor mae %.3g, gradients %s" % (what, mae_c, mae_p, {k: float("%.3g" % v) for k, v in rels.items()}))
        assert mae_c < 1e-5 and mae_p < 1e-5, (what, mae_c, mae_p)
        assert np.array_equal(kept["radii"].cpu().numpy() > 0, np.asarray(f.radii) > 0), what
        for k, v in rels.items():
            assert v < 1e-3, (what, k, v)
        assert int((kept["radii"] > 0).sum()) > 100 and np.abs(ref["xyz"]).max() > 0, what
        self.checked_step(before, kept, f, ref, what)

    def check_stats(self, stats, kept, what):
        acc, den, mr = stats
        densify_ref.add_densification_stats_eager(acc, den, mr, kept["ssp"].cpu(), (kept["radii"] > 0).cpu(), kept["pixels"].cpu(),
                                                  kept["radii"].cpu())
        pc = self.pc
        for name, got, want in (("xyz_gradient_accum", pc.xyz_gradient_accum, acc), ("denom", pc.denom, den), ("max_radii2D", pc.max_radii2D, mr)):
            assert torch.equal(got.cpu(), want), (what, name)

    def event(self, kind):
        """The product's function on the model, the reference's statements on a twin made just before, same generator state:
        the snapshots agree key for key, bit for bit."""
        from gftorf_amd import densify
        pc = self.pc
        tw = pc.twin()
        L.assert_same_snapshot(pc, tw, "twin before " + kind)
        P0, seed, what = self.P, 1000 + self.it, "%s after iteration %d" % (kind, self.it)
        if kind in ("densify", "densify_screen", "densify_fused"):
            th = L.thresholds(pc)
            clone, split, _ = L.selections(pc, th)
            size = 20 if kind == "densify_screen" else None
            torch.manual_seed(seed)
            tw.densify_and_prune(th["max_grad"], th["min_opacity"], th["extent"], size)
            torch.manual_seed(seed)
            product = densify.densify_and_prune_fused if kind == "densify_fused" else densify.densify_and_prune
            product(pc, th["max_grad"], th["min_opacity"], th["extent"], size)
            P1 = pc._xyz.shape[0]
            pruned = P0 + int(clone.sum()) + int(split.sum()) - P1
            assert int(clone.sum()) >= 1 and int(split.sum()) >= 1 and pruned >= 1 and P1 != P0, (what, int(clone.sum()), int(split.sum()), pruned, P1)
        elif kind == "reset":
            step = float(pc.optimizer.state[pc._opacity]["step"])
            tw.reset_opacity()
            pc.reset_opacity()          # the reference's own statements on the product's optimizer
            st = pc.optimizer.state[pc._opacity]
            assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(st["step"]) == step == float(self.it), what
            assert float(pc.get_opacity.detach().max()) <= 0.01 * (1 + 1e-5), what
        elif kind == "prune":
            th = L.thresholds(pc)
            tw.prune_points((tw.get_opacity < th["min_opacity"]).squeeze())
            densify.prune(pc, th["min_opacity"])
            # (after the reset a Gaussian no pixel sees keeps the reset's value bit for bit: in the sparse scene the quantile
            # IS that value and `<` takes only what moved below it)
            assert pc._xyz.shape[0] < P0 or self.sparse, what
        elif kind == "return":
            if P0 <= 1500:              # clone-only densification of every row, so that there is something to take away
                grads = torch.zeros((P0, 1), device=self.dev)
                tw.densify_and_clone(grads, 0.0, float("inf"))
                densify.densify_and_clone(pc, grads, 0.0, float("inf"))
            n = pc._xyz.shape[0]
            assert n > 1500, what
            newest = torch.arange(n, device=self.dev) >= 1500
            tw.prune_points(newest)
            densify.prune_points(pc, newest)
            assert pc._xyz.shape[0] == 1500, what
        L.assert_same_snapshot(pc, tw, what)
        assert [g["name"] for g in pc.optimizer.param_groups] == L.NAMES + ["phase_offset"]
        for g in pc.optimizer.param_groups[:-1]:
            assert g["params"][0] is getattr(pc, L.ATTR[g["name"]]), (what, g["name"])
        print("%s: P %d -> %d" % (what, P0, pc._xyz.shape[0]))
        self.new_shape()
        return kind


def _run(mode, dev, oracle, scene):
    from gftorf_amd import api
    loop = _Loop(mode, dev, oracle, SCENES[scene])
    last_event, shapes = "start", [loop.P]
    n_checked = 3 if mode == "graph" else 2              # graph: two eager iterations and the first replay of the shape
    replays = {}
    while loop.it < ITERATIONS:
        checked = loop.in_shape < (3 if last_event == "return" else n_checked)
        if loop.iteration(checked) and checked:
            replays[last_event] = replays.get(last_event, 0) + 1
        if loop.it in EVENTS:
            last_event = loop.event(EVENTS[loop.it])
            shapes.append(loop.P)
    torch.cuda.synchronize()
    # both densifications change P, the reset keeps it, the last event brings the first P back
    assert len(shapes) == 6 and shapes[0] == shapes[5] == 1500 and shapes[1] != 1500 and shapes[2] not in (1500, shapes[1]), shapes
    assert shapes[3] == shapes[2] and shapes[4] <= shapes[3] and max(shapes) <= 4000, shapes
    # every group that learns has taken every step, re-keyed or not
    for g in loop.pc.optimizer.param_groups:
        st = loop.pc.optimizer.state.get(g["params"][0], None)
        if g["name"] in ("f_seg_color", "phase_offset"):
            assert not st, g["name"]
        else:
            assert float(st["step"]) == float(ITERATIONS), (g["name"], float(st["step"]))
    # operator state: bounded, and the flow every frame took
    assert len(api.state.grad_pool) <= 8 and len(api.state.acc_pool) <= 8 and len(api.state.status) <= api.state.MAX_SHAPES
    seen, backwards = set(), {}
    for fr in loop.frames:
        P, R = fr["P"], fr["R"]
        first = P not in seen
        seen.add(P)
        if fr["captured"]:
            assert R == -1, fr
        elif first:
            assert R >= 0, fr                             # a new P: the blocking flow, a counted frame
        elif mode == "no_host_read":
            assert R == -1, fr                            # ... once: every later frame of the shape is queued without a host read
        else:
            assert R >= 0, fr
        if fr["backward"] and not fr["captured"]:
            backwards.setdefault(P, []).append(fr)
    assert seen == set(shapes)
    print("gradient sets (reused, row by row) per eager backward:", {P: [(int(f["reused"]), int(f["rows_only"])) for f in v] for P, v in backwards.items()})
    for P, v in backwards.items():
        # the kept gradient tensors are in play: every eager backward of a shape but its first takes a kept set -- in the sparse
        # scene row by row (api._GradEntry.write_mode: fewer than _DENSE_SHARE of the rows are written)
        assert not v[0]["reused"] and all(f["reused"] for f in v[1:]), (P, v)
        assert scene != "sparse" or all(f["rows_only"] for f in v[1:]), (P, v)
    if mode != "graph":
        # ... the first backward after the return to P = 1500 included: it takes the set other Gaussians left (8 shapes are kept)
        assert len(backwards[1500]) == EVENTS_AT["densify"] + ITERATIONS - EVENTS_AT["return"], len(backwards[1500])
    else:
        # a checked replay after a cat (both densifications), a prune, replace_tensor_to_optimizer, and at the old P
        assert all(replays.get(k, 0) >= 1 for k in ("densify", "densify_screen", "reset", "prune", "return")), replays
    # no frame that was queued without a host read outgrew its binning buffer (its outputs would have been undefined)
    assert not any(x["overflow"] or x["overflows"] for x in api.enqueue_status())


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("mode", ["eager", "no_host_read", "graph"])
def test_loop_across_densification_pruning_and_opacity_reset(mode, scene, oracle, gpu):
    from gftorf_amd import api
    flags = {k: getattr(api, k) for k in API_FLAGS}
    api.state.reset()
    try:
        api.no_host_read = mode == "no_host_read"
        _run(mode, gpu, oracle, scene)
    finally:
        for k, v in flags.items():
            setattr(api, k, v)
        api.state.reset()
