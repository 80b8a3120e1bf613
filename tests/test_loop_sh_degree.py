"""The training loop ACROSS the SH-degree schedule (oneupSHdegree, train.py: the active degree rises 0 -> 3 while the feature
tensors are sized for degree 3 from the start).  The loops of tests/test_loop_densify.py and tests/test_loop_dynamic.py, their
`_Loop` classes given a degree schedule: 22 iterations from small_scene(P=1500, 96x64, seed=33), degree 0 for iterations 1-4,
1 for 5-9, 2 for 10-16, 3 for 17-22, and one densify_and_prune_fused event after iteration 12 -- a shape change inside a degree
phase, so that new rows inherit inactive coefficients and the last degree step happens on the shape the event left.  The
rasterizer of every iteration carries that iteration's `sh_degree`; the composed reference takes it as cfg["D"].

The degree is part of no key of what the package keeps between calls (api.state.grad_pool: (device, P, layout); the
per-camera schedules; the accumulators): one kept set of gradient tensors is written at degree 0, then 1, 2, 3 -- row by row
(cfg.grads_zeroed = 3) in the sparse scene, in full in the dense one.  In graph mode the graphs of a shape's earlier degrees
stay alive beside the one in use, as bench_loop.py keeps them.

What is pinned, WITHOUT a tolerance, on every iteration: until its degree is active a coefficient's gradient is an exact zero,
its parameter keeps its bits (those of iteration 0; after the event those the event left, which the twin holds to the
reference's) and both its Adam moments are exact zeros, while its group's `step` counts on.  With eps = 1e-15 a stale 1e-12
in such a column would move the parameter by about a whole learning-rate step.
On the checked steps (the first two of every degree phase and after the event; in graph mode the first replay too): the
bounds of test_loop_densify.py, and every SH gradient per degree band (coefficients l^2 .. (l+1)^2 - 1 of every active l,
separately for colour, phase and amplitude) to 1e-3 of the BAND's max-norm -- the dc band is 0.99 of the whole tensor's norm
and hides the others.  On the first checked step of a degree the new band's gradient is non-zero on exactly the rows where the
reference's is, those are the blended Gaussians (but a clamped colour / amplitude), and the step moves every one of them.

Dynamic variant: the "torf" schedule of test_loop_dynamic.py (d_sh a tensor, so the assembly's SH backward is the one that
does not alias the feature tensor) under the same degrees with its own "densify" event after iteration 12: the rows of the
network's r / g / b heads (row k = coefficient k, oracle/deform_ref.py) beyond (D + 1)^2 have an exactly zero gradient in
.weight and .bias, keep their bits and have zero moments.

Observed maxima on an MI355X (printed per checked step and per run), error / the band's max-norm: static cases 4.7e-7 (l = 0),
4.4e-7 (1), 4.0e-7 (2), 3.2e-7 (3); dynamic cases 2.5e-6, 2.4e-6, 2.1e-6, 7.6e-7; bound 1e-3.  Colour / phasor mae <= 1e-7,
whole-tensor gradients <= 1.6e-5, as in the loops this one is built on.  0.2-0.3 s a static case, 1.5 s a dynamic one.

Teeth, on scratch copies ("The SH-degree schedule in the loop"):
(a) the old degree's graph replayed once after a degree step (a graph key that forgets the degree): all three graph cases
    fail the composed reference at iteration 5, colour mae 0.0113 (dense), 0.0047 (sparse), 0.0119 (dynamic) against 1e-5.
(b) sh_backward's tail loop over the inactive coefficients removed: NO case of this file fails, and none can -- with the
    forward's direction-gradient records, which every backward of the Python surface has, dL/dsh is formed by
    sh_backward_basis (a zero basis value times the colour gradient).  sh_backward runs in a backward without the records:
    test_gpu_parity.py::test_sh_degrees_without_direction_records was added for it and fails in its six cases with an
    inactive coefficient (dL_dsh max error 0.21 .. 3.8 against 7e-4 .. 1.4e-3).  The counterpart on the path that runs
    (sh_backward_basis writing the active coefficients only) fails test_kept_gradient_tensors_across_sh_degrees in all four
    configurations (0.49 .. 8.2) and no case here: while the degree only rises, no row holds more columns than are written.
(c) zero_gradient_rows clearing 3 (D + 1)^2 columns only: for the same reason no case here; all four configurations of
    test_kept_gradient_tensors_across_sh_degrees at their first falling step (sparse: dL_dsh max error 3.66 against 1.9e-3).

CPU tests: the composed reference has exact zeros in every inactive column; consecutive degrees differ by at least 100 times
the image bound on both scenes (the teeth of the checked steps: a stale degree cannot pass); the blended share is on either
side of api._DENSE_SHARE; torch.optim.Adam freezes zero-gradient columns bit for bit."""
import numpy as np
import pytest
import torch

import test_loop_densify as TD
import test_loop_dynamic as TY
from tests import helpers, loop_densify as L

ITERATIONS = 22
EVENT_AFTER = 12
REST = ("f_rest_color", "phase_f_rest", "amp_f_rest")
DC = {"f_rest_color": "f_dc_color", "phase_f_rest": "phase_f_dc", "amp_f_rest": "amp_f_dc"}
IMAGE_BOUND = 1e-5        # the loops' bound on the colour / phasor mae
BAND_TOL = 1e-3           # the loops' bound on a gradient, here of the band's own max-norm
RGB_HEADS = ("r", "g", "b")


def degree_of(it):
    """Degree 0 for iterations 1-4, 1 for 5-9, 2 for 10-16, 3 from 17 on."""
    return 0 if it <= 4 else 1 if it <= 9 else 2 if it <= 16 else 3


def first_inactive(D):
    """Index into a rest tensor [P, 15, C] of the first coefficient that degree `D` does not use."""
    return (D + 1) ** 2 - 1


def bands(D):
    """The rest tensors' slices of the active degrees 1 .. D: {l: slice}."""
    return {l: slice(l * l - 1, (l + 1) ** 2 - 1) for l in range(1, D + 1)}


def band_errors(got, ref, D):
    """{(tensor, l): (max error / the band's max-norm, the band's max-norm)} of the dc and rest gradients `got` against `ref`
    (both: group name -> array), for every active degree l <= D."""
    out = {}
    for rest in REST:
        out[(DC[rest], 0)] = (L.rel(got[DC[rest]], ref[DC[rest]]), float(np.abs(ref[DC[rest]]).max()))
        for l, sl in bands(D).items():
            out[(rest, l)] = (L.rel(got[rest][:, sl], ref[rest][:, sl]), float(np.abs(ref[rest][:, sl]).max()))
    return out


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def _reference_at(oracle, spread, D, cache={}):
    """(oracle forward, composed-reference gradients) of the perturbed scene at degree D under the L1 loss against the
    unperturbed scene's own degree-3 render (the loop's first iteration); computed once per (spread, D)."""
    if (spread, D) not in cache:
        scene = helpers.small_scene(P=1500, W=96, H=64, seed=33, spread=spread)
        if spread not in cache:
            cache[spread] = helpers.run_oracle(oracle, scene, backward=False)[0]
        target = cache[spread]
        pc = L.make_model(scene["gaussians"], "cpu", torch.optim.Adam)
        raw = {n: getattr(pc, L.ATTR[n]).detach() for n in L.NAMES}
        at = dict(scene, cfg=dict(scene["cfg"], D=D))
        zero = {k: np.zeros_like(target[k]) for k in ("color", "phasor")}
        f, _ = L.composed_reference(oracle, at, raw, zero["color"], zero["phasor"])
        up_c = L.l1_upstream(f["color"], target["color"], 1.0)
        up_p = L.l1_upstream(f["phasor"], target["phasor"], 0.5)
        cache[(spread, D)] = L.composed_reference(oracle, at, raw, up_c, up_p)
    return cache[(spread, D)]


@pytest.mark.parametrize("scene", list(TD.SCENES))
def test_reference_has_exact_zeros_in_inactive_columns_and_degrees_differ(scene, oracle):
    spread = TD.SCENES[scene]
    refs = [_reference_at(oracle, spread, D) for D in range(4)]
    for D in range(3):
        f, g = refs[D]
        lo = first_inactive(D)
        for name in REST:
            assert g[name].shape[1] == 15 and not g[name][:, lo:].any(), (D, name)
            for l, sl in bands(D).items():
                assert np.abs(g[name][:, sl]).max() > 0, (D, name, l)
        for name in DC.values():
            assert np.abs(g[name]).max() > 0, (D, name)
    # the teeth of the checked steps: the image of the neighbouring degree is at least 100 bounds away, in the measure of the
    # loops' check (mean abs; the phasor planes in units of their largest value where that is above one).  A checked step
    # asserts both planes, so one plane that far away is what a stale degree cannot pass: the colour plane is, on both scenes
    # (dense 0.011 .. 0.018, sparse 0.0048 .. 0.0076), and so is the phasor plane of the dense scene (0.0027 .. 0.0039).  The
    # sparse scene's phasor plane, a seventh of the Gaussians on the image, is 77, 91 and 117 bounds away (0.00077, 0.00091,
    # 0.00117): printed, and held to the bound itself only.
    short = []
    for D in range(3):
        fa, fb = refs[D][0], refs[D + 1][0]
        d_c = float(np.abs(fa["color"] - fb["color"]).mean())
        d_p = float(np.abs(fa["phasor"] - fb["phasor"]).mean()) / max(1.0, float(np.abs(fb["phasor"]).max()))
        print("%s, degree %d against %d: colour %.3g, phasor %.3g mean abs" % (scene, D, D + 1, d_c, d_p))
        short += [(D, plane, d) for plane, d in (("color", d_c), ("phasor", d_p))
                  if d < (IMAGE_BOUND if (scene, plane) == ("sparse", "phasor") else 100 * IMAGE_BOUND)]
    assert not short, (scene, short)


def test_blended_share_is_on_either_side_of_the_full_write_threshold(oracle):
    from gftorf_amd import api
    share = {}
    for scene, spread in TD.SCENES.items():
        f = _reference_at(oracle, spread, 3)[0]
        share[scene] = float(((np.asarray(f.radii) > 0) & (np.asarray(f.pixels).reshape(-1) > 0)).mean())
    print("blended share:", share)
    assert share["sparse"] < api._DENSE_SHARE < share["dense"], share


def test_adam_twin_freezes_zero_gradient_columns():
    """torch.optim.Adam(eps=1e-15), five steps whose gradient is zero in the columns from 3 on: those columns keep their bits
    and their moments stay exact zeros, the others move, and `step` counts every step."""
    g = torch.Generator().manual_seed(1)
    state = {"f_rest_color": dict(param=torch.randn((40, 15, 3), generator=g), exp_avg=None, exp_avg_sq=None, step=None)}
    first = state["f_rest_color"]["param"].clone()
    for it in range(5):
        grad = torch.randn((40, 15, 3), generator=g) * 1e-6
        grad[:, 3:] = 0.0
        grad[0, 5, 1] = -0.0             # (a negative zero is a zero)
        state = L.adam_twin_step(state, {"f_rest_color": grad}, {"f_rest_color": 1e-4})
        s = state["f_rest_color"]
        assert s["step"] == it + 1.0
        assert torch.equal(s["param"][:, 3:], first[:, 3:]) and not s["exp_avg"][:, 3:].any() and not s["exp_avg_sq"][:, 3:].any()
        assert bool((s["param"][:, :3] != first[:, :3]).all())
    stale = torch.zeros((40, 15, 3))
    stale[7, 9, 2] = 1e-12               # ... and what the exact zero is for: a stale 1e-12 is a whole step of the rate
    moved = L.adam_twin_step(state, {"f_rest_color": stale}, {"f_rest_color": 1e-4})["f_rest_color"]["param"]
    assert abs(float(moved[7, 9, 2] - first[7, 9, 2])) > 0.5e-4


def test_degree_schedule():
    assert [degree_of(it) for it in range(1, ITERATIONS + 1)] == [0] * 4 + [1] * 5 + [2] * 7 + [3] * 6
    assert degree_of(EVENT_AFTER) == degree_of(EVENT_AFTER + 1) == 2              # the event lies inside a degree phase
    assert [first_inactive(D) for D in range(4)] == [0, 3, 8, 15] and bands(2) == {1: slice(0, 3), 2: slice(3, 8)}




# ---- GPU -------------------------------------------------------------------------------------------------------------------
FIRST_OF_DEGREE = {it: degree_of(it) for it in range(2, ITERATIONS + 1) if degree_of(it) != degree_of(it - 1)}      # {5: 1, 10: 2, 17: 3}


class _Frozen:
    """What both loops share: the inactive columns of the rest tensors on every iteration, the bands on a checked step."""

    def start(self):
        self.band_maxima = {}
        self.rebase()

    def rebase(self):
        """The bits an inactive coefficient has to keep: those of iteration 0, after the event those the event left."""
        self.base = {n: getattr(self.pc, L.ATTR[n]).detach().cpu().clone() for n in REST}

    def frozen_columns(self, kept, after, what):
        lo = first_inactive(self.D)
        for n in REST:
            grad = kept["grads"][n].cpu()
            assert grad.shape == self.base[n].shape and grad.shape[1] == 15, (what, n)
            assert not grad[:, lo:].any(), (what, n, "gradient of an inactive coefficient", float(grad[:, lo:].abs().max()))
            assert torch.equal(after[n]["param"][:, lo:], self.base[n][:, lo:]), (what, n, "an inactive coefficient moved")
            for k in ("exp_avg", "exp_avg_sq"):
                assert not after[n][k][:, lo:].any(), (what, n, k, float(after[n][k][:, lo:].abs().max()))
            assert after[n]["step"] == float(self.it), (what, n, after[n]["step"])

    def check_bands(self, before, kept, f, ref, what):
        D = self.D
        got = {n: kept["grads"][n].cpu().numpy() for n in REST + tuple(DC.values())}
        errs = band_errors(got, ref, D)
        print("%s: bands, error / band max-norm (band max-norm): %s"
              % (what, {"%s l=%d" % k: "%.3g (%.3g)" % em for k, em in errs.items()}))
        for k, (e, m) in errs.items():
            self.band_maxima[k] = max(self.band_maxima.get(k, 0.0), e)
            assert m > 0 and e < BAND_TOL, (what, k, e, m)
        if FIRST_OF_DEGREE.get(self.it) != D:
            return
        # the first step of a degree: the new band has a gradient on every blended Gaussian -- unless the clamp of its colour
        # (all three channels) or of its amplitude cut it off --, on no other row, and the step moves exactly those rows
        sl = bands(D)[D]
        P = got["f_rest_color"].shape[0]
        blended = (np.asarray(f.radii) > 0) & (np.asarray(f.pixels).reshape(-1) > 0)
        clamped = np.asarray(f.geom["clamped"]).astype(bool).reshape(P, -1)
        clamped_p = np.asarray(f.geom["clamped_p"]).astype(bool).reshape(-1)
        after = L.optimizer_state(self.pc)
        for n, expected in (("f_rest_color", blended & ~clamped.all(1)), ("amp_f_rest", blended & ~clamped_p), ("phase_f_rest", None)):
            rows = np.abs(ref[n][:, sl]).reshape(P, -1).max(1) > 0
            mine = np.abs(got[n][:, sl]).reshape(P, -1).max(1) > 0
            assert np.array_equal(mine, rows), (what, n, "rows with a gradient in the new band", int((mine != rows).sum()))
            assert not rows[~blended].any() and int(rows.sum()) > 100, (what, n, int(rows.sum()))
            if expected is not None:
                assert np.array_equal(rows, expected), (what, n, int((rows != expected).sum()))
            moved = (after[n]["param"][:, sl] != before[n]["param"][:, sl]).flatten(1).any(1).numpy()
            assert np.array_equal(moved, rows), (what, n, "rows of the new band that the step moved", int((moved != rows).sum()))


class _StaticLoop(_Frozen, TD._Loop):
    def __init__(self, mode, dev, oracle, spread):
        TD._Loop.__init__(self, mode, dev, oracle, spread, degrees=degree_of)
        self.start()

    def every_iteration(self, before, kept, after, what):
        self.frozen_columns(kept, after, what)

    def checked_step(self, before, kept, f, ref, what):
        self.check_bands(before, kept, f, ref, what)

    def event(self, kind):
        TD._Loop.event(self, kind)
        self.rebase()


def _steps_taken(optimizer, iterations):
    for g in optimizer.param_groups:             # every group that learns has taken every step, frozen columns or not
        st = optimizer.state.get(g["params"][0], None)
        if g["name"] in ("f_seg_color", "phase_offset"):
            assert not st, g["name"]
        else:
            assert float(st["step"]) == float(iterations), (g["name"], float(st["step"]))


def _run_static(mode, dev, oracle, scene):
    from gftorf_amd import api
    loop = _StaticLoop(mode, dev, oracle, TD.SCENES[scene])
    n_checked = 3 if mode == "graph" else 2              # graph: two eager iterations and the first replay of (shape, degree)
    replays, shapes = {}, [loop.P]
    while loop.it < ITERATIONS:
        D = loop.next_degree()
        checked = loop.in_shape < n_checked
        if loop.iteration(checked) and checked:
            replays[(loop.P, D)] = replays.get((loop.P, D), 0) + 1
        if loop.it == EVENT_AFTER:
            loop.event("densify_fused")
            shapes.append(loop.P)
    torch.cuda.synchronize()
    print("observed band maxima (%s, %s): %s" % (scene, mode, {"%s l=%d" % k: float("%.3g" % v) for k, v in sorted(loop.band_maxima.items())}))
    assert len(shapes) == 2 and shapes[1] != 1500 and max(shapes) <= 4000, shapes
    _steps_taken(loop.pc.optimizer, ITERATIONS)
    assert len(api.state.grad_pool) <= 8 and len(api.state.acc_pool) <= 8 and len(api.state.status) <= api.state.MAX_SHAPES
    backwards = {}
    for fr in loop.frames:
        if fr["backward"] and not fr["captured"]:
            backwards.setdefault(fr["P"], []).append(fr)
    print("gradient sets (degree, reused, row by row) per eager backward:",
          {P: [(f["D"], int(f["reused"]), int(f["rows_only"])) for f in v] for P, v in backwards.items()})
    assert set(backwards) == set(shapes)
    for P, v in backwards.items():
        # one kept set per shape goes through every degree: each eager backward but the shape's first takes it
        assert not v[0]["reused"] and all(f["reused"] for f in v[1:]), (P, v)
        steps = [b for a, b in zip(v, v[1:]) if a["D"] != b["D"]]
        assert len(steps) == (2 if P == 1500 else 1), (P, v)        # 0 -> 1 -> 2 before the event, 2 -> 3 after it
        if scene == "sparse":
            assert all(f["rows_only"] for f in v[1:]), (P, v)       # ... row by row, the degree steps included
        else:
            assert any(not f["rows_only"] for f in v[1:]), (P, v)   # ... and in full once its probe has reported
    if mode == "graph":           # a checked replay in every degree phase, before and after the event
        phases = [(1500, 0), (1500, 1), (1500, 2), (shapes[1], 2), (shapes[1], 3)]
        assert all(replays.get(k, 0) >= 1 for k in phases), replays
    assert not any(x["overflow"] or x["overflows"] for x in api.enqueue_status())


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(TD.SCENES))
@pytest.mark.parametrize("mode", ["eager", "no_host_read", "graph"])
def test_loop_across_the_sh_degree_schedule(mode, scene, oracle, gpu):
    from gftorf_amd import api
    flags = {k: getattr(api, k) for k in TD.API_FLAGS}
    api.state.reset()
    try:
        api.no_host_read = mode == "no_host_read"
        _run_static(mode, gpu, oracle, scene)
    finally:
        for k, v in flags.items():
            setattr(api, k, v)
        api.state.reset()


# ---- the dynamic loop -------------------------------------------------------------------------------------------------------
class _DynamicLoop(_Frozen, TY._Loop):
    def __init__(self, mode, dev, oracle):
        TY._Loop.__init__(self, mode, "torf", dev, oracle, degrees=degree_of)
        self.start()
        self.net_base = {k: v["param"] for k, v in TY.network_state(self.net, self.opt_net).items()}

    def every_iteration(self, before, kept, after, net_grads, net_after, what):
        self.frozen_columns(kept, after, what)
        # the r / g / b heads: row k makes coefficient k (oracle/deform_ref.py forward: d_sh = stack(r, g, b) of [n, 16])
        k0 = (self.D + 1) ** 2
        for h in RGB_HEADS:
            for s in (".weight", ".bias"):
                name = h + s
                assert net_grads[name].shape[0] == 16 and net_grads[name][:k0].any(), (what, name)
                assert not net_grads[name][k0:].any(), (what, name, "gradient of an inactive head row", float(net_grads[name][k0:].abs().max()))
                assert torch.equal(net_after[name]["param"][k0:], self.net_base[name][k0:]), (what, name, "an inactive head row moved")
                for k in ("exp_avg", "exp_avg_sq"):
                    assert not net_after[name][k][k0:].any(), (what, name, k)
                assert net_after[name]["step"] == float(self.it), (what, name)

    def checked_step(self, before, kept, f, ref, what):
        self.check_bands(before, kept, f, ref, what)
        if self.n:                    # the reference's gradient on the network's d_sh: exact zeros where the heads' are asserted
            assert not ref["d_sh"][:, (self.D + 1) ** 2:].any() and np.abs(ref["d_sh"][:, :(self.D + 1) ** 2]).max() > 0, what

    def event(self, kind):
        TY._Loop.event(self, kind)
        self.rebase()


def _run_dynamic(mode, dev, oracle):
    from gftorf_amd import api
    loop = _DynamicLoop(mode, dev, oracle)
    n_checked = 3 if mode == "graph" else 2
    replays, shapes = {}, [(loop.P, loop.n)]
    while loop.it < ITERATIONS:
        D = loop.next_degree()
        checked = loop.in_shape < n_checked
        if loop.iteration(checked) and checked:
            replays[(loop.P, D)] = replays.get((loop.P, D), 0) + 1
        if loop.it == EVENT_AFTER:
            loop.event("densify")
            shapes.append((loop.P, loop.n))
    torch.cuda.synchronize()
    print("shapes (P, n):", shapes)
    print("observed maxima (torf, %s): %s; bands %s" % (mode, {k: float("%.3g" % v) for k, v in sorted(loop.maxima.items())},
                                                        {"%s l=%d" % k: float("%.3g" % v) for k, v in sorted(loop.band_maxima.items())}))
    assert len(shapes) == 2 and shapes[1][0] != 1500 and 0 < shapes[1][1] < shapes[1][0] <= 4000, shapes
    _steps_taken(loop.pc.optimizer, ITERATIONS)
    assert loop.net_steps == ITERATIONS
    assert len(api.state.grad_pool) <= 8 and len(api.state.acc_pool) <= 8 and len(api.state.status) <= api.state.MAX_SHAPES
    assert not any(x["overflow"] or x["overflows"] for x in api.enqueue_status())
    if mode == "graph":
        phases = [(1500, 0), (1500, 1), (1500, 2), (shapes[1][0], 2), (shapes[1][0], 3)]
        assert all(replays.get(k, 0) >= 1 for k in phases), replays


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_dynamic_loop_across_the_sh_degree_schedule(mode, oracle, gpu):
    from gftorf_amd import api, deform as D
    flags = {k: getattr(api, k) for k in TY.API_FLAGS}
    rows_from = D._SPARSE_MIN_POINTS
    api.state.reset()
    try:
        D._SPARSE_MIN_POINTS = 1          # as tests/test_loop_dynamic.py: the row-counting backward at this test's row counts
        _run_dynamic(mode, gpu, oracle)
    finally:
        D._SPARSE_MIN_POINTS = rows_from
        for k, v in flags.items():
            setattr(api, k, v)
        api.state.reset()
