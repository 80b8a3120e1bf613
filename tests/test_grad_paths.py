"""Every path of the rasterizer backward, on the CPU: the float64 re-derivation (tests/torch_ref.py) names the eight uses
of a Gaussian's position (torch_ref.PATHS), helpers.float64_case_grads splits dL/dmeans3D into one term per use, and the
oracle's hand-written backward is held to every term -- not to the largest one, which is all a whole-tensor max-norm sees
(the projected mean is 0.99 of |dL/dmeans3D|_inf in small_scene(); the d_ndc term 0.00024 .. 0.0014, below the 3e-4 bound).

What is checked here, so that tests/test_gpu_grad_paths.py (the same measure on the device, at ten times these bounds)
cannot go blind:
  * closure: for every single upstream plane the eight parts sum to the full gradient (1e-12), and each part equals the
    full gradient minus the one with that use detached (settings["detach"]);
  * the scene (helpers.path_scene): every path that exists for a plane is at least 0.05 of that plane's |dL/dmeans3D|_inf,
    clamped colour channels and clamped amplitudes occur, no discrete decision of the walk sits on its edge, no SH sum
    sits on its clamp;
  * the oracle through the measure (helpers.check_path_case) at GRAD_RTOL / 10 = 3e-5, in every variant and upstream
    case the GPU file runs, and row by row on isolated Gaussians (helpers.isolated_scene).

Measured (float64 against the oracle's fp32; error / yardstick, to be compared with 3e-5):
  dL/dmeans3D against its smallest path: 7e-7 .. 6.5e-6 in the single-plane cases, 1.7e-5 in "all" (there the smallest
  path, d_ndc, is 0.030 of the max-norm; against the max-norm the same error is 5e-7), 1.1e-5 at worst in the variants;
  SH columns <= 1.5e-6, every other tensor <= 2.5e-6 of its max-norm, the offsets <= 4e-7 of their terms;
  isolated Gaussians: 1.4e-5 of a row's own max at worst (means2D; a row is a sum of some twenty pixels with N(0, 1)
  upstream values of both signs).

Teeth (scratch copies): the oracle without the dL_dndc term of dL_dmeans3D, and with one degree-3
direction derivative (d/dz of coefficient 11) scaled by 1.1.  test_oracle_autograd.py::test_sh_paths[3-16] catches both at
its own 5e-5 -- 2.4e-4 and 9.0e-5 of |dL/dmeans3D|_inf, so by 4.8x and 1.8x, and neither at the device tests' 3e-4 -- while
this file fails by 1.9 / 1.0 (depth_distortion, all: the whole smallest path is missing) and by 1.7e-2 .. 0.28 of the
smallest path against a bound of 3e-5.
"""
import numpy as np
import pytest
import torch

import helpers as Hh
import torch_ref
from test_gpu_parity import GRAD_RTOL

ORACLE_RTOL = GRAD_RTOL / 10.0
SINGLE_PLANES = ("color", "phasor", "depth", "acc", "depth_distortion")
MIN_SHARE = 0.05
VARIANT_CASES = [(v, c) for v in Hh.PATH_VARIANTS for c in Hh.path_variant(v)[2]]


def base_reference(oracle):
    """The base scene's references for the GPU cases and the whole phasor plane, computed once."""
    return Hh.path_reference("base", oracle)


@pytest.mark.parametrize("plane", SINGLE_PLANES)
def test_parts_sum_to_the_full_gradient(plane, oracle):
    scene, _, f, ref = base_reference(oracle)
    r = ref[plane]
    full = float(np.abs(r["means3D"]).max())
    total = sum(r["parts"][p] for p in torch_ref.PATHS)
    assert float(np.abs(total - r["means3D"]).max()) <= 1e-12 * full
    shares = {p: float(np.abs(r["parts"][p]).max()) / full for p in torch_ref.PATHS}
    print("\n[paths] %s: %s" % (plane, ", ".join("%s %.3g" % (p, s) for p, s in shares.items() if s)))
    for p in torch_ref.PATHS:
        if p in Hh.CASE_PATHS[plane]:
            assert shares[p] >= MIN_SHARE, "%s: path %s is %.3g of |dL/dmeans3D|_inf" % (plane, p, shares[p])
        else:
            assert shares[p] == 0.0, "%s: path %s should not exist" % (plane, p)


@pytest.mark.parametrize("path", torch_ref.PATHS)
def test_part_is_full_minus_detached(path, oracle):
    """settings["detach"] = {path} removes exactly that term: under the upstream of every plane together the full gradient
    minus the detached one is the part that float64_case_grads took from dL/d(use); nothing else moves."""
    scene, _, f, ref = base_reference(oracle)
    r = ref["all"]
    dt = torch.float64
    params = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in scene["gaussians"].items()}
    for k in ("colors_precomp", "phasors_precomp", "cov3D_precomp"):
        params[k] = None
    params["phase_offset"] = torch.tensor(scene["phase_offset"], dtype=dt, requires_grad=True)
    params["dc_offset"] = torch.tensor(scene["dc_offset"], dtype=dt, requires_grad=True)
    out = torch_ref.render(params, f, Hh.oracle_kwargs(scene, detach={path}))
    sum((out[k] * torch.tensor(scene["grads"][k], dtype=dt)).sum() for k in Hh.GRAD_KEYS).backward()
    full = float(np.abs(r["means3D"]).max())
    detached = params["means3D"].grad.numpy()
    assert float(np.abs((r["means3D"] - detached) - r["parts"][path]).max()) <= 1e-12 * full
    for k in ("opacities", "scales", "rotations", "shs", "shs_p"):        # the other inputs' gradients do not pass through means3D
        assert float(np.abs(params[k].grad.numpy() - r[k]).max()) <= 1e-12 * float(np.abs(r[k]).max()), k


def test_default_render_is_untouched(oracle):
    """Without "detach" and "split_uses" the tensors at the cuts are the ones that were there before the cuts had names
    (no view, no detach: the graph is the old one); with "split_uses" the outputs are the same bits."""
    scene, _, f, _ = base_reference(oracle)
    dt = torch.float64
    params = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in scene["gaussians"].items()}
    for k in ("colors_precomp", "phasors_precomp", "cov3D_precomp"):
        params[k] = None
    params["phase_offset"] = torch.tensor(scene["phase_offset"], dtype=dt)
    params["dc_offset"] = torch.tensor(scene["dc_offset"], dtype=dt)
    a = torch_ref.render(params, f, Hh.oracle_kwargs(scene))
    u = a["uses"]
    assert set(u) == set(torch_ref.PATHS)
    assert u["dir_color"][0] is u["dir_phasor"][0]                                           # `dirs` itself, twice
    assert u["dist_phase"][0] is u["dist_factor"][0] is u["dist_depth"][0] is u["dist_ndc"][0]   # `dist` itself
    assert all(t.grad_fn is not None and "View" not in type(t.grad_fn).__name__ for ts in u.values() for t in ts)
    with torch.no_grad():
        b = torch_ref.render(params, f, Hh.oracle_kwargs(scene, split_uses=True))
    for k in Hh.GRAD_KEYS:
        assert torch.equal(a[k].detach(), b[k]), k


def _sh_sums(scene, D):
    """float64 SH sums + 0.5 of the colour channels [P, 3] and of the amplitude [P], before their clamp at 0."""
    dt = torch.float64
    g = scene["gaussians"]
    d = torch.tensor(g["means3D"], dtype=dt) - torch.tensor(np.asarray(scene["cam"]["campos"]).reshape(3), dtype=dt)
    d = d / d.norm(dim=1, keepdim=True)
    rgb = torch_ref.sh_poly(D, torch.tensor(g["shs"], dtype=dt), d) + 0.5
    amp = (torch_ref.sh_poly(D, torch.tensor(g["shs_p"], dtype=dt), d) + 0.5)[:, 1]
    return rgb.numpy(), amp.numpy()


def test_path_scene_conditions(oracle):
    scene, _, f, _ = base_reference(oracle)
    blended = (f.radii > 0) & (f.pixels.reshape(-1) > 0)
    n_color = int((blended & f.geom["clamped"].any(1)).sum())
    n_amp = int((blended & (f.geom["clamped_p"] > 0)).sum())
    print("\n[scene] blended %d, clamped colour channel %d, clamped amplitude %d" % (int(blended.sum()), n_color, n_amp))
    assert int(blended.sum()) >= 100 and n_color >= 10 and n_amp >= 10
    # Beyond the 1.3 tanfov clamp of computeCov2D: this scene has no such Gaussian on screen -- its principal point is at
    # 0.4 W, so the image ends at 1.2 tanfov -- and does not need one: x_grad_mul = 0 for a blended Gaussian inside the image
    # is held by test_oracle_autograd.py::test_sensor_cameras[shift_right / shift_corner] (oracle against float64) and by
    # test_gpu_parity.py::test_forward_backward_vs_oracle[wide_spread@shift_right / wide_spread@shift_corner] (device), where
    # the cov_t path is all that is left of such a Gaussian's covariance gradient and so is the largest term, not a small one.
    assert not Hh.beyond_the_clamp_on_screen(scene, f).any()
    # no discrete decision on its edge (the float64 reference blends the oracle's lists: a pair that the oracle skips and
    # float64 would not, or the other way round, is not a rounding difference)
    mg = {}
    dt = torch.float64
    params = {k: torch.tensor(v, dtype=dt) for k, v in scene["gaussians"].items()}
    for k in ("colors_precomp", "phasors_precomp", "cov3D_precomp"):
        params[k] = None
    params["phase_offset"] = torch.tensor(scene["phase_offset"], dtype=dt)
    params["dc_offset"] = torch.tensor(scene["dc_offset"], dtype=dt)
    with torch.no_grad():
        out = torch_ref.render(params, f, Hh.oracle_kwargs(scene, margins=mg))
    print("[scene] margins: |alpha - 1/255| %.3g, |power| %.3g, |test_T - 1e-4| %.3g" % (mg["alpha"], mg["power"], mg["test_T"]))
    assert mg["alpha"] > 1e-4 / 255.0
    assert mg["power"] > 1e-6
    assert mg["test_T"] > 1e-7
    for k in Hh.GRAD_KEYS:           # ... so the two forwards agree to fp32 rounding, with no pixel left out
        Hh.assert_close("fwd " + k, out[k].numpy(), f[k], rtol_max=2e-5, atol=1e-6)
    # no SH sum on its clamp, at any degree the variants use; the oracle's bits are the float64 decisions
    for D in (1, 2, 3):
        sc = Hh.path_scene(D=D)
        fD, _ = Hh.run_oracle(oracle, sc, backward=False)
        rgb, amp = _sh_sums(sc, D)
        assert float(np.abs(rgb).min()) > 1e-5 and float(np.abs(amp).min()) > 1e-5, D
        vis = fD.radii > 0
        np.testing.assert_array_equal(fD.geom["clamped"][vis].astype(bool), rgb[vis] < 0)
        np.testing.assert_array_equal(fD.geom["clamped_p"][vis].astype(bool), amp[vis] < 0)


@pytest.mark.parametrize("variant,case", VARIANT_CASES)
def test_oracle_through_the_path_measure(variant, case, oracle):
    scene, inputs, f, ref = base_reference(oracle) if variant == "base" else Hh.path_reference(variant, oracle)
    r = ref[case]
    paths = Hh.case_paths(case, scene, inputs)
    for p in torch_ref.PATHS:
        assert bool(np.abs(r["parts"][p]).max() > 0) == (p in paths), "%s %s: path %s" % (variant, case, p)
    if variant == "no_vdp":          # the SH phase is not used: its columns are exact zeros; the amplitude still carries the direction
        assert not r["shs_p"][:, :, 0].any() and r["shs_p"][:, :, 1].any()
    got = Hh.oracle_case_grads(oracle, scene, f, case, inputs)
    ratios, bad = Hh.check_path_case("oracle", case, r, got, paths, ORACLE_RTOL, f=f, D=scene["cfg"]["D"])
    print("\n[oracle] %s %s: %s" % (variant, case, ", ".join("%s %.2g" % kv for kv in ratios.items())))
    assert not bad, "\n".join(bad)


def test_isolated_gaussians_row_by_row(oracle):
    scene, _, f, ref = Hh.path_reference("isolated", oracle)
    r = ref["all"]
    # 3 sigma extents (the oracle's radii: ceil(3 sigma)) do not overlap, and every Gaussian is blended
    m2, rad = f.geom["means2D"].astype(np.float64), f.radii.astype(np.float64)
    assert (f.radii > 0).all() and (f.pixels.reshape(-1) > 0).all()
    for i in range(len(rad)):
        for j in range(i):
            assert max(abs(m2[i, 0] - m2[j, 0]), abs(m2[i, 1] - m2[j, 1])) >= rad[i] + rad[j], (i, j)
    op = scene["gaussians"]["opacities"]
    assert abs(float(op.min()) - 0.02) < 1e-6 and abs(float(op.max()) - 0.9) < 1e-6
    span = {k: np.abs(r[k].reshape(len(rad), -1)).max(1) for k in ("means3D", "means2D", "opacities", "scales", "rotations", "shs", "shs_p")}
    print("\n[isolated] decades of row max-norms: %s" % ", ".join("%s %.2f" % (k, np.log10(v.max() / v.min())) for k, v in span.items()))
    assert span["means3D"].max() >= 1e3 * span["means3D"].min()
    assert span["shs_p"].max() >= 1e3 * span["shs_p"].min()
    got = Hh.oracle_case_grads(oracle, scene, f, "all")
    ratios, bad = Hh.check_path_case("oracle", "all", r, got, (), ORACLE_RTOL, f=f, rows=True)
    print("[oracle] isolated: %s" % ", ".join("%s %.2g" % kv for kv in ratios.items()))
    assert not bad, "\n".join(bad)
