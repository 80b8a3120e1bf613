"""The device on degenerate Gaussians (helpers.hostile_scene: what its rows are and that each is what its name says is
tests/test_hostile_rows.py's business, on the CPU) and on extreme frame shapes.

  * stages: test_gpu_parity.py's bit-exact measure of preprocess and binning, in both binning modes;
  * forward and backward: check_outputs / check_grads unchanged, then ROW BY ROW -- every named row's error against float64
    (tests/torch_ref.py), relative to that row's own max-norm, at most max(2 x the oracle's error on that row, GRAD_RTOL); the
    oracle's errors are recomputed here, on this host.  Every gradient finite; every row the oracle leaves at an exact zero an
    exact zero on the device;
  * under both forward kernels (gft_set_render_mode 0 / 1), under the deterministic backward (a child process), with the
    covariances and with the colours precomputed, and through the feature blend (flow.render_flows, C = 3 and C = 6);
  * frames of 1 x 1 .. 4112 x 16: a grid dimension of one tile, a tile with one live pixel row or column, a quadrant without
    a pixel, a tile index above 255.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as Hh
from test_flow_render import _geometry, _ours, _reference_pair, _rel
from test_gpu_parity import (GRAD_RTOL, binning_mode, check_grads, check_outputs, check_preprocess_and_binning_bit_exact,
                             render_mode)

pytestmark = pytest.mark.gpu

TENSORS = Hh.ROW_TENSORS + ("colors_precomp", "cov3D_precomp")


def check_rows(tag, scene, rows, ref, b, grads, inputs=None):
    """The row-by-row measure (module docstring).  ref: float64; b: the oracle's backward; grads: the device's."""
    want = Hh.oracle_grads(b, scene, inputs)
    eo, ed = Hh.row_errors(ref, want, rows), Hh.row_errors(ref, grads, rows)
    bad, worst = [], {}
    for k in TENSORS:
        if grads.get(k) is not None:
            assert np.isfinite(grads[k]).all(), "%s: non-finite dL/d%s" % (tag, k)
    for (n, k), (err, own, _) in ed.items():
        err_o = eo[(n, k)][0]
        if own > 0 and err / own > worst.get(k, (0.0,))[0]:
            worst[k] = (err / own, err_o / own, n)
        if not err <= max(2.0 * err_o, GRAD_RTOL * own):
            bad.append("%s %s %s: error %.3g (%.3g of the row's max %.3g), the oracle's %.3g" % (tag, n, k, err, err / max(own, 1e-300), own, err_o))
    print("\n[hostile] %s, worst row per tensor, device (oracle): %s" % (
        tag, ", ".join("%s %.2g (%.2g) %s" % ((k,) + worst[k]) for k in TENSORS if k in worst)))
    # rows that the oracle leaves at an exact zero: culled, blending nothing, below the alpha threshold
    for k in TENSORS:
        if grads.get(k) is None or want.get(k) is None:
            continue
        w, g_ = want[k].reshape(want[k].shape[0], -1), grads[k].reshape(want[k].shape[0], -1)
        zero = ~w.any(1)
        assert zero.sum() >= 6, k
        if g_[zero].any():
            names = {i: n for n, i in rows.items()}
            bad.append("%s %s: rows %s are not exact zeros" % (tag, k, [names.get(i, i) for i in np.flatnonzero(zero & g_.any(1))]))
    assert not bad, "\n".join(bad)


def forward_backward(oracle, gpu, variant=None):
    sc, rows, f, ref, inputs = Hh.hostile_reference(oracle, variant)
    b = Hh.run_oracle(oracle, sc, inputs=inputs)[1]
    out, grads, _ = Hh.run_gpu(sc, gpu, inputs=inputs, optimize_offsets=True)
    return sc, rows, f, ref, inputs, b, out, grads


def check_everything(tag, sc, rows, f, ref, inputs, b, out, grads):
    check_outputs(f, out)
    check_grads(b, grads, dict(sc, gaussians=dict(sc["gaussians"], **(inputs or {}))))
    check_rows(tag, sc, rows, ref, b, grads, inputs)


@pytest.mark.parametrize("mode", [1, 0], ids=["tile_pull", "whole_frame"])
def test_stages_bit_exact(mode, oracle, gpu):
    """radii, rects, tile counts, R, keys, lists, conics and depth bits: the rows whose rectangle ends exactly on a tile edge,
    the giant's clamped rectangle, the clones' order among equal keys."""
    sc, rows = Hh.hostile_scene(oracle)
    check_preprocess_and_binning_bit_exact(sc, mode, oracle, gpu)


@pytest.mark.parametrize("mode", [0, 1], ids=["one_wave_per_quadrant", "segmented"])
def test_rows_against_float64(mode, oracle, gpu):
    with render_mode(mode):
        res = forward_backward(oracle, gpu)
    check_everything("render mode %d" % mode, *res)
    sc, rows, f = res[:3]
    out = res[6]
    # the alpha threshold, on the device's own counters: one float below blends nowhere, 1/255 itself and one float above
    # blend their one pixel
    pix = out["pixels"].reshape(-1)
    assert pix[rows["thr_below"]] == 0 and pix[rows["thr_exact"]] == 1 and pix[rows["thr_above"]] == 1
    np.testing.assert_array_equal(pix[sorted(rows.values())], f.pixels.reshape(-1)[sorted(rows.values())])


@pytest.mark.parametrize("mode", [0, 1], ids=["one_wave_per_quadrant", "segmented"])
def test_rows_under_the_deterministic_backward(mode, tmp_path, oracle):
    """GFT_BWD_DETERMINISTIC=1 is read when the library loads: a child process, as test_deterministic_backward_mode's."""
    child, res = tmp_path / "det.py", tmp_path / "det.npz"
    here = os.path.dirname(os.path.abspath(__file__))
    child.write_text(
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import helpers\n"
        "from oracle import oracle\n"
        "from gftorf_amd import _lib\n"
        "sc, rows = helpers.hostile_scene(oracle)\n"
        "_lib.load().gft_set_render_mode(%d)\n"
        "o, g, t = helpers.run_gpu(sc, torch.device('cuda:0'), optimize_offsets=True)\n"
        "res = {'g_' + k: v for k, v in g.items() if v is not None}\n"
        "res.update({'o_' + k: v for k, v in o.items()})\n"
        "np.savez(%r, **res)\n" % (os.path.dirname(here), here, mode, str(res)))
    subprocess.check_call([sys.executable, str(child)], env=dict(os.environ, GFT_BWD_DETERMINISTIC="1"), timeout=300)
    got = np.load(res)
    grads = {k[2:]: got[k] for k in got.files if k.startswith("g_")}
    out = {k[2:]: got[k] for k in got.files if k.startswith("o_")}
    sc, rows, f, ref, inputs = Hh.hostile_reference(oracle)
    b = Hh.run_oracle(oracle, sc)[1]
    check_everything("deterministic backward, render mode %d" % mode, sc, rows, f, ref, inputs, b, out, grads)


@pytest.mark.parametrize("variant", ["cov3D_precomp", "colors_precomp"])
def test_rows_with_precomputed_inputs(variant, oracle, gpu):
    res = forward_backward(oracle, gpu, variant)
    sc, rows, f, ref, inputs = res[:5]
    if variant == "cov3D_precomp":
        c = inputs["cov3D_precomp"]
        assert not c[rows["zero3"]].any() and c[rows["q_large"]].any()
        m = np.array([[c[rows["zero1"], a] for a in r] for r in ((0, 1, 2), (1, 3, 4), (2, 4, 5))], np.float64)
        assert abs(np.linalg.det(m)) < 1e-5 * np.abs(m).max() ** 3                      # a collapsed axis: singular to fp32 rounding
    else:
        c = inputs["colors_precomp"]
        assert (c < 0).any() and (c > 1).any()
    check_everything(variant, *res)


@pytest.mark.parametrize("binning", [0, 1], ids=["whole_frame", "tile_pull"])
def test_feature_blend_on_hostile_geometry(binning, oracle, gpu):
    """flow.render_flows (C = 3, and the pair's C = 6 route) against two GaussianRasterizer(colors_precomp=...) calls, by
    test_flow_render.py's measure and bounds; zero gradient rows for every Gaussian that is culled or blended nowhere."""
    sc, rows, f, _, _ = Hh.hostile_reference(oracle)
    P, W, H = Hh.HOSTILE_P, Hh.HOSTILE_W, Hh.HOSTILE_H
    geo = _geometry(sc, gpu)
    settings = Hh.gpu_settings(sc, gpu)
    gen = torch.Generator().manual_seed(P + binning)
    fa, fb = ((0.05 * torch.randn((P, 3), generator=gen)).to(gpu) for _ in range(2))
    ga, gb = (torch.randn((3, H, W), generator=gen).to(gpu) for _ in range(2))
    with binning_mode(binning), render_mode(0):      # (the bounds are those of frames drawn by one wave per quadrant)
        ia, ib, dfa, dfb = _ours(settings, geo, fa, fb, ga, gb)
        (ra, rb), (gra, grb), radii = _reference_pair(settings, geo, fa, fb, ga, gb)
        ia1, ib1, dfa1, dfb1 = _ours(settings, geo, fa, None, ga, None)
    torch.cuda.synchronize()
    print("\n[hostile] features, binning %d: image_b %.3g, grad a %.3g, grad b %.3g, grad a (C = 3) %.3g"
          % (binning, _rel(rb, ib), _rel(gra, dfa), _rel(grb, dfb), _rel(gra, dfa1)))
    assert torch.equal(ia, ra) and torch.equal(ia1, ra) and ib1 is None and dfb1 is None
    assert float(rb.abs().max()) > 0 and _rel(rb, ib) <= 1e-6
    assert _rel(gra, dfa) <= 1e-5 and _rel(grb, dfb) <= 1e-5 and _rel(gra, dfa1) <= 1e-5
    np.testing.assert_array_equal(radii.cpu().numpy(), f.radii)
    nothing = torch.tensor((f.radii == 0) | (f.pixels.reshape(-1) == 0), device=gpu)
    assert int(nothing.sum()) >= 6
    for g_ in (dfa, dfb, dfa1, gra, grb):
        assert bool(torch.isfinite(g_).all()) and float(g_[nothing].abs().max()) == 0.0


FRAMES = [(1, 1), (1, 40), (40, 1), (15, 15), (16, 16), (17, 17), (16, 2064), (4112, 16)]      # W, H


@pytest.mark.parametrize("W,H", FRAMES, ids=["%dx%d" % wh for wh in FRAMES])
def test_frame_shapes(W, H, oracle, gpu):
    """The smallest frames with a grid dimension of one tile, a tile with one live pixel row or column (1 x 40, 17 x 17,
    4112 = 257 x 16), a quadrant with no pixel inside (every frame narrower or lower than 9) and a tile index above 255
    (gx = 257); gy = 129 for the transposed walk."""
    sc = Hh.frame_scene(W, H)
    for mode in (1, 0):
        check_preprocess_and_binning_bit_exact(sc, mode, oracle, gpu)
    f, b = Hh.run_oracle(oracle, sc)
    assert f.radii[0] > 8 * min(W, H) and f.num_rendered >= 200
    out, grads, _ = Hh.run_gpu(sc, gpu, optimize_offsets=True)
    check_outputs(f, out)
    check_grads(b, grads, sc)
    assert all(np.isfinite(v).all() for v in grads.values() if v is not None)
    geo = _geometry(sc, gpu)
    settings = Hh.gpu_settings(sc, gpu)
    gen = torch.Generator().manual_seed(W + H)
    fa = (0.05 * torch.randn((200, 3), generator=gen)).to(gpu)
    ga = torch.randn((3, H, W), generator=gen).to(gpu)
    with render_mode(0):
        ia, _, dfa, _ = _ours(settings, geo, fa, None, ga, None)
        (ra, _), (gra, _), radii = _reference_pair(settings, geo, fa, fa, ga, ga)
    torch.cuda.synchronize()
    assert torch.equal(ia, ra) and float(gra.abs().max()) > 0 and _rel(gra, dfa) <= 1e-5, _rel(gra, dfa)
    assert float(dfa[radii == 0].abs().max() if bool((radii == 0).any()) else 0.0) == 0.0
