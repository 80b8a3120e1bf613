"""Degenerate Gaussians on the CPU: helpers.hostile_scene() -- collapsed axes, a needle, a pancake, a Gaussian that covers
the frame, unnormalised and zero quaternions, raw opacities (0, 1, above 1, negative, one float either side of 1/255), means
behind the camera, at the camera centre, on a pixel centre, on a tile corner and off the screen, tile rectangles that end
exactly on a tile edge, and bit-identical clones -- first held to what their names claim, then the oracle's hand-written
backward held to float64 autograd (tests/torch_ref.py) ROW BY ROW: a whole-tensor max-norm is set by one ordinary Gaussian
with a large gradient and sees none of these rows.

The measure (helpers.row_errors): every named row against its own max-norm in float64, all ordinary rows as one block
against the block's; a row whose float64 gradient is an exact zero (culled, blending nothing, below the alpha threshold) must
be an exact zero in the oracle.  The bound is 2 x MEASURED below: the oracle's own fp32 conditioning on that row as measured
when this file was written (never the device's), the factor for another compiler or libm.  tests/test_gpu_hostile.py holds the
device to the same rows.

MEASURED, worst tensor per row (error / the row's yardstick), see the table for every entry:
  thr_exact 5.1e-3 and thr_above 1.3e-3 (means2D, against the floor of helpers.row_errors: such a row's own gradient there is
  a rounding; 2.1e-4 and 2.5e-5 in means3D), needle 5.6e-5 (scales; 1.7e-5 means2D), pixel_centre 1.3e-5 (opacities), q_negw
  9.8e-6 (rotations), clones 8.7e-6 (shs_p), every other named row <= 8.2e-6, the ordinary block <= 1.9e-6.  Nothing is near
  the 1e-2 beyond which a row would be too ill-conditioned to be a yardstick, so no parameter was softened.  (The figures are
  those of this scene: moving one row changes what its neighbours in a tile list see.)

Teeth (scratch copies of the oracle): the rectangle's upper edge with + 16 (off_miss is no longer culled),
the alpha test with <= (thr_exact blends nowhere), and dL/dscales of the Gaussians that have a zero axis times 1.1 (zero1: 0.1
of its own max; the gradient of the zero axis itself is an exact zero on both sides, asserted below) each fail a named-row
assertion of this file.
"""
import numpy as np
import pytest

import helpers as Hh

T = Hh.ROW_TENSORS       # means3D, means2D, opacities, scales, rotations, shs, shs_p
# error / yardstick of the oracle against float64, per row and tensor in the order of T (0: an exact zero on both sides)
MEASURED = {
    "zero3": (9.8e-07, 1.1e-06, 1.1e-06, 0, 0, 7.8e-07, 1.1e-06),
    "zero1": (7.5e-07, 8.4e-07, 3.5e-07, 1.2e-07, 1.3e-07, 3.9e-07, 1e-06),
    "needle": (1.4e-05, 1.7e-05, 4.6e-07, 5.6e-05, 9e-06, 3.9e-07, 7.8e-07),
    "pancake": (2.2e-07, 2.9e-07, 1e-06, 8.4e-07, 1.1e-06, 6.6e-07, 5.4e-07),
    "giant": (1.8e-07, 1.6e-07, 7.6e-07, 1.4e-07, 1.2e-07, 7e-07, 1.6e-07),
    "q_small": (9.5e-07, 1.2e-06, 2.7e-07, 3e-06, 1.7e-06, 5.4e-07, 8.9e-07),
    "q_large": (3.7e-07, 2.2e-07, 9.1e-07, 2.1e-07, 3.6e-07, 3.2e-07, 6.3e-07),
    "q_zero": (4.7e-07, 7.5e-07, 5.4e-06, 3.3e-06, 0, 1.4e-07, 5.5e-07),
    "q_negw": (3e-07, 1.5e-07, 3.5e-06, 7.4e-06, 9.8e-06, 6.8e-08, 1e-06),
    "op_zero": (0, 0, 0, 0, 0, 0, 0),
    "op_one": (5.9e-07, 5e-07, 2.4e-07, 4.4e-07, 1.2e-06, 5.1e-07, 9.1e-07),
    "op_above_one": (8.2e-07, 1.3e-06, 1.7e-06, 3.3e-06, 2.5e-06, 3.1e-07, 2.5e-06),
    "op_negative": (0, 0, 0, 0, 0, 0, 0),
    "thr_below": (0, 0, 0, 0, 0, 0, 0),
    "thr_above": (2.5e-05, 0.0013, 1.3e-07, 3.7e-11, 2.2e-11, 2.9e-07, 4.3e-07),
    "thr_exact": (0.00021, 0.0051, 4.3e-08, 7.1e-10, 6.6e-10, 2.1e-07, 2.3e-07),
    "behind": (0, 0, 0, 0, 0, 0, 0),
    "at_camera": (0, 0, 0, 0, 0, 0, 0),
    "pixel_centre": (2.3e-07, 3.5e-07, 1.3e-05, 5.4e-06, 2.9e-06, 1.3e-07, 1.5e-06),
    "tile_corner": (7.9e-07, 7.3e-07, 1.9e-07, 2.4e-07, 8.1e-07, 1.1e-06, 5.8e-07),
    "off_one_tile_in": (5.3e-07, 6.8e-07, 6.8e-07, 6.2e-07, 6.4e-07, 3.8e-07, 1.5e-07),
    "off_miss": (0, 0, 0, 0, 0, 0, 0),
    "beyond_clamp": (1e-07, 8.5e-08, 1.5e-07, 2.5e-07, 1.5e-07, 6.1e-07, 1e-06),
    "rect_lo_exact": (3.5e-06, 2.3e-06, 2.6e-07, 2.8e-07, 2.4e-07, 3.7e-07, 3.8e-07),
    "rect_hi_exact": (7.2e-07, 8.8e-07, 9.8e-08, 2.9e-07, 9.2e-08, 4.4e-07, 6.6e-07),
    "rect_hi_touch": (1.7e-06, 1.6e-06, 2.8e-07, 3.8e-06, 8.9e-07, 4.2e-07, 8.2e-06),
    "clone_a0": (1.1e-06, 1.3e-06, 2e-07, 1.9e-06, 3.4e-06, 1.1e-06, 2e-06),
    "clone_a1": (1e-06, 1.2e-06, 3.2e-07, 2e-06, 3.6e-06, 2.2e-06, 3.4e-06),
    "clone_a2": (8.4e-07, 1e-06, 3.9e-07, 1.9e-06, 3.5e-06, 2.7e-06, 8.7e-06),
    "pair_front": (3.1e-07, 5.2e-07, 5.1e-08, 1.9e-07, 7.7e-08, 2.6e-07, 2.4e-07),
    "pair_opaque": (3.2e-07, 5e-07, 2.2e-07, 2.3e-07, 2.3e-07, 2e-07, 1.2e-07),
    "pair_back": (3.5e-07, 3.4e-07, 5e-08, 3e-07, 1.6e-07, 4e-07, 4.9e-07),
    "ordinary": (1.8e-06, 1.9e-06, 9.4e-07, 7.3e-07, 4.1e-07, 3.2e-07, 7.1e-07),
}
BLENDS_NOTHING = ("op_zero", "op_negative", "thr_below")
CULLED = ("behind", "at_camera", "off_miss")


def test_hostile_scene_conditions(oracle):
    """Every named row has the property its name claims, on the oracle."""
    sc, rows, f, _, _ = Hh.hostile_reference(oracle)
    g, W, H = sc["gaussians"], Hh.HOSTILE_W, Hh.HOSTILE_H
    assert sorted(rows) == sorted(Hh.HOSTILE_ROWS) and len(set(rows.values())) == len(rows)
    rad, pix, m2 = f.radii, f.pixels.reshape(-1), f.geom["means2D"]
    i = lambda n: rows[n]
    # scales
    assert not g["scales"][i("zero3")].any() and rad[i("zero3")] == 3 and pix[i("zero3")] > 0      # the 0.3 px dilation alone
    s = g["scales"][i("zero1")]
    assert (s == 0).sum() == 1 and rad[i("zero1")] > 0 and pix[i("zero1")] > 0
    s = np.sort(g["scales"][i("needle")])
    assert s[2] >= 1e4 * s[1] and pix[i("needle")] > 0
    s = np.sort(g["scales"][i("pancake")])
    assert s[1] >= 1e5 * s[0] and s[2] == s[1] and pix[i("pancake")] > 0
    assert 10 * max(W, H) < rad[i("giant")] < 1e5 and pix[i("giant")] == W * H and f.geom["tiles_touched"][i("giant")] == 6
    # rotations
    norm = lambda n: float(np.linalg.norm(g["rotations"][i(n)].astype(np.float64)))
    assert abs(norm("q_small") - 0.1) < 1e-6 and abs(norm("q_large") - 10.0) < 1e-4 and norm("q_zero") == 0.0
    assert g["rotations"][i("q_negw")][0] < 0 and abs(norm("q_negw") - 1.0) < 1e-6
    for n in ("q_small", "q_large", "q_zero", "q_negw"):
        assert rad[i(n)] > 0 and pix[i(n)] > 0, n
    # opacities
    op = lambda n: g["opacities"][i(n), 0]
    assert op("op_zero") == 0 and op("op_one") == 1 and op("op_above_one") > 1 and op("op_negative") < 0
    for n in ("op_zero", "op_negative"):
        assert rad[i(n)] > 0 and pix[i(n)] == 0, n
    for n in ("op_one", "op_above_one"):
        assert pix[i(n)] > 0, n
    inf = np.float32(np.inf)
    assert op("thr_below") == np.nextafter(Hh.ALPHA_MIN, -inf) and op("thr_above") == np.nextafter(Hh.ALPHA_MIN, inf)
    assert op("thr_exact") == Hh.ALPHA_MIN
    for n in ("thr_below", "thr_above", "thr_exact"):
        k = i(n)
        assert rad[k] > 0 and (m2[k] == np.round(m2[k])).all(), n              # exactly on a pixel centre
        # the centre pixel is the only one that can blend it: at every other centre alpha is below half the threshold
        con = f.geom["conic_opacity"][k].astype(np.float64)
        ys, xs = np.mgrid[0:H, 0:W]
        dx, dy = m2[k, 0] - xs, m2[k, 1] - ys
        alpha = float(op("thr_above")) * np.exp(-0.5 * (con[0] * dx * dx + con[2] * dy * dy) - con[1] * dx * dy)
        assert (alpha >= 0.5 * Hh.ALPHA_MIN).sum() == 1 and alpha[int(m2[k, 1]), int(m2[k, 0])] == op("thr_above"), n
        assert g["means3D"][k, 2] < g["means3D"][[j for j in range(Hh.HOSTILE_P) if rad[j] > 0 and j not in (i("thr_below"), i("thr_above"), i("thr_exact"))], 2].min()
    assert pix[i("thr_below")] == 0 and pix[i("thr_above")] == 1 and pix[i("thr_exact")] == 1
    # means
    assert g["means3D"][i("behind"), 2] < 0 and rad[i("behind")] == 0
    assert not g["means3D"][i("at_camera")].any() and rad[i("at_camera")] == 0
    k = i("pixel_centre")
    assert (m2[k] == np.array([30, 10], np.float32)).all() and pix[k] > 0
    k = i("tile_corner")
    assert (m2[k] == np.float32(15.5)).all() and f.geom["tiles_touched"][k] == 4 and pix[k] > 0
    k = i("off_one_tile_in")
    assert m2[k, 0] < 0 and 0 <= m2[k, 0] + rad[k] < 16 and f.geom["tiles_touched"][k] == 2 and pix[k] > 0      # one column, both rows
    px, py, r = Hh.ewa_radius(sc, i("off_miss"))
    assert rad[i("off_miss")] == 0 and 0 < px + r < 1 and 0 <= py < H, (px, r)      # ends inside pixel 0's half: getRect's (px + r + 15) / 16 is 0
    k = i("beyond_clamp")
    assert g["means3D"][k, 0] / g["means3D"][k, 2] > 1.3 * sc["cam"]["tanfovx"] and m2[k, 0] > W - 1 + 16
    assert m2[k, 0] - rad[k] < W - 1 and pix[k] > 0
    # rect edges: exact integers in getRect's own float arithmetic
    f32 = np.float32
    k = i("rect_lo_exact")
    q = (m2[k, 0] - f32(rad[k])) / f32(16)
    assert q == 1.0 and pix[k] > 0
    k = i("rect_hi_exact")
    q = (m2[k, 0] + f32(rad[k]) + f32(15)) / f32(16)
    assert q == 2.0 and pix[k] > 0
    k = i("rect_hi_touch")
    assert m2[k, 0] + f32(rad[k]) == 16 and m2[k, 1] + f32(rad[k]) == 16 and f.geom["tiles_touched"][k] == 1 and pix[k] > 0
    # the rect of every named row, from means2D and radii by getRect restated in numpy
    idx = np.array(sorted(rows.values()))
    np.testing.assert_array_equal(oracle.tiles_from_rect(W, H, m2, rad)[idx], f.geom["tiles_touched"][idx])
    # clones
    for a, b in (("clone_a0", "clone_a1"), ("clone_a0", "clone_a2"), ("pair_front", "pair_back")):
        for k_, v in g.items():
            assert v[i(a)].tobytes() == v[i(b)].tobytes(), (a, b, k_)
    assert g["means3D"][i("pair_opaque")].tobytes() == g["means3D"][i("pair_front")].tobytes() and op("pair_opaque") == 1
    assert i("pair_front") < i("pair_opaque") < i("pair_back")
    trio, seen = [i("clone_a0"), i("clone_a1"), i("clone_a2")], 0
    for t in range(f.ranges.shape[0]):
        lst = f.point_list[int(f.ranges[t, 0]):int(f.ranges[t, 1])].tolist()
        if trio[0] in lst:
            at = lst.index(trio[0])
            assert lst[at:at + 3] == trio, "tile %d" % t
            seen += 1
        if i("pair_front") in lst:
            at = lst.index(i("pair_front"))
            assert lst[at:at + 3] == [i("pair_front"), i("pair_opaque"), i("pair_back")], "tile %d" % t
            seen += 1
    assert seen >= 3
    assert pix[trio[0]] == pix[trio[1]] == pix[trio[2]] > 0 and pix[i("pair_front")] == pix[i("pair_back")] > 0
    # clamped colour channels and amplitudes occur among the blended rows
    blended = (rad > 0) & (pix > 0)
    assert f.geom["clamped"][blended].any() and f.geom["clamped_p"][blended].any()
    assert np.isfinite(f["color"]).all() and np.isfinite(f["phasor"]).all() and f.num_rendered > 200


def test_float64_reference_is_finite_and_zero_on_culled_rows(oracle):
    """tests/torch_ref.py on a Gaussian at the camera centre (a direction of length zero, 0 / 0 in the Jacobian): the oracle
    culls it, and the reference gives exact zeros, not NaN, there and in every other row."""
    sc, rows, f, ref, _ = Hh.hostile_reference(oracle)
    for k in T:
        assert np.isfinite(ref[k]).all(), k
        for n in CULLED + BLENDS_NOTHING:
            assert not ref[k][rows[n]].any(), (k, n)
    assert np.isfinite(ref["phase_offset"]).all() and np.isfinite(ref["dc_offset"]).all()
    for p, part in ref["parts"].items():
        assert np.isfinite(part).all(), p


def test_oracle_row_by_row_against_float64(oracle):
    sc, rows, f, ref, _ = Hh.hostile_reference(oracle)
    _, b = Hh.run_oracle(oracle, sc)
    assert all(np.isfinite(v).all() for v in b.values())
    got = Hh.oracle_grads(b, sc)
    e = Hh.row_errors(ref, got, rows)
    bad = []
    print()
    for n in list(rows) + ["ordinary"]:
        ratios = [e[(n, k)][0] / e[(n, k)][2] if e[(n, k)][2] else 0.0 for k in T]
        print('    "%s": (%s),' % (n, ", ".join("%.2g" % r for r in ratios)))
        for k, r, m in zip(T, ratios, MEASURED[n]):
            err, own, yard = e[(n, k)]
            if own == 0.0:
                assert m == 0.0, (n, k)
                if got[k][rows[n]].any():
                    bad.append("%s %s: %.3g where float64 is an exact zero" % (n, k, err))
            elif not r <= 2.0 * m:
                bad.append("%s %s: %.3g of its yardstick %.3g, measured %.3g" % (n, k, r, yard, m))
            assert m <= 1e-2, "%s %s: too ill-conditioned to be a yardstick" % (n, k)
    # exact zeros: every row the oracle culls or never blends, in every tensor (means2D with its third column)
    zero_rows = [rows[n] for n in CULLED + BLENDS_NOTHING]
    for k in T:
        assert not got[k][zero_rows].any(), k
    # a zero axis has no gradient of its own: dL/ds = 2 s (...), an exact zero on both sides
    zero_axis = sc["gaussians"]["scales"][rows["zero1"]] == 0
    assert not got["scales"][rows["zero1"]][zero_axis].any() and not ref["scales"][rows["zero1"]][zero_axis].any()
    assert got["scales"][rows["zero1"]][~zero_axis].all()
    # the pair around the opaque row: identical inputs, gradients that differ by the transmittance the opaque row leaves
    a, c = rows["pair_front"], rows["pair_back"]
    assert np.abs(got["opacities"][c]).max() < 0.5 * np.abs(got["opacities"][a]).max()
    assert not bad, "\n".join(bad)
