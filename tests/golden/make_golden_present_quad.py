"""Generate tests/golden/present_quad.npz from the reference's tof_to_image and matplotlib's seismic map.

Usage: python tests/golden/make_golden_present_quad.py <checkout of the reference project>.  The reference files themselves
never travel; only the input/output vectors written here do.  Needs matplotlib.

scene/torf_utils.py is loaded by file path, with the stubs make_golden_tof.py uses.  The statements are
render_ftorf_viz_traj.py:237-243 on the CPU in numpy float32, as the reference runs them after its `.cpu()` copies; the
inputs come from tests/test_present_quad.py's draw_quad.  Every step of them is an IEEE float32 operation (asserted here
against test_present_quad.quad_np for every pixel), so no value has to keep a distance from a bin edge.

  present_quad.npz, per size <c> of test_present_quad.SIZES:
    <c>_phasor [7, H, W]       the input
    <c>_out_<g><t> [4, H, W, 3] tof_to_image of plane 3 + PERMUTATION[i], after - 0.5 when g and x / (1 + x) when t
  seismic_u8 [257, 4]          (255 * seismic(.)).astype(uint8) of the 256 entries, then of a NaN
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
SEED = 20261020


def reference_quads(tu, phasor, permutation, has_gt, tonemap):
    """render_ftorf_viz_traj.py:237-243 with the reference's own tof_to_image"""
    out = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(4):
            quad_im = phasor[3:][np.array(permutation)][i]
            if has_gt:
                quad_im = quad_im - 0.5
            if tonemap:
                quad_im = quad_im / (1 + quad_im)
            assert quad_im.dtype == np.float32
            out.append(tu.tof_to_image(quad_im))
    return np.stack(out)


def main():
    from make_golden_tof import load_reference
    import matplotlib.pyplot as plt
    import test_present_quad as tq
    tu, _, _ = load_reference(sys.argv[1])
    rng = np.random.default_rng(SEED)
    cmap = plt.get_cmap("seismic")
    with np.errstate(invalid="ignore"):
        table = np.concatenate([(255 * cmap(np.arange(256))).astype(np.uint8),
                                (255 * cmap(np.array([np.nan], np.float32))).astype(np.uint8)])
    out = dict(seismic_u8=table)
    for name, (H, W) in tq.SIZES.items():
        ph = tq.draw_quad(rng, H, W)
        out[name + "_phasor"] = ph
        for has_gt, tonemap in tq.OPTIONS:
            res = reference_quads(tu, ph, tq.PERMUTATION, has_gt, tonemap)
            assert res.dtype == np.uint8 and res.shape == (4, H, W, 3)
            assert np.array_equal(res, tq.quad_np(ph, table, tq.PERMUTATION, has_gt, tonemap)), (name, has_gt, tonemap)
            out["%s_out_%d%d" % (name, has_gt, tonemap)] = res
    path = os.path.join(HERE, "present_quad.npz")
    np.savez_compressed(path, **out)
    print("wrote present_quad.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
