"""Generate tests/golden/present.npz from the reference's display statements and matplotlib's cm.magma.

Usage: python tests/golden/make_golden_present.py <checkout of the reference project>.  The reference files themselves never
travel; only the input/output vectors written here do.  Needs matplotlib.

scene/torf_utils.py (to8b, normalize_im, normalize_im_gt, depth_from_tof) and utils/graphics_utils.py (phasor2real_img_amp)
are loaded by file path, with the stubs make_golden_tof.py uses.  The statements are render.py:129-184 on the CPU in numpy
float32, as the reference runs them after its `.cpu()` copies; the inputs come from tests/test_present.py's draw_view, whose
phasors are conditioned so that depth_tof's colours do not hang on the last bits of arctan2 (asserted there for every pixel).

  present.npz, per case <c>:
    inputs   <c>_image [3,H,W], <c>_phasor [C,H,W], <c>_depth, <c>_acc, <c>_dd [1,H,W] (those the case has), <c>_ranges [6],
             <c>_znear, <c>_zfar, <c>_depth_range, <c>_phase_offset, <c>_tof_multiplier (0-d float32)
    results  <c>_out_<image> for color, real, imag, amp, quad, depth, depth_tof, depth_norm, dd (uint8) and depth_tof_f,
             depth_norm_f (float32), those the inputs produce
      plain   12 x 16, a 3-plane phasor, tof_multiplier 1, phase_offset 0
      quad    19 x 27, a 7-plane phasor, tof_multiplier 2, phase_offset 0.3
      tofcam  5 x 7, depth and acc only (the ToF-camera pass of render.py:127, 168-172)
  magma_u8 [257, 4]       to8b(cm.magma(.)) of the 256 entries, then of a NaN
  ref_err_depth_tof       the largest |numpy float32 - float64 restatement| / depth_range of the ToF depth over the cases
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
SEED = 20261019


def reference_view(tu, gu, cm, v):
    """render.py:129-184 with the reference's own functions; `v` as draw_view returns it"""
    out = {}
    znear, zfar = v["znear"], v["zfar"]
    magma = lambda d: tu.to8b(cm.magma(1 - (d - znear) / (zfar - znear)))
    if "image" in v:
        out["color"] = tu.to8b(v["image"].transpose(1, 2, 0))
    if "phasor" in v:
        hwc = v["phasor"].transpose(1, 2, 0)
        chans = gu.phasor2real_img_amp(hwc * float(v["tof_multiplier"]))
        for k, (name, im) in enumerate(zip(("real", "imag", "amp"), chans)):
            out[name] = tu.to8b(tu.normalize_im_gt(im, v["ranges"][2 * k:2 * k + 2]))
        if v["phasor"].shape[0] == 7:
            out["quad"] = np.stack([tu.to8b(np.abs(v["phasor"][3:][k])) for k in range(4)])
        d = tu.depth_from_tof(hwc, v["depth_range"], float(v["phase_offset"]))[:, :, 0]
        out["depth_tof_f"], out["depth_tof"] = d, magma(d)
    if "depth" in v:
        out["depth"] = magma(v["depth"][0])
        if "acc" in v:
            dn = v["depth"][0] / v["acc"][0]
            out["depth_norm_f"], out["depth_norm"] = dn, magma(dn)
    if "dd" in v:
        out["dd"] = tu.to8b(tu.normalize_im(v["dd"][0]))
    return out


def main():
    from make_golden_tof import load_reference
    import test_present as tp
    from matplotlib import cm
    tu, gu, _ = load_reference(sys.argv[1])
    rng = np.random.default_rng(SEED)
    with np.errstate(invalid="ignore"):
        table = np.concatenate([tu.to8b(cm.magma(np.arange(256))), tu.to8b(cm.magma(np.array([np.nan], np.float32)))])
    out = dict(magma_u8=table)
    worst = 0.0
    for name, (H, W, planes, mult, off, dr, inputs) in tp.CASES.items():
        v = tp.draw_view(rng, H, W, planes, dr, off, mult, inputs)
        zn, zf = 0.05 * v["depth_range"] * 0.9, 0.55 * v["depth_range"] * 1.1                    # render.py:54
        assert zn.dtype == np.float32 and zn == v["znear"] and zf == v["zfar"]
        res = reference_view(tu, gu, cm, v)
        mine = tp.view_np(v, table)
        assert set(res) == set(mine)
        for k, a in res.items():
            assert a.dtype == mine[k].dtype and np.array_equal(a, mine[k]), (name, k)
        if "phasor" in v:
            d64 = tp.depth_from_tof_np(v["phasor"], float(v["depth_range"]), float(v["phase_offset"]), np.float64)
            worst = max(worst, float(np.abs(res["depth_tof_f"] - d64).max()) / float(v["depth_range"]))
        for k, a in v.items():
            out["%s_%s" % (name, k)] = np.asarray(a)
        for k, a in res.items():
            assert a.dtype in (np.uint8, np.float32), (k, a.dtype)
            out["%s_out_%s" % (name, k)] = a
    out["ref_err_depth_tof"] = np.float64(worst)
    path = os.path.join(HERE, "present.npz")
    np.savez_compressed(path, **out)
    print("wrote present.npz", os.path.getsize(path), "bytes; ref_err_depth_tof %.3g" % worst)


if __name__ == "__main__":
    main()
