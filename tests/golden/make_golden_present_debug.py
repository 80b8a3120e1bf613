"""Generate tests/golden/present_debug.npz with the reference's own image functions, applied as its pipe.debug block applies them
(train.py:295-378, ToF branch).

Usage: python tests/golden/make_golden_present_debug.py <checkout of the reference project>.  The reference files themselves
never travel; only the input/output vectors written here do.  Needs numpy >= 2 (`0.05 * depth_range * 0.9` on the camera's 0-d
float32 depth_range stays float32 there, which gftorf_amd.present.zplanes pins), torch (the two ToF depths are the reference's
depth_from_tof_torch of the phasors, as train.py:188-189 computes them) and matplotlib (cm.magma; its table is asserted to be
the one tests/golden/present.npz holds and tests/test_present.py pins).

scene/torf_utils.py (to8b, normalize_im, normalize_im_gt, depth_from_tof, depth_from_tof_torch) and utils/graphics_utils.py
(phasor2real_img_amp) are loaded by file path, with the stubs make_golden_tof.py uses.  `block_images` calls them in the block's
order on numpy arrays as the `.cpu()` copies hold them: first what lines 194-200 form (the scattering phases), then the images
of lines 295-378; `sequence_lists` forms the four lists of lines 57-64 over the three training views, so the ranges really
come from lists.  Line 317 pairs three channels with the first three of five lists; the pairing is made here the same way, by
a zip that stops at the shorter side.  The inputs come from tests/test_present_debug.py's draw_debug;
test_present_debug.debug_np is asserted here to give every byte for every case, and its ranges_np every range.

Two pixels of `ragged` carry a NaN into an unnormalised to8b, where numpy's cast to uint8 is the platform's; it is asserted (in
the test file, on the fixture) to have given 0.

  present_debug.npz, per case <c> of test_present_debug.CASES:
    inputs   <c>_phasor [7,H,W], <c>_gt_phasor [3,H,W], <c>_depth, <c>_dd [1,H,W], <c>_phase_depth, <c>_gt_phase_depth [H,W],
             <c>_image, <c>_gt_image [3,H,W], <c>_gt_quad [4,H,W] (float32), <c>_permutation [4], <c>_quad_index (int32),
             <c>_ranges [8], <c>_znear, <c>_zfar, <c>_tof_multiplier, <c>_depth_range (float32), <c>_phase_offset,
             <c>_gt_views [3,3,H,W] (the training views of lines 57-64; the first is this iteration's), <c>_seed
    results  <c>_out_<image> (uint8) for the 19 images of test_present_debug.IMAGES
  magma_u8 [257, 4]   to8b(cm.magma(.)) of the 256 entries, then of a NaN
  numpy               the version of numpy that ran the reference
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
SEED = 20261021


def hwc(chw):
    return chw.transpose(1, 2, 0)


def sequence_lists(tu, gu, views, depth_range, phase_offset):
    """the four lists of train.py:57-64: per training view the red / blue real and imaginary images, the amplitude, and the
    amplitude times the squared numpy ToF depth"""
    lists = [], [], [], []
    for view in views:
        re, im, amp = gu.phasor2real_img_amp(hwc(view[0:3]))
        sp = amp * (tu.depth_from_tof(hwc(view[0:3]), depth_range=depth_range, phase_offset=phase_offset)[:, :, 0]) ** 2
        for seq, a in zip(lists, (re, im, amp, sp)):
            seq.append(a)
    return lists


def block_images(tu, gu, cm, v, lists, depth_range):
    """{image name: the array the block hands to imageio.imwrite}, with the reference's functions in the block's order"""
    out = {}
    mult = float(v["tof_multiplier"])
    znear, zfar = 0.05 * depth_range * 0.9, 0.55 * depth_range * 1.1
    magma = lambda d: tu.to8b(cm.magma(1 - (d - znear) / (zfar - znear)))
    pd, gpd, d = v["phase_depth"], v["gt_phase_depth"], v["depth"][0]
    # :194-200
    amp = gu.phasor2real_img_amp(hwc(v["phasor"][:3]) * mult)[2]
    gt_amp = gu.phasor2real_img_amp(hwc(v["gt_phasor"]))[2]
    gt_sp = gt_amp * (gpd ** 2)
    sp = amp * (d ** 2)
    sp_tof = amp * (pd ** 2)
    sp_error, sp_tof_error = np.abs(gt_sp - sp), np.abs(gt_sp - sp_tof)
    # :295-338
    out["depth"] = magma(d)
    amp = gu.phasor2real_img_amp(hwc(v["phasor"][:3]) * mult)[2]
    gt_amp = gu.phasor2real_img_amp(hwc(v["gt_phasor"]))[2]
    amp_error = tu.normalize_im(np.abs(gt_amp - amp))
    names = ["amp", "scattering_phase", "scattering_phase_tof_depth"]
    for name, im, err, gt_list in zip(names, [amp, sp, sp_tof], [amp_error, sp_error, sp_tof_error], list(lists) + [lists[3]]):
        out[name] = tu.to8b(tu.normalize_im_gt(im, gt_list))
        out[name + "_error"] = tu.to8b(err)
    out["scattering_phase_gt"] = tu.to8b(tu.normalize_im_gt(gt_sp, lists[3]))
    out["depth_error"] = tu.to8b(tu.normalize_im(np.abs(gpd - d)))
    out["phase_depth"], out["phase_depth_gt"] = magma(pd), magma(gpd)
    out["phase_depth_error"] = tu.to8b(tu.normalize_im(np.abs(gpd - pd)))
    # :358-367
    image, gt_image = hwc(v["image"]), hwc(v["gt_image"])
    out["color"], out["color_gt"], out["color_error"] = tu.to8b(image), tu.to8b(gt_image), tu.to8b(np.abs(gt_image - image))
    out["dd"] = tu.to8b(tu.normalize_im(v["dd"][0]))
    # :369-378
    perm, shown = [int(k) for k in v["permutation"]], int(v["quad_index"]) % 4
    planes = {"quad": [], "quad_error": [], "quad_gt": []}
    for i in range(4):
        q, g = v["phasor"][3:][i], v["gt_quad"][perm][i]
        planes["quad"].append(tu.to8b(np.abs(q)))
        planes["quad_error"].append(tu.to8b(tu.normalize_im(np.abs(q - g)) if perm[i] == shown else np.zeros_like(q)))
        planes["quad_gt"].append(tu.to8b(np.abs(g)))
    out.update({k: np.stack(a) for k, a in planes.items()})
    return out


def main():
    import torch
    from make_golden_tof import load_reference
    import test_present_debug as td
    from matplotlib import cm
    assert int(np.__version__.split(".")[0]) >= 2, "numpy >= 2 keeps the colour map's planes float32, this is %s" % np.__version__
    tu, gu, _ = load_reference(sys.argv[1])
    with np.errstate(invalid="ignore"):
        table = np.concatenate([tu.to8b(cm.magma(np.arange(256))), tu.to8b(cm.magma(np.array([np.nan], np.float32)))])
    assert np.array_equal(table, np.load(os.path.join(HERE, "present.npz"))["magma_u8"])
    tof_depth = lambda tof, dr, off: tu.depth_from_tof_torch(torch.from_numpy(np.ascontiguousarray(tof)), dr, phase_offset=off).numpy()
    out = dict(magma_u8=table, numpy=np.array(np.__version__))
    for k, (name, (H, W, perm, qi, kind)) in enumerate(td.CASES.items()):
        seed = SEED + k
        v, views = td.draw_debug(np.random.default_rng(seed), H, W, perm, qi, kind, tof_depth)
        depth_range = np.array(td.DEPTH_RANGE, np.float32)
        zn, zf = 0.05 * depth_range * 0.9, 0.55 * depth_range * 1.1
        assert zn.dtype == np.float32 and zn == v["znear"] and zf == v["zfar"]
        lists = sequence_lists(tu, gu, list(views), depth_range, td.PHASE_OFFSET)
        ranges = np.array([f(seq) for seq in lists for f in (np.min, np.max)], np.float32)
        assert np.array_equal(ranges, v["ranges"]), (name, ranges, v["ranges"])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            res = block_images(tu, gu, cm, v, lists, depth_range)
        mine = td.debug_np(v, table)
        assert list(mine) == list(td.IMAGES) and set(res) == set(mine)
        for key, a in res.items():
            assert a.dtype == np.uint8 and a.shape == mine[key].shape, (name, key, a.dtype, a.shape)
            assert np.array_equal(a, mine[key]), (name, key, np.argwhere(a != mine[key])[:4].tolist())
            out["%s_out_%s" % (name, key)] = a
        for key, a in v.items():
            out["%s_%s" % (name, key)] = np.asarray(a)
        out.update({name + "_gt_views": views, name + "_depth_range": depth_range, name + "_phase_offset": np.float64(td.PHASE_OFFSET),
                    name + "_seed": np.int64(seed)})
        print("%-7s %3d x %3d seed %d: %s" % (name, H, W, seed, " ".join("%s %d..%d" % (key[:14], res[key].min(), res[key].max())
                                                                         for key in td.IMAGES)))
    path = os.path.join(HERE, "present_debug.npz")
    np.savez_compressed(path, **out)
    print("wrote present_debug.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
