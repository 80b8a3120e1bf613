"""Generate tests/golden/metrics.npz from the reference's evaluation statements (train.py:535-579).

Usage: python tests/golden/make_golden_metrics.py <checkout of the reference project>.  The reference files themselves never
travel; only the input/output vectors written here do.

utils/image_utils.py (psnr), utils/loss_utils.py (l1_loss, l2_loss) and scene/torf_utils.py (depth_from_tof_torch) are loaded by
file path, with cv2, imageio and scene.cameras stubbed exactly as make_golden_tof.py does.  The statements are train.py:535-566
on the CPU in float32, one fixture case per view, the eight sums kept as the reference keeps them (`+= x.mean().double()`) and
divided by the three views as train.py:570-579 does.

  metrics.npz, per case <c> in ("plain", "ragged", "full"):
    inputs   <c>_image, <c>_gt_image [3,H,W]; <c>_phasor [C,Ht,Wt] (render_phasor), <c>_tof_planes (first, last: the planes of
             it that are tof_rendered), <c>_gt_tof (tof_gt); "ragged" and "full" also <c>_depth, <c>_gt_depth [1,Ht,Wt],
             <c>_depth_range, <c>_phase_offset (0-d float32)
    results  the float32 values <c>_l1, <c>_psnr, <c>_l1_p, <c>_l2_p, <c>_psnr_p, <c>_l1_d, <c>_l2_d, <c>_l2_d_tof (0 where the
             reference adds nothing)
      plain   colour and ToF 24 x 32, a 3-plane phasor, num_phasor_channels = 2, no gt_depth
      ragged  colour 37 x 53, ToF 24 x 40, a 7-plane phasor, use_quad with frame_id 6 and tof_inverse_permutation (2, 0, 3, 1):
              plane 3 + 3 = 6; gt_depth, phase_offset 0.3
      full    colour and ToF 48 x 64, a 3-plane phasor, num_phasor_channels = 3, gt_depth, phase_offset -0.2
    avg_<name>   the float64 three-view averages
    ref_err_rel, ref_err_db   the float32 error of the reference's own means: the largest distance of any of the values above
             from the float64 restatement of the same lines (tests/test_metrics.py view64) -- relative for l1* / l2*, in dB for
             psnr*.  tests/test_metrics.py allows three times it.

Inputs are drawn so that the reference alone is well-conditioned, and asserted to be: image values in [0, 1], every channel's
mse at least 1e-4, the wrapped phase after the offset in [0.05, 2 pi - 0.05] with no pixel taking another `+ 2 pi` branch in
float32 than in float64.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_tof import draw_phasor, load, load_reference  # noqa: E402
from test_metrics import CASES, VALUES, view64  # noqa: E402

SEED = 20261019


def noisy(rng, a, lo, hi):
    return np.clip(a + rng.normal(0.0, 0.05, size=a.shape), lo, hi).astype(np.float32)


def main():
    ref = sys.argv[1]
    tu = load_reference(ref)[0]
    iu, lu = load(ref, "image_utils", "utils", "image_utils.py"), load(ref, "loss_utils", "utils", "loss_utils.py")
    l1_loss, l2_loss, psnr, depth_from_tof_torch = lu.l1_loss, lu.l2_loss, iu.psnr, tu.depth_from_tof_torch
    rng = np.random.default_rng(SEED)
    # (colour, ToF, phasor planes, use_quad, num_phasor_channels, frame_id, depth_range, phase_offset or None without gt_depth)
    cases = {"plain": ((24, 32), (24, 32), 3, False, 2, 0, 10.0, None), "ragged": ((37, 53), (24, 40), 7, True, 3, 6, 7.5, 0.3),
             "full": ((48, 64), (48, 64), 3, False, 3, 0, 12.0, -0.2)}
    assert tuple(cases) == CASES
    tof_inverse_permutation = torch.tensor([2, 0, 3, 1])
    out, err_rel, err_db = {}, 0.0, 0.0
    # train.py:516-517
    l1_test, l1_p_test, l2_p_test, l1_d_test, l2_d_test, l2_d_tof_test = 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
    psnr_test, psnr_p_test = 0.0, 0.0
    num_val_cams = 0
    total64 = dict.fromkeys(VALUES, 0.0)

    def distance(name, got, want):
        nonlocal err_rel, err_db
        if name.startswith("psnr"):
            err_db = max(err_db, abs(got - want))
        elif want != 0.0:
            err_rel = max(err_rel, abs(got - want) / abs(want))

    for name, ((Hc, Wc), (Ht, Wt), planes, use_quad, num_phasor_channels, frame_id, depth_range, phase_offset) in cases.items():
        image = rng.uniform(0.0, 1.0, size=(3, Hc, Wc)).astype(np.float32)
        phasor = draw_phasor(rng, planes, Ht, Wt, phase_offset or 0.0)
        inp = dict(image=image, gt_image=noisy(rng, image, 0.0, 1.0), phasor=phasor)
        assert inp["gt_image"].min() >= 0.0 and inp["gt_image"].max() <= 1.0 and image.min() >= 0.0 and image.max() <= 1.0
        rendered_image, gt_image = torch.tensor(inp["image"]), torch.tensor(inp["gt_image"])                  # :535-536
        res = dict.fromkeys(VALUES, torch.tensor(0.0))
        res["l1"], res["psnr"] = l1_loss(rendered_image, gt_image).mean(), psnr(rendered_image, gt_image).mean()
        l1_test += res["l1"].double()                                                                        # :537
        psnr_test += res["psnr"].double()                                                                    # :538
        rendered_phasor = torch.tensor(phasor)                                                                # :541
        if use_quad:                                                                                          # :543-546
            plane = 3 + int(tof_inverse_permutation[frame_id % 4])
            inp.update(tof_planes=np.array([plane, plane + 1]), gt_tof=noisy(rng, phasor[plane:plane + 1], -2.0, 2.0))
            gt_quad = torch.zeros(4, Ht, Wt)
            gt_quad[frame_id % 4] = torch.tensor(inp["gt_tof"][0])
            tof_gt = gt_quad[frame_id % 4].unsqueeze(0)
            tof_rendered = rendered_phasor[3:][tof_inverse_permutation][frame_id % 4].unsqueeze(0)
        else:                                                                                                 # :548-549
            inp.update(tof_planes=np.array([0, num_phasor_channels]), gt_tof=noisy(rng, phasor[:num_phasor_channels], -2.0, 2.0))
            gt_phasor = torch.tensor(inp["gt_tof"])
            tof_gt = gt_phasor[:num_phasor_channels]
            tof_rendered = rendered_phasor[:num_phasor_channels]
        assert torch.equal(tof_rendered, rendered_phasor[int(inp["tof_planes"][0]):int(inp["tof_planes"][1])])
        res["l1_p"], res["l2_p"] = l1_loss(tof_rendered, tof_gt).mean(), l2_loss(tof_rendered, tof_gt).mean()
        res["psnr_p"] = psnr(tof_rendered, tof_gt).mean()
        l1_p_test += res["l1_p"].double()                                                                    # :550
        l2_p_test += res["l2_p"].double()                                                                    # :551
        psnr_p_test += res["psnr_p"].double()                                                                # :552
        assert float(iu.mse(rendered_image, gt_image).min()) >= 1e-4 and float(iu.mse(tof_rendered, tof_gt).min()) >= 1e-4
        if phase_offset is not None:                                                                          # :559
            depth = rng.uniform(0.3, depth_range / 2, size=(1, Ht, Wt)).astype(np.float32)
            inp.update(depth=depth, gt_depth=(depth + rng.normal(0.0, 0.2, size=depth.shape)).astype(np.float32),
                       depth_range=np.float32(depth_range), phase_offset=np.float32(phase_offset))
            gt_depth, rendered_depth = torch.tensor(inp["gt_depth"]), torch.tensor(depth)                     # :560-561
            rendered_depth_tof = depth_from_tof_torch(rendered_phasor, inp["depth_range"].item(),
                                                      phase_offset=inp["phase_offset"].item()).unsqueeze(0)   # :562-563
            res["l1_d"], res["l2_d"] = l1_loss(rendered_depth, gt_depth).mean(), l2_loss(rendered_depth, gt_depth).mean()
            res["l2_d_tof"] = l2_loss(rendered_depth_tof, gt_depth).mean()
            l1_d_test += res["l1_d"].double()                                                                # :564
            l2_d_test += res["l2_d"].double()                                                                # :565
            l2_d_tof_test += res["l2_d_tof"].double()                                                        # :566
            assert min(float(res["l2_d"]), float(res["l2_d_tof"])) >= 1e-4
        num_val_cams += 1                                                                                     # :568
        v = dict(inp, tof_planes=tuple(int(x) for x in inp["tof_planes"]))
        if "depth_range" in v:
            v.update(depth_range=float(v["depth_range"]), phase_offset=float(v["phase_offset"]))
        ref64, _ = view64(v)
        for k in VALUES:
            assert res[k].dtype == torch.float32
            distance(k, float(res[k]), ref64[k])
            total64[k] += ref64[k]
            out["%s_%s" % (name, k)] = res[k].numpy()
        for k, a in inp.items():
            a = np.asarray(a)
            assert a.dtype in (np.float32, np.int64), (k, a.dtype)
            out["%s_%s" % (name, k)] = a
    # train.py:570-579
    sums = dict(l1=l1_test, psnr=psnr_test, l1_p=l1_p_test, l2_p=l2_p_test, psnr_p=psnr_p_test, l1_d=l1_d_test, l2_d=l2_d_test,
                l2_d_tof=l2_d_tof_test)
    for k in VALUES:
        avg = sums[k] / num_val_cams
        assert avg.dtype == torch.float64
        distance(k, float(avg), total64[k] / num_val_cams)
        out["avg_" + k] = avg.numpy()
    out["ref_err_rel"], out["ref_err_db"] = np.float64(err_rel), np.float64(err_db)
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote metrics.npz", os.path.getsize(path), "bytes; ref_err_rel %.3g ref_err_db %.3g" % (err_rel, err_db))


if __name__ == "__main__":
    main()
