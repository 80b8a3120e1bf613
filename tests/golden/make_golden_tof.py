"""Generate tests/golden/tof.npz from the reference's ToF depth and the statements of its training log.

Usage: python tests/golden/make_golden_tof.py <checkout of the reference project>.  The reference files themselves never
travel; only the input/output vectors written here do.

scene/torf_utils.py (depth_from_tof_torch), utils/graphics_utils.py (phasor2real_img_amp) and utils/sh_utils.py (SH2PA) are
loaded by file path, with cv2, imageio and scene.cameras stubbed exactly as make_golden_flow.py does.  The statements are
train.py:188-200 and :420-433 on the CPU in float32, as the reference runs them (torch for the two depths, numpy for the
scattering-phase maps):

    pd, gpd  depth_from_tof_torch of phasor[:3] and of gt_phasor[:3] with the camera's depth_range and the phase offset
    amp      plane 2 of phasor[:3] * tof_multiplier through phasor2real_img_amp (numpy, [H, W, 3] layout); gt_amp likewise
    gsp = gt_amp * gpd^2, sp = amp * depth[0]^2, sp_tof = amp * pd^2 and |gsp - sp|, |gsp - sp_tof|, all numpy float32

  tof.npz, per case <c> in ("plain", "ragged", "full"):
    inputs   <c>_phasor [C,H,W], <c>_gt_phasor [3,H,W], <c>_depth [1,H,W], <c>_depth_range, <c>_phase_offset,
             <c>_tof_multiplier (0-d float32); "full" also <c>_gt_depth [1,H,W], <c>_features_phasor [257,4,2], <c>_visible [257]
    results  <c>_phase_depth, <c>_gt_phase_depth [H,W]; the float32 scalars <c>_sp, <c>_sp_tof, <c>_gsp, <c>_sp_err,
             <c>_sp_tof_err, <c>_tof_depth_err, <c>_amp_err; "full" also <c>_depth_err, <c>_gs_sp, <c>_gs_sp_visible
      plain   24 x 32, phase_offset 0,    tof_multiplier 1, a 3-plane phasor
      ragged  37 x 53, phase_offset 0.3,  tof_multiplier 2, the first three planes of a 7-plane phasor
      full    48 x 64, phase_offset -0.2, tof_multiplier 1, gt_depth, 257 amplitude rows of which 60 % are visible

Inputs are drawn so that the reference alone is well-conditioned: the wrapped phase after the offset lies in
[0.05, 2 pi - 0.05] and amplitudes in [0.02, 1]; draw() asserts that no pixel takes another `+ 2 pi` branch in float32 than
in float64.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch


HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261018


def load(ref, name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref):
    for name in ("cv2", "imageio"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["cv2"].INTER_AREA = 3           # a default argument of the image helpers
    for name in ("scipy", "scipy.io", "matplotlib", "matplotlib.pyplot"):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    scene = types.ModuleType("scene")
    scene.__path__ = []
    cameras = types.ModuleType("scene.cameras")
    cameras.ToFCamera = object
    scene.cameras = cameras
    sys.modules["scene"], sys.modules["scene.cameras"] = scene, cameras
    return (load(ref, "torf_utils", "scene", "torf_utils.py"), load(ref, "graphics_utils", "utils", "graphics_utils.py"),
            load(ref, "sh_utils", "utils", "sh_utils.py"))


def draw_phasor(rng, planes, H, W, phase_offset):
    """[planes, H, W] float32: plane 2 an amplitude in [0.02, 1], planes 0 / 1 a vector of length 0.05-1 whose phase, less
    the offset and wrapped, lies in [0.05, 2 pi - 0.05]; the same +2 pi branch in float32 as in float64"""
    wrapped = rng.uniform(0.05, 2 * np.pi - 0.05, size=(H, W))
    theta = wrapped + phase_offset
    length = rng.uniform(0.05, 1.0, size=(H, W))
    out = rng.uniform(-1.0, 1.0, size=(planes, H, W))
    out[0], out[1], out[2] = length * np.cos(theta), length * np.sin(theta), rng.uniform(0.02, 1.0, size=(H, W))
    out = out.astype(np.float32)
    assert float(np.abs(out[0]).min()) > 1e-5           # the clamp of the real part has its own test
    p64 = np.arctan2(out[1].astype(np.float64), out[0].astype(np.float64)) - phase_offset
    p32 = np.arctan2(out[1], out[0]) - np.float32(phase_offset)
    assert p32.dtype == np.float32 and np.array_equal(p64 < 0, p32 < 0)
    w64 = np.where(p64 < 0, p64 + 2 * np.pi, p64)
    assert 0.049 <= w64.min() and w64.max() <= 2 * np.pi - 0.049
    return out


def main():
    tu, gu, shu = load_reference(sys.argv[1])
    rng = np.random.default_rng(SEED)
    cases = {"plain": (24, 32, 3, 10.0, 0.0, 1.0, False), "ragged": (37, 53, 7, 7.5, 0.3, 2.0, False),
             "full": (48, 64, 3, 12.0, -0.2, 1.0, True)}
    out = {}
    for name, (H, W, planes, depth_range, phase_offset, tof_multiplier, full) in cases.items():
        ph = draw_phasor(rng, planes, H, W, phase_offset)
        gt = draw_phasor(rng, 3, H, W, phase_offset)
        dep = rng.uniform(0.3, depth_range / 2, size=(1, H, W)).astype(np.float32)
        phasor, gt_phasor, depth = torch.tensor(ph), torch.tensor(gt), torch.tensor(dep)
        # train.py:188-200: the two depths in torch, the maps in numpy
        pd = tu.depth_from_tof_torch(phasor[:3], depth_range, phase_offset=phase_offset)
        gpd = tu.depth_from_tof_torch(gt_phasor[:3], depth_range, phase_offset=phase_offset)
        amp = gu.phasor2real_img_amp(phasor[:3].numpy().transpose(1, 2, 0) * tof_multiplier)[2]
        gt_amp = gu.phasor2real_img_amp(gt_phasor.numpy().transpose(1, 2, 0))[2]
        gsp = gt_amp * (gpd.numpy() ** 2)
        sp = amp * (depth.numpy()[0] ** 2)
        sp_tof = amp * (pd.numpy() ** 2)
        assert pd.dtype == torch.float32 and sp.dtype == np.float32 and amp.dtype == np.float32
        # train.py:422-433: the means as the writer gets them
        res = dict(phase_depth=pd.numpy(), gt_phase_depth=gpd.numpy(), sp=sp.mean(), sp_tof=sp_tof.mean(), gsp=gsp.mean(),
                   sp_err=np.abs(gsp - sp).mean(), sp_tof_err=np.abs(gsp - sp_tof).mean(),
                   tof_depth_err=torch.abs(pd - gpd).mean().numpy(), amp_err=np.abs(amp - gt_amp).mean())
        inp = dict(phasor=ph, gt_phasor=gt, depth=dep, depth_range=np.float32(depth_range), phase_offset=np.float32(phase_offset),
                   tof_multiplier=np.float32(tof_multiplier))
        if full:
            P = 257
            gdep = (dep + rng.normal(0.0, 0.2, size=dep.shape)).astype(np.float32)
            feats = rng.normal(0.0, 1.0, size=(P, 4, 2)).astype(np.float32)
            vis = rng.random(P) < 0.6
            coeff = torch.tensor(feats)[:, 0, 1]
            res.update(depth_err=torch.abs(depth - torch.tensor(gdep)).mean().numpy(),            # train.py:431
                       gs_sp=shu.SH2PA(coeff).mean().numpy(),                                     # :420
                       gs_sp_visible=shu.SH2PA(coeff[torch.tensor(vis)]).mean().numpy())          # :421
            inp.update(gt_depth=gdep, features_phasor=feats, visible=vis)
        for k, v in list(inp.items()) + list(res.items()):
            v = np.asarray(v)
            assert v.dtype in (np.float32, np.bool_), (k, v.dtype)
            out["%s_%s" % (name, k)] = v
    path = os.path.join(HERE, "tof.npz")
    np.savez_compressed(path, **out)
    print("wrote tof.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
