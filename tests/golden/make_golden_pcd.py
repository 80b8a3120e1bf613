"""Generate tests/golden/pcd.npz and tests/golden/points3d_small.ply from tests/pcd_ref.py.

Usage: python tests/golden/make_golden_pcd.py.  Both files come from the numpy restatement of the reference's statements
(tests/pcd_ref.py), not from a run of the reference: its dataset readers import cv2 and plyfile, which the machines that run
this suite do not have.

  pcd.npz
    view [4, 4] float32, znear, fov_x, fov_y, depth_range, phase_offset, stride     the camera and the call's scalars
    tof [5, 7, 3] float32, rendered [5, 7] float64                                  the frame and a rendered depth image
    <mode>_xyz [rows, 3] float32 (the f4 column), <mode>_dist, and for the two init modes _amp, _sh_color, _color, _sh_amp,
    _amplitude                                                                      pcd_ref.unproject for the three modes
    cloud_xyz, cloud_colors, cloud_phases, cloud_amplitudes, cloud_seg              pcd_ref.make_cloud(5, SEED)
  points3d_small.ply                                                                pcd_ref.store_bytes of that cloud
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
SEED = 20261020


def main():
    import pcd_ref as R
    H, W, stride = 5, 7, 2
    cam = R.camera(W, H)
    tof = R.make_frame(H, W, SEED)
    rendered = np.random.default_rng(SEED + 1).uniform(1.0, 3.0, (H, W))
    out = dict(view=cam["view"], znear=cam["znear"], fov_x=cam["fov_x"], fov_y=cam["fov_y"], depth_range=R.DEPTH_RANGE,
               phase_offset=R.PHASE_OFFSET, stride=stride, tof=tof, rendered=rendered)
    for mode in ("torf_init", "ftorf_init", "proxy"):
        got = R.unproject(tof, 1 if mode == "proxy" else stride, cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], R.DEPTH_RANGE,
                          R.PHASE_OFFSET, mode, rendered=rendered if mode == "proxy" else None)
        for k, v in got.items():
            out["%s_%s" % (mode, k)] = v.astype(np.float32) if k == "xyz" else v
    cloud = R.make_cloud(5, SEED)
    out.update(dict(zip(("cloud_xyz", "cloud_colors", "cloud_phases", "cloud_amplitudes", "cloud_seg"), cloud)))
    np.savez_compressed(os.path.join(HERE, "pcd.npz"), **out)
    with open(os.path.join(HERE, "points3d_small.ply"), "wb") as f:
        f.write(R.store_bytes(*cloud))


if __name__ == "__main__":
    main()
