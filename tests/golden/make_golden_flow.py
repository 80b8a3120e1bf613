"""Generate tests/golden/flow.npz from the reference's flow helpers (scene/torf_utils.py).

Usage: python tests/golden/make_golden_flow.py <checkout of the reference project>.  The reference files themselves never
travel; only the input/output vectors written here do.

torf_utils.py is loaded by file path: cv2 and imageio are not needed by the flow helpers, and scene/__init__.py pulls in
the whole model, so those modules (and scene.cameras, for the ToFCamera annotation) are stubbed first.  The composition is
train.py:244-259's, on the CPU in float32, with autograd with respect to both 3-D flows:

    points3d = distance_to_points3d(depth, cam); points2d = project_points(points3d, cam)
    flow2d_<dir> = project_flow(points2d, points3d, flow3d_<dir>, cam)
    l2_<dir> = torch.square(flow2d_<dir> - gt_<dir>).mean()

  flow.npz, per case <c> in ("ident", "ragged", "fwdonly"):
    <c>_depth [1,H,W], <c>_K, <c>_K_tof [3,3], <c>_w2v, <c>_w2v_tof [4,4] (world_view_transform(_tof) as the reference
    stores them: the transposed world-to-view matrix), <c>_flow3d_<dir> [3,H,W], <c>_gt_<dir> [2,H,W] (float32 inputs);
    <c>_points3d, <c>_points2d, <c>_flow2d_<dir>, <c>_l2_<dir> (a 0-d value), <c>_grad_<dir> [3,H,W] (the reference's
    float32 results).  <dir> is "fwd" and "bwd"; the "fwdonly" case has no backward direction.
      ident    24 x 32, identity colour and ToF poses
      ragged   37 x 53, rotated and translated colour pose; the ToF pose differs by a rotation and a baseline
      fwdonly  48 x 64, fx != fy, off-centre principal point, forward flow only
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch


HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261017


def load_torf_utils(ref):
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
    spec = importlib.util.spec_from_file_location("torf_utils", os.path.join(ref, "scene", "torf_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rotation(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def stored_w2v(R, t):
    """scene/cameras.py:121: the world-to-view matrix [[R, t], [0, 1]], transposed (float32)"""
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return np.ascontiguousarray(M.T.astype(np.float32))


def intrinsics(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def tof_z(p, w2v_tof):
    """z of [3, N] points in the ToF camera (float64)"""
    M = w2v_tof.astype(np.float64).T
    return M[2, :3] @ p + M[2, 3]


def draw(rng, H, W, K, w2v, w2v_tof, dirs):
    """depth in 0.5-8 and 3-D flows of magnitude 0.01-0.2, re-drawn until no current or next point has |z| < 0.1 in the
    ToF camera; 2-D ground truth of a few pixels"""
    for _ in range(100):
        depth = rng.uniform(0.5, 8.0, size=(1, H, W)).astype(np.float32)
        flows = {d: (rng.uniform(0.01, 0.2, size=(3, H, W)) * rng.choice([-1.0, 1.0], size=(3, H, W))).astype(np.float32)
                 for d in dirs}
        u, v = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
        fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
        z = depth[0] / np.sqrt(((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2 + 1)
        pc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z]).reshape(3, -1)
        p = (np.linalg.inv(w2v.astype(np.float64)) @ np.vstack([pc, np.ones((1, H * W))]))[:3]
        zs = [tof_z(p, w2v_tof)] + [tof_z(p + flows[d].reshape(3, -1), w2v_tof) for d in dirs]
        if min(np.abs(zz).min() for zz in zs) >= 0.1:
            gts = {d: (2.0 * rng.normal(size=(2, H, W))).astype(np.float32) for d in dirs}
            return depth, flows, gts
    raise RuntimeError("no admissible draw")


def main():
    tu = load_torf_utils(sys.argv[1])
    rng = np.random.default_rng(SEED)
    I = np.eye(3)
    Rc = rotation(0.3, -0.2, 0.1)
    cases = {
        "ident": (24, 32, intrinsics(28.0, 28.0, 16.0, 12.0), intrinsics(28.0, 28.0, 16.0, 12.0),
                  stored_w2v(I, np.zeros(3)), stored_w2v(I, np.zeros(3)), ("fwd", "bwd")),
        "ragged": (37, 53, intrinsics(45.5, 44.25, 26.0, 18.0), intrinsics(41.0, 40.5, 25.5, 18.5),
                   stored_w2v(Rc, np.array([0.3, -0.2, 0.5])),
                   stored_w2v(rotation(0.08, 0.05, -0.04) @ Rc, np.array([0.3 - 0.06, -0.2 + 0.01, 0.5 + 0.02])),
                   ("fwd", "bwd")),
        "fwdonly": (48, 64, intrinsics(52.0, 61.0, 20.25, 30.75), intrinsics(50.0, 58.5, 34.5, 21.25),
                    stored_w2v(rotation(-0.15, 0.1, 0.0), np.array([-0.1, 0.05, 0.2])),
                    stored_w2v(rotation(-0.1, 0.12, 0.02), np.array([-0.15, 0.05, 0.25])), ("fwd",)),
    }
    out = {}
    for name, (H, W, K, K_tof, w2v, w2v_tof, dirs) in cases.items():
        depth, flows, gts = draw(rng, H, W, K, w2v, w2v_tof, dirs)
        cam = types.SimpleNamespace(fx=float(K[0, 0]), fy=float(K[1, 1]), cx=float(K[0, 2]), cy=float(K[1, 2]),
                                    K=torch.tensor(K), K_tof=torch.tensor(K_tof), world_view_transform=torch.tensor(w2v),
                                    world_view_transform_tof=torch.tensor(w2v_tof))
        f3 = {d: torch.tensor(flows[d], requires_grad=True) for d in dirs}
        # train.py:244-259
        points3d = tu.distance_to_points3d(torch.tensor(depth).detach(), cam)
        points2d = tu.project_points(points3d, cam)
        total = 0.0
        for d in dirs:
            flow2d = tu.project_flow(points2d, points3d, f3[d], cam)
            l2 = torch.square(flow2d - torch.tensor(gts[d])).mean()
            total = total + l2
            out["%s_flow2d_%s" % (name, d)] = flow2d.detach().numpy()
            out["%s_l2_%s" % (name, d)] = np.float32(l2.item())
        total.backward()
        out.update({name + "_depth": depth, name + "_K": K, name + "_K_tof": K_tof, name + "_w2v": w2v,
                    name + "_w2v_tof": w2v_tof, name + "_points3d": points3d.numpy(), name + "_points2d": points2d.numpy()})
        for d in dirs:
            out["%s_flow3d_%s" % (name, d)] = flows[d]
            out["%s_gt_%s" % (name, d)] = gts[d]
            out["%s_grad_%s" % (name, d)] = f3[d].grad.numpy()
    path = os.path.join(HERE, "flow.npz")
    np.savez_compressed(path, **out)
    print("wrote flow.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
