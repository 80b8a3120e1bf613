"""Writes tests/golden/query.npz: the deformation queries of an iteration as the reference states them, for
tests/test_query.py.  Run by hand where the reference is checked out (as make_golden.py); the tests read only the .npz.

The network is utils/time_utils.py's DeformNetwork constructed as scene/deform_model.py:9-16 does, with the seeded
parameters of oracle/deform_ref.random_params (as deform.npz).  Every query is scene/gaussian_model.py:170-174 restated:
`t = torch.tensor(np.array([fid])).float()` expanded over the points, `xyz = (xyz / scene_extent).detach()`.  The scene
extent is a power of two, so the division is exact whichever way it is formed.

  points   : 48 of 64 seeded ones, those furthest from a ReLU edge (deform_ref.relu_margin > 1e-6) at all three times
  lerp     : frame 5 of 12 -- train.py:169-176: times 4/11 and 8/11,
             d_xyz = 0.25 * ((5 - 4) * d_xyz_next + (8 - 5) * d_xyz_curr)
  flow     : frame 4 -- train.py:171-173, 248-249, 255-256: times 4/11, 8/11 and 0,
             d_xyz = d_xyz_curr, flow_next = d_xyz_next - d_xyz, flow_prev = d_xyz_prev - d_xyz
  torf     : train.py:167: one time 5/11, d_xyz and d_sh
For each case: the outputs, seeded upstream gradients g and the reference's autograd parameter gradients of
sum_i (out_i * g_i).sum(), sub-sampled and named as in deform.npz (`grad:` whole, `grad_s:` [::8, ::4]).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
from utils.time_utils import DeformNetwork  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import deform_ref  # noqa: E402
from make_golden import DEFORM_SEED, reference_kwargs  # noqa: E402

TOTAL_NUM_VIEWS = 12
SCENE_EXTENT = 4.0


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self          # time_utils.py:121,127 on a CPU-only host
    net = DeformNetwork(**reference_kwargs())
    net.isotropic = False
    params = deform_ref.random_params(DEFORM_SEED, t_multires=net.t_multires)
    net.load_state_dict({k: torch.tensor(v) for k, v in params.items()})
    rng = np.random.default_rng(DEFORM_SEED + 11)
    den = TOTAL_NUM_VIEWS - 1
    fids = [4 / den, 8 / den, 0 / den, 5 / den]
    as_t = lambda fid, n: torch.tensor(np.array([fid])).float().unsqueeze(0).expand(n, -1)       # gaussian_model.py:171
    cand = (rng.random((64, 3)) * 2.0 - 0.5).astype(np.float32) * np.float32(SCENE_EXTENT)       # raw positions, some outside [0, extent)
    norm = (torch.tensor(cand) / SCENE_EXTENT).numpy()
    margin = np.min([deform_ref.relu_margin(params, norm, as_t(fid, 64).numpy()) for fid in fids], axis=0)
    keep = np.sort(np.argsort(-margin)[:48])
    assert margin[keep].min() > 1e-6, margin[keep].min()
    xyz = cand[keep]
    n = xyz.shape[0]
    _xyz = torch.tensor(xyz, requires_grad=True)

    def query_dmlp(fid):                                    # gaussian_model.py:170-174, every Gaussian dynamic
        t = as_t(fid, n)
        x = (_xyz / SCENE_EXTENT).detach()
        return net(x, t)

    out = dict(xyz=xyz, scene_extent=np.float64(SCENE_EXTENT), total_num_views=np.int64(TOTAL_NUM_VIEWS),
               seed=np.int64(DEFORM_SEED), x=(_xyz / SCENE_EXTENT).detach().numpy())

    def record(case, frame_id, times, outs, names):
        net.zero_grad(set_to_none=True)
        gs = [rng.normal(size=tuple(o.shape)).astype(np.float32) for o in outs]
        sum((o * torch.tensor(g)).sum() for o, g in zip(outs, gs)).backward()
        out[case + ":frame_id"] = np.int64(frame_id)
        out[case + ":times"] = np.array(times, np.float64)
        out[case + ":names"] = np.array(names)
        for name, o, g in zip(names, outs, gs):
            out["%s:out:%s" % (case, name)] = o.detach().numpy()
            out["%s:g:%s" % (case, name)] = g
        none = []
        for name, p in net.named_parameters():
            if p.grad is None:
                none.append(name)
            elif p.grad.numel() <= 4096:
                out["%s:grad:%s" % (case, name)] = p.grad.numpy().copy()
            else:
                out["%s:grad_s:%s" % (case, name)] = p.grad.numpy()[::8, ::4].copy()
        out[case + ":grad_none"] = np.array(none)

    # lerp: train.py:169-176 on frame 5
    frame_id = 5
    curr_int_fid = (frame_id // 4) * 4
    next_int_fid = (frame_id // 4 + 1) * 4
    d_xyz_curr, _, _, _ = query_dmlp(curr_int_fid / den)
    d_xyz_next, _, _, _ = query_dmlp(next_int_fid / den)
    d_xyz = 0.25 * ((frame_id - curr_int_fid) * d_xyz_next + (next_int_fid - frame_id) * d_xyz_curr)
    record("lerp", frame_id, [curr_int_fid / den, next_int_fid / den], [d_xyz], ["d_xyz"])

    # flow: train.py:171-173, 248-249, 255-256 on frame 4
    frame_id = 4
    curr_int_fid = (frame_id // 4) * 4
    d_xyz_curr, _, _, _ = query_dmlp(curr_int_fid / den)
    d_xyz = d_xyz_curr
    d_xyz_next, _, _, _ = query_dmlp((frame_id + 4) / den)
    d_xyz_prev, _, _, _ = query_dmlp((frame_id - 4) / den)
    record("flow", frame_id, [curr_int_fid / den, (frame_id + 4) / den, (frame_id - 4) / den],
           [d_xyz, d_xyz_next - d_xyz, d_xyz_prev - d_xyz], ["d_xyz", "flow_next", "flow_prev"])

    # torf: train.py:167 on frame 5
    frame_id = 5
    d_xyz, d_rot, d_sh, d_sh_p = query_dmlp(frame_id / den)
    assert not d_rot.any() and not d_sh_p.any()
    record("torf", frame_id, [frame_id / den], [d_xyz, d_sh], ["d_xyz", "d_sh"])

    np.savez(os.path.join(HERE, "query.npz"), **out)
    print("query.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(HERE, "query.npz"))))


if __name__ == "__main__":
    main()
