"""Generate tests/golden/rigid.npz from the reference's find_knn, rigidity_loss and isometry_loss (utils/loss_utils.py:35-72).

Usage: python tests/golden/make_golden_rigid.py <checkout of the reference project>.  The reference files themselves never
travel; only the input/output vectors written here do.  utils/loss_utils.py is loaded by file path (it imports torch alone).

Three cases <c>: u21 (21 points uniform in [-1, 1], K = 20), u1025 (1025 such points, K = 20) and c3000 (3000 points of
tests/rigid_ref.py's `centred` cloud -- test_knn.py's clustered one, its mean at the origin --, K = 20).  Per case:

  <c>_prev [P, 3] float32, <c>_curr = prev + N(0, 0.01) float32, <c>_idx int16 [P, K] the exact table of `prev`
  (rigid_ref.exact_knn; equal to brute force, asserted).  w_i_j and initial_xyz_to_knn_dist are NOT stored: they are
  rigid_ref.table_weights(prev, idx), correctly rounded float32 operations that give the same bits everywhere -- stored, the
  two would double the file.
  <c>_rig, <c>_iso            float64 [2]: the reference function's value computed in float32 and in float64
  <c>_rig_g_curr, <c>_iso_g_curr   float64 [P, 3]: autograd's gradient of the float64 value.  d rigidity / d prev is the
                              negative of <c>_rig_g_curr (asserted here to 1e-14 of its max-norm) and is not stored.
  <c>_e_ref                   float64 [5]: |float32 result - float64 result| in max-norm over the max-norm of the float64
                              one, for rig, iso, rig_g_curr, rig_g_prev, iso_g_curr
  <c>_find_knn                int16 [P, K], u21 and u1025 only: the reference's own find_knn(prev, K) in float32, which on
                              these two clouds is the exact table (asserted)

The float32 gradients themselves are not stored either; what the tests need of them is e_ref.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rigid_ref as R  # noqa: E402

SEED = 20261021
CASES = {"u21": (21, 20, "uniform"), "u1025": (1025, 20, "uniform"), "c3000": (3000, 20, "centred")}
TENSORS = ("rig", "iso", "rig_g_curr", "rig_g_prev", "iso_g_curr")


def load_reference(ref):
    spec = importlib.util.spec_from_file_location("ref_loss_utils", os.path.join(ref, "utils", "loss_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_results(lu, prev, curr, idx, w, d0, dtype):
    """the two functions and autograd, every tensor in `dtype`"""
    class G:
        w_i_j = torch.tensor(w).to(dtype)
        initial_xyz_to_knn_dist = torch.tensor(d0).to(dtype)
    t_idx = torch.tensor(idx.astype(np.int64))
    out = {}
    p, c = (torch.tensor(a).to(dtype).requires_grad_() for a in (prev, curr))
    rig = lu.rigidity_loss(G, p, c, t_idx)
    rig.backward()
    out.update(rig=rig.detach().numpy(), rig_g_curr=c.grad.numpy(), rig_g_prev=p.grad.numpy())
    c = torch.tensor(curr).to(dtype).requires_grad_()
    iso = lu.isometry_loss(G, c, t_idx)
    iso.backward()
    out.update(iso=iso.detach().numpy(), iso_g_curr=c.grad.numpy())
    return out


def main():
    lu = load_reference(sys.argv[1])
    rng = np.random.default_rng(SEED)
    out = {}
    for name, (P, K, kind) in CASES.items():
        prev = R.clouds(P, kind)
        curr = (prev + rng.normal(0, 0.01, prev.shape)).astype(np.float32)
        idx, _ = R.exact_knn(prev, K)
        assert np.array_equal(idx, R.knn_bruteforce(prev, K)[0]), name
        assert not (idx == np.arange(P)[:, None]).any() and idx.max() < 2 ** 15
        w, d0 = R.table_weights(prev, idx)
        r32, r64 = (reference_results(lu, prev, curr, idx, w, d0, dt) for dt in (torch.float32, torch.float64))
        own = R.losses(prev, curr, idx, w, d0)
        e_ref = []
        for k in TENSORS:
            assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64
            scale = np.abs(r64[k]).max()
            assert np.abs(own[k] - r64[k]).max() <= 1e-12 * scale, (name, k)
            e_ref.append(float(np.abs(r32[k].astype(np.float64) - r64[k]).max() / scale))
        assert np.abs(r64["rig_g_prev"] + r64["rig_g_curr"]).max() <= 1e-14 * np.abs(r64["rig_g_curr"]).max(), name
        out[name + "_prev"], out[name + "_curr"], out[name + "_idx"] = prev, curr, idx.astype(np.int16)
        for k in ("rig", "iso"):
            out["%s_%s" % (name, k)] = np.array([float(r32[k]), float(r64[k])], np.float64)
        out[name + "_rig_g_curr"], out[name + "_iso_g_curr"] = r64["rig_g_curr"], r64["iso_g_curr"]
        out[name + "_e_ref"] = np.array(e_ref, np.float64)
        if kind == "uniform":
            found = lu.find_knn(torch.tensor(prev), K).numpy()
            assert np.array_equal(found, idx), name
            out[name + "_find_knn"] = found.astype(np.int16)
        print(name, "e_ref", " ".join("%s %.3g" % kv for kv in zip(TENSORS, e_ref)), "max in-degree", R.max_in_degree(idx))
    path = os.path.join(HERE, "rigid.npz")
    np.savez_compressed(path, **out)
    print("wrote rigid.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
