"""Generate tests/golden/tracks.npz from the reference's project_points_subset and its colour generator.

Usage: python tests/golden/make_golden_tracks.py <checkout of the reference project>.  The reference files themselves never
travel; only the input/output vectors written here do.

scene/torf_utils.py is loaded by file path, with the stubs make_golden_tof.py uses; generate_color_array is compiled alone
out of render_ftorf_viz_traj.py (the module itself imports a video stack).  The statements are
render_ftorf_viz_traj.py:264-283 and :294-295 on the CPU in torch float32, as the reference states them, and once more in
float64; the inputs come from tests/test_tracks.py's draw_cameras / draw_points.

Every point is redrawn until, in every frame, both of its coordinates lie at least 1e-3 px from an integer in the float64
AND in the reference's float32 evaluation (asserted at the end): only then are int(xy) and the comparisons of :318 / :339 the
same in any evaluation whose error stays far below that, and tests may compare them without leaving a point out.  Every point
is at least 0.2 in front of every camera (asserted).

  tracks.npz, per case <c> of test_tracks.CASES:
    inputs   <c>_initial_pos [P, 3], <c>_flow [U, P, 3], <c>_flow_index int32 [T], <c>_K [T, 3, 3], <c>_world_view [T, 4, 4]
    results  <c>_ref_pos_last [P, 3] float32 (the sequential sums), <c>_ref_step_ok uint8 [T, P], <c>_ref_xy_int int32 [T, P, 2]
             (int() of the reference's all_2D_pos)
  ref_err_xy, ref_err_motion, ref_err_mean_z   the largest |reference float32 - float64| of the quantity over all cases
  select_opacity [1000, 1], select_scaling [1000, 3]   get_opacity / get_scaling for the selection test on case `wide`
  colors_1, colors_40        generate_color_array(S) after np.random.shuffle
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
SEED = 20261021


def reference_function(ref, file_name, name):
    """one function of a reference file, compiled on its own with numpy as `np`"""
    path = os.path.join(ref, file_name)
    tree = ast.parse(open(path).read(), path)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    scope = {"np": np}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), scope)
    return scope[name]


def reference_statements(tu, c, dtype):
    """:264-283 with the reference's project_points_subset, every tensor in `dtype`"""
    T = len(c["flow_index"])
    views = [types.SimpleNamespace(K_tof=torch.tensor(c["K"][t]).to(dtype), world_view_transform_tof=torch.tensor(c["world_view"][t]).to(dtype))
             for t in range(T)]
    gs_xyz_flow = torch.stack([torch.tensor(c["flow"][u]).to(dtype) for u in c["flow_index"]], dim=0)
    initial_3D_pos = torch.tensor(c["initial_pos"]).to(dtype)
    all_3D_pos = [initial_3D_pos]
    all_2D_pos = [tu.project_points_subset(initial_3D_pos, views[0])]
    for vid, view in enumerate(views):
        if vid > 0:
            next_3D_pos = all_3D_pos[vid - 1] + gs_xyz_flow[vid - 1]
            all_3D_pos.append(next_3D_pos)
            all_2D_pos.append(tu.project_points_subset(next_3D_pos, view))
    motion = torch.mean(torch.sum(gs_xyz_flow ** 2, dim=-1), dim=0)
    mean_z = torch.mean(torch.stack(all_3D_pos, dim=0)[:, :, -1], dim=0)
    return dict(xy=torch.stack(all_2D_pos, dim=0).numpy(), pos_last=all_3D_pos[-1].numpy(), motion=motion.numpy(), mean_z=mean_z.numpy())


def main():
    from make_golden_tof import load_reference
    import test_tracks as tt
    ref = sys.argv[1]
    tu, _, _ = load_reference(ref)
    generate_color_array = reference_function(ref, "render_ftorf_viz_traj.py", "generate_color_array")
    rng = np.random.default_rng(SEED)
    out = {}
    worst = dict(xy=0.0, motion=0.0, mean_z=0.0)
    for name, (P, T, U) in tt.CASES.items():
        K, view = tt.draw_cameras(T)
        pos, flow = tt.draw_points(rng, P, U)
        c = dict(initial_pos=pos, flow=flow, flow_index=np.array([t * U // T for t in range(T)], np.int32), K=K, world_view=view)
        for _ in range(200):
            r32, r64 = reference_statements(tu, c, torch.float32), reference_statements(tu, c, torch.float64)
            bad = tt.unsafe_points(r32["xy"].astype(np.float64)) | tt.unsafe_points(r64["xy"])
            if not bad.any():
                break
            c["initial_pos"][bad], c["flow"][:, bad] = tt.draw_points(rng, int(bad.sum()), U)
        assert not bad.any(), name
        assert r32["xy"].dtype == np.float32 and r64["xy"].dtype == np.float64
        s64, s32 = tt.statements_np(c), tt.statements_np(c, np.float32)
        for k in ("xy", "motion", "mean_z"):
            assert np.abs(s64[k] - r64[k]).max() <= 1e-12 * max(1.0, np.abs(r64[k]).max()), (name, k)
            worst[k] = max(worst[k], float(np.abs(r32[k].astype(np.float64) - r64[k]).max()))
        assert np.array_equal(s32["pos_last"].view(np.uint32), r32["pos_last"].view(np.uint32)), name
        homog = np.concatenate([tt.positions_np(c["initial_pos"], c["flow"], c["flow_index"], np.float64), np.ones((T, P, 1))], axis=2)
        assert np.einsum("tpk,tkr->tpr", homog, c["world_view"].astype(np.float64))[..., 2].min() >= 0.2, name
        ok32, ok64 = tt.step_ok_np(r32["xy"]), tt.step_ok_np(r64["xy"])
        assert np.array_equal(ok32, ok64) and np.array_equal(r32["xy"].astype(np.int32), r64["xy"].astype(np.int32)), name
        for k, a in c.items():
            out["%s_%s" % (name, k)] = a
        out[name + "_ref_pos_last"] = r32["pos_last"]
        out[name + "_ref_step_ok"] = ok32
        out[name + "_ref_xy_int"] = r32["xy"].astype(np.int32)
    for k, v in worst.items():
        out["ref_err_" + k] = np.float64(v)
    out["select_opacity"] = rng.uniform(0.01, 0.99, size=(1000, 1)).astype(np.float32)
    out["select_scaling"] = np.exp(rng.normal(-4.0, 0.7, size=(1000, 3))).astype(np.float32)
    state = np.random.get_state()
    for S in (1, 40):
        colors = generate_color_array(S)
        np.random.shuffle(colors)
        out["colors_%d" % S] = colors
    np.random.set_state(state)
    path = os.path.join(HERE, "tracks.npz")
    np.savez_compressed(path, **out)
    print("wrote tracks.npz", os.path.getsize(path), "bytes;", ", ".join("ref_err_%s %.3g" % kv for kv in worst.items()))


if __name__ == "__main__":
    main()
