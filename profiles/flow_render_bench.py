"""The two scene-flow renders of an ftorf flow iteration (train.py:243-261) at the reference's size: 100 k Gaussians, 320x240,
30 % dynamic, both flows, forward + backward of a loss on both images.  Today's two render_flow calls (the reference's
gaussian_renderer/__init__.py:141-204: torch.zeros, boolean-mask assignments, GaussianRasterizer with colors_precomp) against
gftorf_amd.flow.render_flow_pair, eagerly and (render_flow_pair only: the masked assignments read the host) captured in a
graph.  Device events around each iteration after warm-up; prints the median, 10th and 90th percentile in microseconds as one
JSON line (and writes it to --out).

    python profiles/flow_render_bench.py [--iters 200] [--warmup 20] [--fused-only] [--out FILE]

Run with --fused-only under `rocprofv3 --kernel-trace --stats` for the kernel times."""
import argparse
import json
import math
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np        # noqa: E402
import torch              # noqa: E402

from gftorf_amd import GaussianRasterizationSettings, GaussianRasterizer, flow, synth      # noqa: E402


def scene(dev, P, W, H, seed):
    cam = synth.make_camera(W, H, w2c=synth.look_at_w2c(0.05, -0.02, 0.0, (0.05, 0.0, 0.1)))
    g = synth.make_gaussians(P, cam, seed, scale_lo=0.004, scale_hi=0.03)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    gen = torch.Generator().manual_seed(seed)
    mask = (torch.rand(P, generator=gen) < 0.3).to(dev)
    normalize = lambda q: torch.nn.functional.normalize(q, dim=-1)
    raw = t(g["rotations"])
    pc = types.SimpleNamespace(get_xyz=t(g["means3D"]), get_opacity=torch.full((P, 1), 0.1, device=dev), get_scaling=t(g["scales"]),
                               _rotation=raw, get_rotation=normalize(raw), rotation_activation=normalize,
                               get_features_color=t(g["shs"]), get_features_phasor=t(g["shs_p"]), get_motion_mask=mask,
                               active_sh_degree=3, use_view_dependent_phase=True)
    tof = types.SimpleNamespace(tof_image_height=H, tof_image_width=W, FoVx_tof=2 * math.atan(cam["tanfovx"]),
                                FoVy_tof=2 * math.atan(cam["tanfovy"]), world_view_transform_tof=t(cam["viewmatrix"]),
                                full_proj_transform_tof=t(cam["projmatrix"]), camera_center_tof=t(cam["campos"]),
                                znear=cam["znear"], zfar=cam["zfar"], depth_range=10.0)
    n = int(mask.sum())
    d = {k: (s * torch.randn((n, c), generator=gen)).to(dev) for k, s, c in
         (("d_xyz_curr", 0.01, 3), ("d_rot", 0.05, 4), ("d_xyz", 0.01, 3), ("next", 0.02, 3), ("prev", 0.02, 3))}
    up = [torch.randn((3, H, W), generator=gen).to(dev) for _ in range(2)]
    return pc, tof, d, up


def render_flow(cam, pc, d_xyz, d_rot, flow3d, bg):
    """the reference's render_flow body (gaussian_renderer/__init__.py:141-204) on this package's GaussianRasterizer"""
    s = GaussianRasterizationSettings(
        image_height=int(cam.tof_image_height), image_width=int(cam.tof_image_width), tanfovx=math.tan(cam.FoVx_tof * 0.5),
        tanfovy=math.tan(cam.FoVy_tof * 0.5), bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform_tof,
        projmatrix=cam.full_proj_transform_tof, sh_degree=pc.active_sh_degree, campos=cam.camera_center_tof,
        prefiltered=False, debug=False, near_n=cam.znear, far_n=cam.zfar, depth_range=cam.depth_range,
        use_view_dependent_phase=pc.use_view_dependent_phase)
    screenspace = torch.zeros_like(pc.get_xyz, requires_grad=True) + 0
    m = pc.get_motion_mask
    means3D = torch.zeros(pc.get_xyz.shape, device=m.device)
    means2D = torch.zeros(screenspace.shape, device=m.device)
    opacity = torch.zeros(pc.get_opacity.shape, device=m.device)
    scales = torch.zeros(pc.get_scaling.shape, device=m.device)
    rotations = torch.zeros(pc.get_rotation.shape, device=m.device)
    flow3d_ = torch.zeros(pc.get_xyz.shape, device=m.device)
    means3D[~m] = pc.get_xyz[~m]
    means2D[~m] = screenspace[~m]
    opacity[~m] = pc.get_opacity[~m]
    scales[~m] = pc.get_scaling[~m]
    rotations[~m] = pc.get_rotation[~m]
    flow3d_[~m] = torch.zeros_like(pc.get_xyz[~m])
    means3D[m] = pc.get_xyz[m] + d_xyz
    means2D[m] = screenspace[m]
    opacity[m] = pc.get_opacity[m]
    scales[m] = pc.get_scaling[m]
    rotations[m] = pc.rotation_activation(pc._rotation[m] + d_rot)
    flow3d_[m] = flow3d
    return GaussianRasterizer(raster_settings=s)(means3D=means3D.detach(), means2D=means2D.detach(), opacities=opacity.detach(),
                                                  colors_precomp=flow3d_, scales=scales.detach(), rotations=rotations.detach())[0]


def iteration(fused, cam, pc, d, leaves, up, bg):
    ff, fb = leaves["next"] - leaves["d_xyz"], leaves["prev"] - leaves["d_xyz"]
    if fused:
        imf, imb = flow.render_flow_pair(cam, pc, d["d_xyz_curr"], d["d_rot"], ff, fb, bg)
    else:
        imf = render_flow(cam, pc, d["d_xyz_curr"], d["d_rot"], ff, bg)
        imb = render_flow(cam, pc, d["d_xyz_curr"], d["d_rot"], fb, bg)
    ((imf * up[0]).sum() + (imb * up[1]).sum()).backward()
    return imf, imb


def captured(fn, args):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn(*args)
    return graph.replay


def time_it(fn, args, iters, warmup):
    for _ in range(warmup):
        fn(*args)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(*args)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0)
    ts = np.array(ts)
    return {"median_us": round(float(np.median(ts)), 2), "p10_us": round(float(np.percentile(ts, 10)), 2),
            "p90_us": round(float(np.percentile(ts, 90)), 2), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_render_bench.py needs a HIP device")
    dev = torch.device("cuda:0")
    P, W, H = 100_000, 320, 240
    pc, cam, d, up = scene(dev, P, W, H, 7)
    bg = torch.zeros((7, H, W), device=dev)
    leaves = {k: d[k].clone().requires_grad_() for k in ("d_xyz", "next", "prev")}

    def step(fused):
        for v in leaves.values():
            v.grad = None
        iteration(fused, cam, pc, d, leaves, up, bg)

    res = {"gaussians": P, "size": [H, W], "dynamic_share": round(float(pc.get_motion_mask.float().mean()), 3),
           "device": torch.cuda.get_device_name(dev)}
    res["render_flow_pair"] = time_it(step, (True,), a.iters, a.warmup)
    res["render_flow_pair_graph_replay"] = time_it(captured(step, (True,)), (), a.iters, a.warmup)
    if not a.fused_only:
        res["render_flow_x2"] = time_it(step, (False,), a.iters, a.warmup)
        res["render_flow_x2_graph_replay"] = "not capturable: the boolean-mask assignments read the host"
        out = {}
        for fused in (True, False):
            for v in leaves.values():
                v.grad = None
            ims = iteration(fused, cam, pc, d, leaves, up, bg)
            out[fused] = [x.detach().clone() for x in ims] + [leaves[k].grad.clone() for k in ("d_xyz", "next", "prev")]
        res["max_rel_diff"] = {n: float((x - y).abs().max() / y.abs().max()) for n, x, y in
                               zip(("image_fwd", "image_bwd", "grad_d_xyz", "grad_next", "grad_prev"), out[True], out[False])}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
