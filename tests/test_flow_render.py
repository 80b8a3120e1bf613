"""gftorf_amd.flow.render_flows / render_flow_pair: the two scene-flow renders of an ftorf flow iteration (the reference's
render_flow, gaussian_renderer/__init__.py:141-204, called from train.py:249,256) from one rasterizer forward, the second flow
blended over its frame (csrc/k_features.hip, include/gftorf_features.h) and the gradient of both flows from one walk.  Checked
against GaussianRasterizer(colors_precomp=...) and its backward, the CPU oracle, render_flow restated with stock-torch masked
assignments, flow_loss on top, without host syncs and captured in a graph."""
import ctypes as C
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_features.h")


@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


def test_header_is_plain_c_and_every_symbol_is_exported(tmp_path, lib):
    from gftorf_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src)) - {"gft_config"})
    assert set(names) == set(_lib.FEATURE_EXPORTS), names
    assert not set(names) & (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS))
    for n in names:
        assert hasattr(lib, n), n
    prog = tmp_path / "features_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_features.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "features_abi.o")])
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16


def test_argument_errors_of_the_c_entry_points(lib):
    from gftorf_amd import _lib
    cfg = _lib.Config()
    cfg.P, cfg.W, cfg.H = 10, 32, 16
    x = C.c_void_p(16)                        # never dereferenced: the calls fail before any launch
    assert lib.gft_render_features(None, None, x, x, x, 64, 3, x, None, x) != 0
    assert "config is NULL" in _lib.last_error()
    assert lib.gft_render_features(None, C.byref(cfg), x, x, x, 64, 4, x, None, x) != 0
    assert "C must be 3 or 6" in _lib.last_error()
    assert lib.gft_render_features(None, C.byref(cfg), None, x, x, 64, 3, x, None, x) != 0
    assert "NULL scratch" in _lib.last_error()
    assert lib.gft_render_features(None, C.byref(cfg), x, x, None, 64, 3, x, None, x) != 0
    assert lib.gft_render_features(None, C.byref(cfg), x, x, x, -1, 3, x, None, x) != 0
    assert "instance count" in _lib.last_error()
    assert lib.gft_render_features(None, C.byref(cfg), x, x, x, 64, 3, None, None, x) != 0
    assert "NULL argument" in _lib.last_error()
    assert lib.gft_render_features(None, C.byref(cfg), x, x, x, 64, 6, C.c_void_p(20), None, x) != 0
    assert "8-byte aligned" in _lib.last_error()
    assert lib.gft_render_features_backward(None, C.byref(cfg), x, x, x, 64, 6, x, None, x) != 0
    assert "NULL argument" in _lib.last_error()
    assert lib.gft_render_features_backward(None, C.byref(cfg), x, x, x, 64, 2, x, x, x) != 0
    cfg.W = 0
    assert lib.gft_render_features_backward(None, C.byref(cfg), x, x, x, 64, 3, x, x, x) != 0
    assert "bad sizes" in _lib.last_error()
    cfg.W, cfg.P = 32, 0
    assert lib.gft_render_features_backward(None, C.byref(cfg), x, x, None, 0, 3, x, x, x) == 0      # nothing to write


def test_python_argument_errors():
    from gftorf_amd import flow
    P = 5
    geo = dict(means3D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4))
    f = torch.zeros(P, 3)
    s = object()              # never reached: the arguments are refused first
    with pytest.raises(RuntimeError, match="HIP device"):
        flow.render_flows(s, geo["means3D"], geo["opacities"], geo["scales"], geo["rotations"], f, f)
    with pytest.raises(RuntimeError, match="flow_b must be"):
        flow.render_flows(s, geo["means3D"], geo["opacities"], geo["scales"], geo["rotations"], f, torch.zeros(P, 6))
    with pytest.raises(RuntimeError, match="rotations must be"):
        flow.render_flows(s, geo["means3D"], geo["opacities"], geo["scales"], torch.zeros(P, 3), f)
    with pytest.raises(RuntimeError, match="opacities must be"):
        flow.render_flows(s, geo["means3D"], torch.zeros(P + 1), geo["scales"], geo["rotations"], f)
    for k in geo:
        bad = dict(geo)
        bad[k] = geo[k].clone().requires_grad_()
        with pytest.raises(NotImplementedError, match="%s requires grad" % k):
            flow.render_flows(s, bad["means3D"], bad["opacities"], bad["scales"], bad["rotations"], f.requires_grad_(), f)


def _masked_assembly(pc, d_xyz, d_rot, flow3d, render_regions=("static", "dynamic")):
    """render_flow's tensors (gaussian_renderer/__init__.py:165-185) by its masked assignments"""
    m = pc.get_motion_mask
    out = [torch.zeros(pc.get_xyz.shape), torch.zeros(pc.get_opacity.shape), torch.zeros(pc.get_scaling.shape),
           torch.zeros(pc.get_rotation.shape), torch.zeros(pc.get_xyz.shape)]
    if "static" in render_regions:
        for t, src in zip(out, (pc.get_xyz, pc.get_opacity, pc.get_scaling, pc.get_rotation)):
            t[~m] = src[~m]
    if "dynamic" in render_regions:
        out[0][m] = pc.get_xyz[m] + d_xyz
        out[1][m] = pc.get_opacity[m]
        out[2][m] = pc.get_scaling[m]
        out[3][m] = pc.rotation_activation(pc._rotation[m] + d_rot)
        out[4][m] = flow3d
    return out


@pytest.mark.parametrize("dynamic", [0, 3])
def test_flow_inputs_equal_the_masked_assignments(dynamic):
    """The device-side assembly of render_flow_pair equals render_flow's masked assignments bit for bit -- also for a model
    without a dynamic Gaussian, whose deformations and flows have no rows (nothing may be gathered from them)."""
    from gftorf_amd import flow
    P = 9
    gen = torch.Generator().manual_seed(dynamic)
    mask = torch.zeros(P, dtype=torch.bool)
    mask[torch.randperm(P, generator=gen)[:dynamic]] = True
    normalize = lambda q: torch.nn.functional.normalize(q, dim=-1)
    raw = torch.randn((P, 4), generator=gen)
    pc = types.SimpleNamespace(get_xyz=torch.randn((P, 3), generator=gen), get_opacity=torch.rand((P, 1), generator=gen),
                               get_scaling=torch.rand((P, 3), generator=gen), _rotation=raw, get_rotation=normalize(raw),
                               rotation_activation=normalize, get_motion_mask=mask)
    d_xyz, d_rot = torch.randn((dynamic, 3), generator=gen), torch.randn((dynamic, 4), generator=gen)
    leaf = torch.randn((dynamic, 3), generator=gen).requires_grad_()
    for regions in (("static", "dynamic"), ("static",), ("dynamic",)):
        got = flow._assemble_flow_inputs(pc, d_xyz, d_rot, [leaf * 2.0], regions)
        want = _masked_assembly(pc, d_xyz, d_rot, (leaf * 2.0).detach(), regions)
        for k, (g, w) in enumerate(zip(got[:4] + (got[4][0],), want)):
            assert torch.equal(g.detach(), w), (regions, k)
    got[4][0].sum().backward()
    assert leaf.grad is not None and leaf.grad.shape == (dynamic, 3)
    assert torch.equal(leaf.grad, torch.full((dynamic, 3), 2.0))


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _geometry(scene, dev, culled=0):
    g = scene["gaussians"]
    geo = {k: torch.tensor(g[k], dtype=torch.float32, device=dev) for k in ("means3D", "opacities", "scales", "rotations")}
    if culled:
        geo["means3D"][::culled, 0] += 1000.0           # far outside the frustum: radius 0
    return geo


def _reference_pair(settings, geo, fa, fb, ga, gb):
    """Two GaussianRasterizer calls with colors_precomp = fa / fb on the detached geometry, and their colour gradients."""
    from gftorf_amd import GaussianRasterizer
    rast = GaussianRasterizer(raster_settings=settings)
    P = geo["means3D"].shape[0]
    out, grads, radii = [], [], None
    for f, g in ((fa, ga), (fb, gb)):
        leaf = f.clone().requires_grad_()
        o = rast(means3D=geo["means3D"], means2D=torch.zeros((P, 3), device=f.device), opacities=geo["opacities"],
                 colors_precomp=leaf, scales=geo["scales"], rotations=geo["rotations"])
        (o[0] * g).sum().backward()
        out.append(o[0].detach())
        grads.append(leaf.grad.detach())
        radii = o[10]
    return out, grads, radii


def _ours(settings, geo, fa, fb, ga, gb):
    from gftorf_amd import flow
    a = fa.clone().requires_grad_()
    b = fb.clone().requires_grad_() if fb is not None else None
    ia, ib = flow.render_flows(settings, geo["means3D"], geo["opacities"], geo["scales"], geo["rotations"], a, b)
    loss = (ia * ga).sum() + ((ib * gb).sum() if ib is not None else 0.0)
    loss.backward()
    return ia.detach(), (ib.detach() if ib is not None else None), a.grad, (b.grad if b is not None else None)


def _rel(ref, got):
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _quad_flags(img, P, W, H, cap):
    """Quadrants that walked their sorted head unsaturated (GFT_CTRL_NFLAG): their lists were completed on demand."""
    from gftorf_amd import _lib
    L = _lib.get_layout(P, W, H, cap)
    return int(img[L.img_ctrl + 16:L.img_ctrl + 20].cpu().numpy().view(np.uint32)[0])


CASES = {
    # name: small_scene arguments, culled stride, zero background
    "small": (dict(P=400, W=80, H=48, seed=3), 0, False),
    "ragged": (dict(P=1500, W=70, H=37, seed=5, opacity=0.6), 0, True),
    "culled": (dict(P=3000, W=96, H=64, seed=9, z_lo=-1.0), 7, False),
    "deep": (dict(P=30000, W=64, H=48, seed=13, opacity=0.01, scale_lo=0.02, scale_hi=0.08), 0, True),
    "ftorf": (dict(P=100_000, W=320, H=240, seed=21, scale_lo=0.004, scale_hi=0.03, opacity=0.1), 0, True),
    # a sensor camera of helpers.CAMERAS: the principal point at 0.72 W
    "sensor": (dict(P=3000, W=96, H=64, seed=9, camera="shift_right"), 7, False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("binning", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_flows_match_two_rasterizer_calls(case, binning, gpu, monkeypatch):
    from gftorf_amd import _lib, api
    lib = _lib.load()
    args, culled, zero_bg = CASES[case]
    scene = Hh.small_scene(**args)
    W, H, P = args["W"], args["H"], args["P"]
    # (no per-camera schedule: every frame sorts heads only and completes the lists its quadrants ask for)
    monkeypatch.setattr(api, "_TILE_HINTS", False)
    monkeypatch.setattr(api, "keep_last_buffers", True)
    geo = _geometry(scene, gpu, culled)
    settings = Hh.gpu_settings(scene, gpu, bg=torch.zeros((7, H, W), device=gpu) if zero_bg else None)
    gen = torch.Generator().manual_seed(P + binning)
    fa, fb = ((0.05 * torch.randn((P, 3), generator=gen)).to(gpu) for _ in range(2))
    ga, gb = (torch.randn((3, H, W), generator=gen).to(gpu) for _ in range(2))
    # (one wave per quadrant draws the frame: image_b's walk multiplies T up as that kernel does, so the two images of a flow
    # differ only in how the colour sums round; frames of the segment-parallel forward: test_both_forward_kernels)
    lib.gft_set_binning_mode(binning)
    lib.gft_set_render_mode(0)
    try:
        ia, ib, dfa, dfb = _ours(settings, geo, fa, fb, ga, gb)
        flags = _quad_flags(api.last_call_buffers["img"], P, W, H, api.last_call_buffers["cap"])
        (ra, rb), (gra, grb), radii = _reference_pair(settings, geo, fa, fb, ga, gb)
        ia1, ib1, dfa1, dfb1 = _ours(settings, geo, fa, None, ga, None)
    finally:
        lib.gft_set_binning_mode(-1)
        lib.gft_set_render_mode(-1)
    torch.cuda.synchronize()
    print("\n%s binning %d: image_b %.3g, grad a %.3g, grad b %.3g, flagged quadrants %d"
          % (case, binning, _rel(rb, ib), _rel(gra, dfa), _rel(grb, dfb), flags))
    assert torch.equal(ia, ra), case                               # the same forward
    assert float(rb.abs().max()) > 0
    assert _rel(rb, ib) <= 1e-6, (case, _rel(rb, ib))
    assert _rel(gra, dfa) <= 1e-5 and _rel(grb, dfb) <= 1e-5, (case, _rel(gra, dfa), _rel(grb, dfb))
    assert ib1 is None and dfb1 is None and torch.equal(ia1, ra)
    assert _rel(gra, dfa1) <= 1e-5
    if culled:
        assert int((radii == 0).sum()) > 0
        assert float(dfa[radii == 0].abs().max()) == 0.0           # written in full: zero rows for culled Gaussians
    if case == "deep" and binning == 1:
        assert flags > 0, "no quadrant asked for its list's tail"


@pytest.mark.gpu
@pytest.mark.parametrize("render_mode", [0, 1])
def test_both_forward_kernels(render_mode, gpu):
    """frames drawn by one wave per quadrant and by the segment-parallel forward.  The latter forms the transmittance in front
    of a segment as a product of segment factors: its own images differ from one wave per quadrant by up to 2e-6
    (test_gpu_parity.py::test_segmented_forward_matches_one_wave_per_quadrant), and image_b, a serial walk, by as much."""
    from gftorf_amd import _lib
    lib = _lib.load()
    scene = Hh.small_scene(P=8000, W=160, H=96, seed=31, opacity=0.2)
    geo = _geometry(scene, gpu)
    settings = Hh.gpu_settings(scene, gpu)
    gen = torch.Generator().manual_seed(31)
    fa, fb = ((0.05 * torch.randn((8000, 3), generator=gen)).to(gpu) for _ in range(2))
    ga, gb = (torch.randn((3, 96, 160), generator=gen).to(gpu) for _ in range(2))
    lib.gft_set_render_mode(render_mode)
    try:
        ia, ib, dfa, dfb = _ours(settings, geo, fa, fb, ga, gb)
        (ra, rb), (gra, grb), _ = _reference_pair(settings, geo, fa, fb, ga, gb)
    finally:
        lib.gft_set_render_mode(-1)
    print("\nrender mode %d: image_b %.3g, grad a %.3g, grad b %.3g" % (render_mode, _rel(rb, ib), _rel(gra, dfa), _rel(grb, dfb)))
    assert torch.equal(ia, ra)
    assert _rel(rb, ib) <= (1e-6 if render_mode == 0 else 2e-6)
    assert _rel(gra, dfa) <= 1e-5 and _rel(grb, dfb) <= 1e-5


@pytest.mark.gpu
def test_gradients_match_the_oracle(gpu):
    from oracle import oracle
    oracle.build()
    scene = Hh.small_scene(P=600, W=64, H=48, seed=17)
    geo = _geometry(scene, gpu)
    settings = Hh.gpu_settings(scene, gpu)
    rng = np.random.default_rng(17)
    fa, fb = (0.1 * rng.standard_normal((600, 3)).astype(np.float32) for _ in range(2))
    ga, gb = (rng.standard_normal((3, 48, 64)).astype(np.float32) for _ in range(2))
    t = lambda a: torch.tensor(a, device=gpu)
    ia, ib, dfa, dfb = _ours(settings, geo, t(fa), t(fb), t(ga), t(gb))
    z = lambda c: np.zeros((c, 48, 64), np.float32)
    for f, g, img, grad in ((fa, ga, ia, dfa), (fb, gb, ib, dfb)):
        fw, bw = Hh.run_oracle(oracle, scene, backward=False, inputs=dict(shs=None, shs_p=None, colors_precomp=f))[0], None
        bw = oracle.backward(fw, g, z(7), z(1), z(1), z(1))
        assert np.abs(img.cpu().numpy() - fw["color"]).max() <= 1e-6 * np.abs(fw["color"]).max()
        e = np.abs(grad.cpu().numpy() - bw["dL_dcolors"]).max() / np.abs(bw["dL_dcolors"]).max()
        assert e <= 5e-5, e


# ---- the drop-in -------------------------------------------------------------------------------------------------------

def _pc(scene, dev, dyn_share=0.3, seed=0):
    g = scene["gaussians"]
    P = g["means3D"].shape[0]
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    gen = torch.Generator().manual_seed(seed)
    mask = (torch.rand(P, generator=gen) < dyn_share).to(dev)
    rot_raw = t(g["rotations"]) * 1.7
    normalize = lambda q: torch.nn.functional.normalize(q, dim=-1)
    shs = t(g["shs"])
    return types.SimpleNamespace(get_xyz=t(g["means3D"]), get_opacity=t(g["opacities"]), get_scaling=t(g["scales"]),
                                 _rotation=rot_raw, get_rotation=normalize(rot_raw), rotation_activation=normalize,
                                 get_features_color=shs, get_features_phasor=t(g["shs_p"]), get_motion_mask=mask,
                                 active_sh_degree=3, use_view_dependent_phase=True)


def _tof_cam(scene, dev, gt=None):
    cam = scene["cam"]
    W, H = scene["cfg"]["W"], scene["cfg"]["H"]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    # the scene's own intrinsics (a sensor camera of helpers.CAMERAS), or the centred camera's
    fx = cam.get("fx", W / (2 * cam["tanfovx"]))
    K = t([[fx, 0, cam.get("cx", W / 2)], [0, cam.get("fy", fx), cam.get("cy", H / 2)], [0, 0, 1]])
    return types.SimpleNamespace(tof_image_height=H, tof_image_width=W, FoVx_tof=2 * math.atan(cam["tanfovx"]),
                                 FoVy_tof=2 * math.atan(cam["tanfovy"]), world_view_transform_tof=t(cam["viewmatrix"]),
                                 full_proj_transform_tof=t(cam["projmatrix"]), camera_center_tof=t(cam["campos"]),
                                 znear=cam["znear"], zfar=cam["zfar"], depth_range=torch.tensor(scene["depth_range"]),
                                 K=K, K_tof=K, world_view_transform=t(cam["viewmatrix"]), forward_flow=gt and gt[0],
                                 backward_flow=gt and gt[1])


def render_flow_restated(cam, pc, d_xyz, d_rot, flow3d, bg_color, render_regions=("static", "dynamic")):
    """gaussian_renderer/__init__.py:141-204 with stock-torch masked assignments and GaussianRasterizer."""
    from gftorf_amd import GaussianRasterizationSettings, GaussianRasterizer
    s = GaussianRasterizationSettings(
        image_height=int(cam.tof_image_height), image_width=int(cam.tof_image_width), tanfovx=math.tan(cam.FoVx_tof * 0.5),
        tanfovy=math.tan(cam.FoVy_tof * 0.5), bg=bg_color, scale_modifier=1.0, viewmatrix=cam.world_view_transform_tof,
        projmatrix=cam.full_proj_transform_tof, sh_degree=pc.active_sh_degree, campos=cam.camera_center_tof,
        prefiltered=False, debug=False, near_n=cam.znear, far_n=cam.zfar, depth_range=cam.depth_range.item(),
        use_view_dependent_phase=pc.use_view_dependent_phase, optimize_phase_offset=False, optimize_dc_offset=False)
    m = pc.get_motion_mask
    means3D = torch.zeros(pc.get_xyz.shape, device=pc.get_xyz.device)
    opacity = torch.zeros(pc.get_opacity.shape, device=m.device)
    scales = torch.zeros(pc.get_scaling.shape, device=m.device)
    rotations = torch.zeros(pc.get_rotation.shape, device=m.device)
    flow3d_ = torch.zeros(pc.get_xyz.shape, device=m.device)
    if "static" in render_regions:
        means3D[~m] = pc.get_xyz[~m]
        opacity[~m] = pc.get_opacity[~m]
        scales[~m] = pc.get_scaling[~m]
        rotations[~m] = pc.get_rotation[~m]
    if "dynamic" in render_regions:
        means3D[m] = pc.get_xyz[m] + d_xyz
        opacity[m] = pc.get_opacity[m]
        scales[m] = pc.get_scaling[m]
        rotations[m] = pc.rotation_activation(pc._rotation[m] + d_rot)
        flow3d_[m] = flow3d
    out = GaussianRasterizer(raster_settings=s)(means3D=means3D.detach(), means2D=torch.zeros_like(means3D),
                                                 opacities=opacity.detach(), colors_precomp=flow3d_,
                                                 scales=scales.detach(), rotations=rotations.detach())
    return out[0]


def _deform(pc, dev, seed):
    n = int(pc.get_motion_mask.sum())
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)
    return dict(d_xyz_curr=0.01 * r(n, 3), d_rot=0.05 * r(n, 4), d_xyz=0.01 * r(n, 3), next=0.02 * r(n, 3), prev=0.02 * r(n, 3))


def _flow_iteration(cam, pc, d, bg, fused, with_loss, depth=None):
    """The flow part of train.py:243-261: returns the two images and the gradients of d_xyz_next, d_xyz_prev and d_xyz."""
    from gftorf_amd import flow
    leaves = {k: d[k].clone().requires_grad_() for k in ("d_xyz", "next", "prev")}
    ff, fb = leaves["next"] - leaves["d_xyz"], leaves["prev"] - leaves["d_xyz"]
    if fused:
        imf, imb = flow.render_flow_pair(cam, pc, d["d_xyz_curr"], d["d_rot"], ff, fb, bg)
    else:
        imf = render_flow_restated(cam, pc, d["d_xyz_curr"], d["d_rot"], ff, bg)
        imb = render_flow_restated(cam, pc, d["d_xyz_curr"], d["d_rot"], fb, bg)
    if with_loss:
        lf, lb = flow.flow_loss(depth, cam, imf, imb)
        loss = 0.01 * (lf + lb)
    else:
        gen = torch.Generator().manual_seed(5)
        loss = (imf * torch.randn(imf.shape, generator=gen).to(imf.device)).sum() + (imb * imb).sum()
    loss.backward()
    return imf.detach(), imb.detach(), {k: v.grad for k, v in leaves.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("with_loss", [False, True])
def test_render_flow_pair_is_a_drop_in(with_loss, gpu):
    _drop_in(with_loss, None, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("with_loss", [False, True])
def test_render_flow_pair_is_a_drop_in_through_a_sensor_camera(with_loss, gpu):
    """... with K / K_tof from the camera's own fx, fy, cx, cy (helpers.CAMERAS `sensor`)."""
    _drop_in(with_loss, "sensor", gpu)


def _drop_in(with_loss, camera, gpu):
    W, H = 320, 240
    scene = Hh.small_scene(P=20_000, W=W, H=H, seed=47, scale_lo=0.004, scale_hi=0.03, opacity=0.3, camera=camera)
    pc = _pc(scene, gpu)
    gen = torch.Generator().manual_seed(3)
    gt = [(2.0 * torch.randn((2, H, W), generator=gen)).to(gpu) for _ in range(2)]
    cam = _tof_cam(scene, gpu, gt)
    depth = (1.0 + 4.0 * torch.rand((1, H, W), generator=gen)).to(gpu)
    d = _deform(pc, gpu, 1)
    bg = torch.zeros((7, H, W), device=gpu)
    share = float(pc.get_motion_mask.float().mean())
    assert 0.25 < share < 0.35
    ours = _flow_iteration(cam, pc, d, bg, True, with_loss, depth)
    ref = _flow_iteration(cam, pc, d, bg, False, with_loss, depth)
    torch.cuda.synchronize()
    # the same geometry bit for bit: the forward image is the same rasterizer call's; the backward image is blended over that
    # frame, drawn here by the segment-parallel forward (test_both_forward_kernels)
    assert torch.equal(ours[0], ref[0])
    assert float(ref[1].abs().max()) > 0 and _rel(ref[1], ours[1]) <= 2e-6, _rel(ref[1], ours[1])
    for k in ("d_xyz", "next", "prev"):
        assert float(ref[2][k].abs().max()) > 0, k
        assert _rel(ref[2][k], ours[2][k]) <= 1e-5, (k, _rel(ref[2][k], ours[2][k]))
    # one direction only; the static or the dynamic region only
    from gftorf_amd import flow
    f = (d["next"] - d["d_xyz"])
    assert flow.render_flow_pair(cam, pc, d["d_xyz_curr"], d["d_rot"], None, None, bg) == (None, None)
    none_f, only_b = flow.render_flow_pair(cam, pc, d["d_xyz_curr"], d["d_rot"], None, f, bg)
    assert none_f is None and torch.equal(render_flow_restated(cam, pc, d["d_xyz_curr"], d["d_rot"], f, bg), only_b)
    for regions in (("static",), ("dynamic",)):
        got, _ = flow.render_flow_pair(cam, pc, d["d_xyz_curr"], d["d_rot"], f, None, bg, regions)
        assert torch.equal(got, render_flow_restated(cam, pc, d["d_xyz_curr"], d["d_rot"], f, bg, regions)), regions


@pytest.mark.gpu
def test_no_host_sync(gpu):
    from gftorf_amd import flow
    W, H = 160, 96
    scene = Hh.small_scene(P=5000, W=W, H=H, seed=51)
    pc = _pc(scene, gpu)
    gen = torch.Generator().manual_seed(4)
    cam = _tof_cam(scene, gpu, [(torch.randn((2, H, W), generator=gen)).to(gpu) for _ in range(2)])
    cam.depth_range = float(scene["depth_range"])
    depth = (1.0 + torch.rand((1, H, W), generator=gen)).to(gpu)
    d = _deform(pc, gpu, 2)
    bg = torch.zeros((7, H, W), device=gpu)

    def step():
        leaves = {k: d[k].clone().requires_grad_() for k in ("d_xyz", "next", "prev")}
        imf, imb = flow.render_flow_pair(cam, pc, d["d_xyz_curr"], d["d_rot"], leaves["next"] - leaves["d_xyz"],
                                         leaves["prev"] - leaves["d_xyz"], bg)
        lf, lb = flow.flow_loss(depth, cam, imf, imb)
        (lf + lb).backward()
        return leaves

    step()                    # the first frame of a shape sizes its binning buffer with one blocking read
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        leaves = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in leaves.values())


@pytest.mark.gpu
def test_captured_flow_part_follows_new_flows_and_cameras(gpu):
    from gftorf_amd import flow
    W, H = 160, 96
    scenes = [Hh.small_scene(P=8000, W=W, H=H, seed=61, w2c=Hh.synth.look_at_w2c(0.1 + 0.03 * k, -0.1, 0.05, (0.1, -0.05, 0.2)))
              for k in range(4)]
    pc = _pc(scenes[0], gpu)
    gen = torch.Generator().manual_seed(6)
    gts = [[torch.randn((2, H, W), generator=gen).to(gpu) for _ in range(2)] for _ in scenes]
    depths = [(1.0 + torch.rand((1, H, W), generator=gen)).to(gpu) for _ in scenes]
    cams = [_tof_cam(s, gpu, g) for s, g in zip(scenes, gts)]
    for c in cams:
        c.depth_range = float(scenes[0]["depth_range"])
    ds = [_deform(pc, gpu, 10 + k) for k in range(4)]
    bg = torch.zeros((7, H, W), device=gpu)
    cam_keys = ("world_view_transform_tof", "full_proj_transform_tof", "camera_center_tof", "K", "K_tof",
                "world_view_transform", "forward_flow", "backward_flow")
    static_cam = types.SimpleNamespace(**vars(cams[0]))
    for k in cam_keys:
        setattr(static_cam, k, getattr(cams[0], k).clone())
    static = {k: v.clone() for k, v in ds[0].items()}
    depth = depths[0].clone()
    leaves = {k: static[k].clone().requires_grad_() for k in ("d_xyz", "next", "prev")}

    def step(cam, dd, lv, dep):
        imf, imb = flow.render_flow_pair(cam, pc, dd["d_xyz_curr"], dd["d_rot"], lv["next"] - lv["d_xyz"],
                                         lv["prev"] - lv["d_xyz"], bg)
        lf, lb = flow.flow_loss(dep, cam, imf, imb)
        (0.01 * (lf + lb)).backward()
        return torch.stack([lf.detach(), lb.detach()]), imf.detach(), imb.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            for v in leaves.values():
                v.grad = None
            step(static_cam, static, leaves, depth)
    torch.cuda.current_stream().wait_stream(side)
    for v in leaves.values():
        v.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(static_cam, static, leaves, depth)
    for k in (1, 2, 3):
        with torch.no_grad():
            for key in cam_keys:
                getattr(static_cam, key).copy_(getattr(cams[k], key))
            for key in static:
                static[key].copy_(ds[k][key])
            for key in leaves:
                leaves[key].copy_(ds[k][key])
            depth.copy_(depths[k])
        graph.replay()
        torch.cuda.synchronize()
        lv = {key: ds[k][key].clone().requires_grad_() for key in leaves}
        eager = step(cams[k], ds[k], lv, depths[k])
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert _rel(b, a) <= 1e-5, k
        for key in leaves:
            assert _rel(lv[key].grad, leaves[key].grad) <= 1e-5, (k, key)


@pytest.mark.gpu
def test_render_flow_pair_without_dynamic_gaussians(gpu):
    """No dynamic Gaussian: deformations and flows of no rows, zero flow images and empty gradients, as render_flow gives"""
    W, H = 96, 64
    scene = Hh.small_scene(P=3000, W=W, H=H, seed=71)
    pc = _pc(scene, gpu, dyn_share=0.0)
    assert not bool(pc.get_motion_mask.any())
    cam = _tof_cam(scene, gpu)
    d = _deform(pc, gpu, 3)
    assert d["next"].shape == (0, 3)
    bg = torch.zeros((7, H, W), device=gpu)
    ours = _flow_iteration(cam, pc, d, bg, True, False)
    ref = _flow_iteration(cam, pc, d, bg, False, False)
    torch.cuda.synchronize()
    for a, b in zip(ours[:2], ref[:2]):
        assert torch.equal(a, b) and float(a.abs().max()) == 0.0
    for k in ("d_xyz", "next", "prev"):
        assert ours[2][k] is not None and ours[2][k].shape == ref[2][k].shape == (0, 3), k
