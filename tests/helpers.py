"""Shared helpers of the parity tests: build a scene, run it through the CPU
oracle and through the HIP path (public Python API -> C ABI), compare."""
import contextlib

import numpy as np
import torch

from gftorf_amd import synth

GRAD_KEYS = ["color", "phasor", "depth", "acc", "depth_distortion"]


@contextlib.contextmanager
def deform_modes(**modes):
    """Module switches of gftorf_amd.deform set for a block."""
    from gftorf_amd import deform as D
    old = {k: getattr(D, k) for k in modes}
    try:
        for k, v in modes.items():
            setattr(D, k, v)
        yield D
    finally:
        for k, v in old.items():
            setattr(D, k, v)


# the blocking selection on exactly the rows with a gradient (with `_save_state = {"fraction": 0.0}`: a forward that keeps
# nothing, a host read of the count, buffers and launches of exactly that size): the reference of every rows test
DEFORM_BLOCKING = dict(device_row_count=False, lazy_save=True, _SPARSE_MAX_FRACTION=2.0)


# Sensor cameras (the reference hands every colour and ToF camera its own fx, fy, cx, cy: scene/dataset_readers.py:360-375,
# and builds the projection with getProjectionMatrixShift: scene/cameras.py:122-140).  Focal lengths as fractions of
# f0 = W / (2 tan 30 deg) (the centred camera's) or, where `of_size` is set, of the image size; the principal point as a
# fraction of the image size: one entry works at every image size.  `z`: the depth range its scenes use when the caller
# names none.
CAMERAS = {
    # tests/golden/camera.npz's shift_args: 320 x 240, fx 260, fy 262, cx 155.5, cy 118.25
    "sensor": dict(fx=260.0 / 320.0, fy=262.0 / 240.0, of_size=True, cx=155.5 / 320.0, cy=118.25 / 240.0),
    "shift_right": dict(fx=1.0, fy=1.0, cx=0.72, cy=0.5),
    "shift_corner": dict(fx=1.0, fy=1.0, cx=0.25, cy=0.78),
    "anisotropic": dict(fx=1.3, fy=0.8, cx=0.55, cy=0.45),
    "tele": dict(fx=4.0, fy=4.0, cx=0.5, cy=0.6),
    "wide": dict(fx=0.45, fy=0.45, cx=0.4, cy=0.5),
    # ToFCamera's own defaults (scene/cameras.py): near 0.01, far 100, depth_range 100
    "default_planes": dict(fx=1.0, fy=1.0, cx=0.52, cy=0.48, znear=0.01, zfar=100.0, depth_range=100.0, z=(0.02, 90.0)),
}


def sensor_camera(camera, W, H, w2c=None):
    """synth.make_sensor_camera of an entry of CAMERAS (by name, or a dict of the same form) at the image size W x H."""
    e = CAMERAS[camera] if isinstance(camera, str) else camera
    f0 = W / (2.0 * np.tan(np.radians(30.0)))
    fx = e["fx"] * (W if e.get("of_size") else f0)
    fy = e["fy"] * (H if e.get("of_size") else f0)
    return synth.make_sensor_camera(W, H, float(fx), float(fy), e["cx"] * W, e["cy"] * H, znear=e.get("znear", 0.45),
                                    zfar=e.get("zfar", 6.05), w2c=w2c)


def small_scene(P=400, W=80, H=48, seed=3, D=3, sh_coeffs=16, scale_lo=0.01, scale_hi=0.12,
                w2c="tilted", spread=1.05, tof=True, opacity=None, z_lo=None, z_hi=None, camera=None, depth_range=10.0):
    """camera: None (synth.make_camera, the centred 60 degree one), a name from CAMERAS or a dict of that form; the
    Gaussians are placed in that camera's frustum, and the entry's depth_range, where it has one, replaces the argument.
    z_lo / z_hi default to 1.0 / 5.5, or to the camera entry's `z`."""
    if isinstance(w2c, str):
        w2c = synth.look_at_w2c(0.15, -0.1, 0.05, (0.1, -0.05, 0.2)) if w2c == "tilted" else None
    zr = (1.0, 5.5)
    if camera is None:
        cam = synth.make_camera(W, H, w2c=w2c)
    else:
        e = CAMERAS[camera] if isinstance(camera, str) else camera
        cam = sensor_camera(e, W, H, w2c=w2c)
        depth_range = e.get("depth_range", depth_range)
        zr = e.get("z", zr)
    z_lo = zr[0] if z_lo is None else z_lo
    z_hi = zr[1] if z_hi is None else z_hi
    g = synth.make_gaussians(P, cam, seed, sh_coeffs=sh_coeffs, scale_lo=scale_lo, scale_hi=scale_hi,
                             spread=spread, z_lo=z_lo, z_hi=z_hi)
    if not tof:
        g["shs_p"] = None
    if opacity is not None:
        g["opacities"] = np.full_like(g["opacities"], opacity)
    return dict(cfg=dict(P=P, W=W, H=H, D=D, sh_coeffs=sh_coeffs, tof=tof), cam=cam, gaussians=g,
                bg=synth.make_background(W, H, seed), grads=synth.make_pixel_grads(W, H, seed),
                depth_range=depth_range, phase_offset=0.1, dc_offset=0.05, use_view_dependent_phase=True)


PLANES = {"bench": (0.45, 6.05, 10.0), "tof_default": (0.01, 100.0, 100.0)}      # near, far, depth_range


def plane_edge_scene(znear, zfar, depth_range, W=48, H=32, per_depth=4):
    """Gaussians at `near`, `far` and the floats next to each on both sides, under the identity pose, where the view-space
    z is the world z exactly.  The reference culls with `<` and `>` (auxiliary.h:169): one exactly on a plane is kept.
    Returns (scene, kept): kept[i] says whether Gaussian i lies on or between the planes."""
    zn, zf, inf = np.float32(znear), np.float32(zfar), np.float32(np.inf)
    depths = [np.nextafter(zn, -inf), zn, np.nextafter(zn, inf), np.nextafter(zf, -inf), zf, np.nextafter(zf, inf)]
    inside = [False, True, True, True, True, False]
    P = len(depths) * per_depth
    sc = small_scene(P=P, W=W, H=H, w2c=None, depth_range=depth_range)
    cam = synth.make_camera(W, H, znear=znear, zfar=zfar)
    z = np.repeat(np.array(depths, np.float32), per_depth)
    rng = np.random.default_rng(77)
    u, v = rng.uniform(-0.7, 0.7, P), rng.uniform(-0.7, 0.7, P)
    g = dict(sc["gaussians"])
    g["means3D"] = np.stack([u * z * cam["tanfovx"], v * z * cam["tanfovy"], z], 1).astype(np.float32)
    g["means3D"][:, 2] = z
    g["scales"] = (g["scales"] * (z[:, None] / np.float32(3.0))).astype(np.float32)     # the same size on screen at every depth
    g["opacities"] = np.full_like(g["opacities"], 0.5)
    return dict(sc, cam=cam, gaussians=g), np.repeat(np.array(inside), per_depth)


def translated_pair(dx, dy, camera="anisotropic", **kw):
    """Two scenes of the same Gaussians and pose whose principal points differ by (dx, dy) pixels: the second image is the first
    one moved by (dx, dy).  With dx, dy multiples of the 16 pixel tile every tile-relative quantity moves with it.  Zero
    background; the upstream gradients are zero outside the overlap and translated inside it."""
    a = small_scene(camera=camera, **kw)
    W, H = a["cfg"]["W"], a["cfg"]["H"]
    e = dict(CAMERAS[camera] if isinstance(camera, str) else camera)
    e["cx"], e["cy"] = e["cx"] + dx / W, e["cy"] + dy / H
    cam_b = sensor_camera(e, W, H, w2c=a["cam"]["w2c"])
    a["bg"] = np.zeros_like(a["bg"])
    ga, gb = {}, {}
    for k, v in a["grads"].items():
        ga[k], gb[k] = np.zeros_like(v), np.zeros_like(v)
        va, vb = overlap(ga[k], gb[k], dx, dy)
        src, _ = overlap(v, v, dx, dy)
        va[...] = src
        vb[...] = src
    a["grads"] = ga
    return a, dict(a, cam=cam_b, grads=gb)


def overlap(img_a, img_b, dx, dy):
    """Views of the pixels that both images of translated_pair see: img_b[..., y + dy, x + dx] is img_a[..., y, x]."""
    H, W = img_a.shape[-2:]
    x0, x1, y0, y1 = max(0, -dx), min(W, W - dx), max(0, -dy), min(H, H - dy)
    return img_a[..., y0:y1, x0:x1], img_b[..., y0 + dy:y1 + dy, x0 + dx:x1 + dx]


def rect_inside_both(means2D, radii, W, H, dx, dy, margin=1.0):
    """Gaussians (of the first scene of translated_pair) whose square of `radii` pixels lies inside both images, with a
    margin: their tile rectangle is clipped by neither image."""
    r = radii.astype(np.float64)
    ok = radii > 0
    for lo, hi, d, size in ((means2D[:, 0] - r, means2D[:, 0] + r, dx, W), (means2D[:, 1] - r, means2D[:, 1] + r, dy, H)):
        ok &= (lo >= margin) & (hi <= size - 1 - margin) & (lo + d >= margin) & (hi + d <= size - 1 - margin)
    return ok


TRANSLATED = {
    # scenes of the whole-tile translation property (translated_pair).  spread 1.6: the Gaussians cover both images
    "base": dict(P=600, W=96, H=64, spread=1.6),
    "opaque": dict(P=3000, W=96, H=64, spread=1.6, scale_lo=0.03, scale_hi=0.2, opacity=0.9, seed=7),
    "small_sensor": dict(P=1500, W=80, H=48, spread=1.6, scale_lo=0.005, scale_hi=0.06, seed=11, camera="sensor"),
}


def beyond_the_clamp_on_screen(scene, f):
    """Gaussians that are blended (`radii > 0`, `pixels > 0`), whose centre lies inside the image and whose view-space
    t.x / t.z or t.y / t.z is beyond computeCov2D's 1.3 tanfov clamp (forward.cu computeCov2D: their Jacobian is taken at
    the clamped point and x_grad_mul / y_grad_mul = 0).  Only a principal point away from the centre has any."""
    cam, cfg = scene["cam"], scene["cfg"]
    m = scene["gaussians"]["means3D"].astype(np.float64)
    t = np.concatenate([m, np.ones((m.shape[0], 1))], 1) @ cam["viewmatrix"].astype(np.float64)
    beyond = (np.abs(t[:, 0] / t[:, 2]) > 1.3 * cam["tanfovx"]) | (np.abs(t[:, 1] / t[:, 2]) > 1.3 * cam["tanfovy"])
    m2 = f.geom["means2D"]
    inside = (m2[:, 0] >= 0) & (m2[:, 0] <= cfg["W"] - 1) & (m2[:, 1] >= 0) & (m2[:, 1] <= cfg["H"] - 1)
    return (f.radii > 0) & (f.pixels.reshape(-1) > 0) & inside & beyond


def oracle_kwargs(scene, **over):
    cam, cfg = scene["cam"], scene["cfg"]
    kw = dict(bg=scene["bg"], viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"],
              campos=cam["campos"], image_height=cfg["H"], image_width=cfg["W"],
              tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], sh_degree=cfg["D"],
              near_n=cam["znear"], far_n=cam["zfar"], depth_range=scene["depth_range"],
              use_view_dependent_phase=scene["use_view_dependent_phase"],
              phase_offset=scene["phase_offset"], dc_offset=scene["dc_offset"])
    kw.update(over)
    return kw


def run_oracle(oracle, scene, backward=True, inputs=None, **over):
    g = dict(scene["gaussians"])
    if inputs:
        g.update(inputs)
    kw = oracle_kwargs(scene, **over)
    f = oracle.forward(g["means3D"], g["opacities"], shs=g.get("shs"), shs_p=g.get("shs_p"),
                       colors_precomp=g.get("colors_precomp"), phasors_precomp=g.get("phasors_precomp"),
                       scales=g.get("scales"), rotations=g.get("rotations"),
                       cov3D_precomp=g.get("cov3D_precomp"), **kw)
    b = None
    if backward:
        gr = scene["grads"]
        b = oracle.backward(f, gr["color"], gr["phasor"], gr["depth"], gr["acc"], gr["depth_distortion"])
    return f, b


def gpu_settings(scene, dev, bg=None, debug=False, optimize_offsets=False, **over):
    from gftorf_amd import GaussianRasterizationSettings
    cam, cfg = scene["cam"], scene["cfg"]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    kw = dict(image_height=cfg["H"], image_width=cfg["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
              bg=t(scene["bg"]) if bg is None else bg, scale_modifier=1.0,
              viewmatrix=t(cam["viewmatrix"]), projmatrix=t(cam["projmatrix"]), sh_degree=cfg["D"],
              campos=t(cam["campos"]), prefiltered=False, debug=debug, near_n=cam["znear"],
              far_n=cam["zfar"], depth_range=scene["depth_range"],
              use_view_dependent_phase=scene["use_view_dependent_phase"],
              optimize_phase_offset=optimize_offsets, optimize_dc_offset=optimize_offsets)
    kw.update(over)
    return GaussianRasterizationSettings(**kw)


def gpu_rasterizer(scene, dev, **over):
    from gftorf_amd import GaussianRasterizer
    return GaussianRasterizer(raster_settings=gpu_settings(scene, dev, **over))


OUT_NAMES = ["color", "phasor", "depth", "normal", "acc", "entropy", "depth_distortion",
             "amp_distortion", "pixels", "distribution", "radii"]


def run_gpu(scene, dev, backward=True, inputs=None, settings=None, optimize_offsets=False, **over):
    """Runs the public API on the HIP device.  Returns (outputs dict of numpy, grads dict of numpy,
    tensors dict)."""
    from gftorf_amd import GaussianRasterizer
    g = dict(scene["gaussians"])
    if inputs:
        g.update(inputs)
    P = g["means3D"].shape[0]
    leaf = {}
    for k, v in g.items():
        if v is None:
            continue
        leaf[k] = torch.tensor(v, dtype=torch.float32, device=dev, requires_grad=backward)
    means2D = torch.zeros((P, 3), dtype=torch.float32, device=dev, requires_grad=backward)
    if settings is None:
        settings = gpu_settings(scene, dev, optimize_offsets=optimize_offsets, **over)
    if optimize_offsets:
        ph = torch.tensor([scene["phase_offset"]], dtype=torch.float32, device=dev, requires_grad=True)
        dc = torch.tensor([scene["dc_offset"]], dtype=torch.float32, device=dev, requires_grad=True)
    else:
        ph, dc = scene["phase_offset"], scene["dc_offset"]
    rast = GaussianRasterizer(raster_settings=settings)
    outs = rast(means3D=leaf["means3D"], means2D=means2D, opacities=leaf["opacities"],
                shs=leaf.get("shs"), shs_p=leaf.get("shs_p"), colors_precomp=leaf.get("colors_precomp"),
                phasors_precomp=leaf.get("phasors_precomp"), scales=leaf.get("scales"),
                rotations=leaf.get("rotations"), cov3D_precomp=leaf.get("cov3D_precomp"),
                phase_offset=ph, dc_offset=dc)
    assert len(outs) == 11
    o = dict(zip(OUT_NAMES, outs))
    grads = None
    if backward:
        gr = scene["grads"]
        loss = sum((o[k] * torch.tensor(gr[k], device=dev)).sum() for k in GRAD_KEYS)
        loss.backward()
        grads = {k: (v.grad.detach().cpu().numpy() if v.grad is not None else None) for k, v in leaf.items()}
        grads["means2D"] = means2D.grad.detach().cpu().numpy()
        if optimize_offsets:
            grads["phase_offset"] = ph.grad.detach().cpu().numpy()
            grads["dc_offset"] = dc.grad.detach().cpu().numpy()
    torch.cuda.synchronize()
    out_np = {k: v.detach().cpu().numpy() for k, v in o.items()}
    return out_np, grads, dict(leaf=leaf, outs=o, means2D=means2D)


def rel_err(ref, got):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    den = np.abs(ref).max()
    return float(np.abs(ref - got).max() / (den + 1e-30)), float(den)


def assert_close(name, ref, got, rtol_max=2e-4, atol=1e-6, frac_bad=0.0, rtol_elem=None):
    """max-norm relative check: |ref-got|_inf <= rtol_max * |ref|_inf + atol.
    frac_bad > 0 tolerates that fraction of elements outside an element-wise band
    (discrete skip/termination flips on borderline alphas)."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    assert ref.shape == got.shape, "%s: shape %s vs %s" % (name, ref.shape, got.shape)
    if ref.size == 0:
        return
    assert np.isfinite(got).all(), "%s: non-finite values" % name
    den = np.abs(ref).max()
    err = np.abs(ref - got)
    if frac_bad > 0.0:
        tol = (rtol_elem or rtol_max) * den + atol
        bad = (err > tol).mean()
        assert bad <= frac_bad, "%s: %.3g of elements differ by more than %.3g (max err %.3g, scale %.3g)" % (
            name, bad, tol, err.max(), den)
    else:
        assert err.max() <= rtol_max * den + atol, "%s: max err %.3g > %.3g*%.3g+%.3g" % (
            name, err.max(), rtol_max, den, atol)


class _OracleRasterize(torch.autograd.Function):
    """The CPU oracle behind the operator's autograd surface (CPU tensors): forward = oracle.forward, backward =
    oracle.backward.  Stand-in for the HIP rasterizer where a composed step is rehearsed without a GPU."""

    @staticmethod
    def forward(ctx, oracle, kw, means3D, means2D, opacities, shs, shs_p, scales, rotations):
        n = lambda t: t.detach().cpu().numpy()
        f = oracle.forward(n(means3D), n(opacities), shs=n(shs), shs_p=n(shs_p), scales=n(scales), rotations=n(rotations), **kw)
        ctx.oracle, ctx.f, ctx.op_shape = oracle, f, opacities.shape
        t = lambda a: torch.tensor(np.asarray(a))
        outs = (t(f.color), t(f.phasor), t(f.depth), t(f.normal), t(f.acc), t(f.entropy), t(f.depth_distortion),
                t(f.amp_distortion), t(f.pixels), t(f.distribution), t(f.radii))
        ctx.mark_non_differentiable(outs[10])
        return outs

    @staticmethod
    def backward(ctx, g_color, g_phasor, g_depth, _gn, g_acc, _ge, g_dd, *_rest):
        f = ctx.f
        z = lambda g, c: np.zeros((c, f.H, f.W), np.float32) if g is None else g.detach().numpy()
        b = ctx.oracle.backward(f, z(g_color, 3), z(g_phasor, 7), z(g_depth, 1), z(g_acc, 1), z(g_dd, 1))
        t = lambda a: torch.tensor(np.asarray(a, np.float32))
        return (None, None, t(b["dL_dmeans3D"]), t(b["dL_dmeans2D"]), t(b["dL_dopacity"]).reshape(ctx.op_shape), t(b["dL_dsh"]),
                t(b["dL_dsh_p"]), t(b["dL_dscales"]), t(b["dL_drotations"]))


def oracle_rasterizer(oracle, scene, **over):
    """render(frame_id, means3D=, means2D=, opacities=, shs=, shs_p=, scales=, rotations=) -> 11-tuple, on the CPU oracle."""
    kw = oracle_kwargs(scene, **over)

    def render(frame_id, means3D, means2D, opacities, shs, shs_p, scales, rotations):
        return _OracleRasterize.apply(oracle, kw, means3D, means2D, opacities, shs, shs_p, scales, rotations)
    return render


# ---------------------------------------------------------------------------
# The paths of dL/dmeans3D (tests/test_grad_paths.py, tests/test_gpu_grad_paths.py): a Gaussian's position is used eight
# times (torch_ref.PATHS), and its gradient is the sum of one term per use.  A whole-tensor max-norm sees the largest
# term only (the projected mean: 0.99 of |dL/dmeans3D|_inf in small_scene()); here every term is a yardstick of its own.
PATH_CASES = {      # upstream case -> {plane: its channels that are non-zero}; every other upstream value is an exact zero
    "color": dict(color=slice(0, 3)),
    "phasor01": dict(phasor=slice(0, 2)),
    "phasor2": dict(phasor=slice(2, 3)),
    "phasor3to6": dict(phasor=slice(3, 7)),
    "depth": dict(depth=slice(0, 1)),
    "acc": dict(acc=slice(0, 1)),
    "depth_distortion": dict(depth_distortion=slice(0, 1)),
    "all": {k: slice(None) for k in GRAD_KEYS},
    "phasor": dict(phasor=slice(0, 7)),          # (the whole plane: for the shares of DESIGN.md section 11b, not a GPU case)
}
_PHASOR_PATHS = ("mean2D", "cov_t", "dir_phasor", "dist_phase", "dist_factor")
CASE_PATHS = {      # the paths that exist for a case (every other part of dL/dmeans3D is an exact zero)
    "color": ("mean2D", "cov_t", "dir_color"),
    "phasor01": _PHASOR_PATHS,
    "phasor2": ("mean2D", "cov_t", "dir_phasor", "dist_factor"),      # amplitude / dist^2: no phase
    "phasor3to6": _PHASOR_PATHS,
    "phasor": _PHASOR_PATHS,
    "depth": ("mean2D", "cov_t", "dist_depth"),
    "acc": ("mean2D", "cov_t"),
    "depth_distortion": ("mean2D", "cov_t", "dist_ndc"),
    "all": ("mean2D", "cov_t", "dir_color", "dir_phasor", "dist_phase", "dist_factor", "dist_depth", "dist_ndc"),
}
GPU_PATH_CASES = ("color", "phasor01", "phasor2", "phasor3to6", "depth", "acc", "depth_distortion", "all")
PHASOR_CASES = ("phasor01", "phasor2", "phasor3to6")


def case_paths(case, scene, inputs=None):
    """CASE_PATHS under the scene's argument pattern: precomputed colours have no view direction; precomputed phasors have
    neither a view direction nor, in the reference's backward, any phasor chain (torch_ref's docstring)."""
    g = dict(scene["gaussians"], **(inputs or {}))
    drop = set()
    if g.get("shs") is None:
        drop.add("dir_color")
    if g.get("shs_p") is None:
        drop |= {"dir_phasor", "dist_phase", "dist_factor"}
    return tuple(p for p in CASE_PATHS[case] if p not in drop)


def case_upstream(scene, case):
    """scene["grads"] with everything outside the case's channels set to zero."""
    up = {k: np.zeros_like(v) for k, v in scene["grads"].items()}
    for k, sl in PATH_CASES[case].items():
        up[k][sl] = scene["grads"][k][sl]
    return up


def path_scene(D=3, vdp=True):
    """A scene in which every path of dL/dmeans3D is large: 120 Gaussians, 48 x 32, near the wide camera (z 0.5 .. 1.5:
    directions and distances change fast), large splats, and higher SH degrees of size 0.5 (colour) and 0.3 (phasor)
    instead of synth's 0.1 and 0.05.  All 120 Gaussians are blended; 60 of them have a clamped colour channel, 23 a
    clamped amplitude.  Shares of |dL/dmeans3D|_inf per path when only the named upstream plane is non-zero (float64,
    tests/test_grad_paths.py asserts that each is at least 0.05):
        color              mean2D 0.94, cov_t 0.63, dir_color 0.57
        phasor             mean2D 0.50, cov_t 0.24, dir_phasor 0.52, dist_phase 0.36, dist_factor 0.87
        depth              mean2D 0.88, cov_t 0.20, dist_depth 0.38
        acc                mean2D 0.95, cov_t 0.19
        depth_distortion   mean2D 0.35, cov_t 0.30, dist_ndc 0.56
        all five together  mean2D 0.93, cov_t 0.33, dir_color 0.41, dir_phasor 0.41, dist_phase 0.29, dist_factor 0.68,
                           dist_depth 0.094, dist_ndc 0.030
    Seed 7: with seed 5 (shares as low as 0.089) one pair of the walk has |alpha - 1/255| = 2.0e-7, inside the 1e-4 / 255
    that test_grad_paths.py asks for; here the closest pair is 1.2e-6 away, |power| >= 3.5e-5, |test_T - 1e-4| >= 8.4e-4,
    and no SH sum is within 4.9e-4 of its clamp.
    D, vdp: the SH degree in use (of 16 coefficients) and use_view_dependent_phase."""
    sc = small_scene(P=120, W=48, H=32, D=D, scale_lo=0.05, scale_hi=0.3, z_lo=0.5, z_hi=1.5, camera="wide", seed=7)
    rng = np.random.default_rng(1)
    g = sc["gaussians"]
    g["shs"][:, 1:, :] = rng.normal(0, 0.5, g["shs"][:, 1:, :].shape).astype(np.float32)
    g["shs_p"][:, 1:, :] = rng.normal(0, 0.3, g["shs_p"][:, 1:, :].shape).astype(np.float32)
    sc["use_view_dependent_phase"] = vdp
    return sc


def isolated_scene(seed=20):
    """12 Gaussians on a 4 x 3 grid of a 48 x 32 image (identity pose, the centred camera) whose 3 sigma extents do not
    overlap: every pixel blends one Gaussian at most, so a row of a gradient tensor is one Gaussian's own sum.  Opacities
    0.02 .. 0.9, screen-space sigmas 0.45 .. 1.45 pixels and depths 0.6 .. 4 make the rows' sizes span decades (asserted in
    tests/test_grad_paths.py), which a whole-tensor norm never looks at."""
    W, H, nx, ny = 48, 32, 4, 3
    P = nx * ny
    sc = small_scene(P=P, W=W, H=H, w2c=None, seed=seed)
    cam = sc["cam"]
    rng = np.random.default_rng(seed + 500)
    focal = W / (2.0 * cam["tanfovx"])
    order = rng.permutation(P)
    cx = ((order % nx) + 0.5) * (W / nx) - 0.5 + rng.uniform(-0.4, 0.4, P)
    cy = ((order // nx) + 0.5) * (H / ny) - 0.5 + rng.uniform(-0.4, 0.4, P)
    z = np.exp(np.linspace(np.log(0.5), np.log(5.5), P))
    sigma_px = np.linspace(1.45, 0.35, P)                     # 3 sqrt(1.45^2 + 0.3) = 4.7 < 16/3 - 0.4, half a cell less the jitter
    g = sc["gaussians"]
    g["means3D"] = np.stack([(cx - (W - 1) / 2.0) / focal * z, (cy - (H - 1) / 2.0) / focal * z, z], 1).astype(np.float32)
    g["scales"] = ((sigma_px * z / focal)[:, None] * rng.uniform(0.5, 1.0, (P, 3))).astype(np.float32)
    g["opacities"] = np.exp(np.linspace(np.log(0.9), np.log(0.02), P))[:, None].astype(np.float32)
    return sc


_GRAD_NAMES = dict(means3D="dL_dmeans3D", means2D="dL_dmeans2D", opacities="dL_dopacity", scales="dL_dscales",
                   rotations="dL_drotations", shs="dL_dsh", shs_p="dL_dsh_p", colors_precomp="dL_dcolors",
                   cov3D_precomp="dL_dcov3D", phase_offset="dL_dphase_offset", dc_offset="dL_ddc_offset")


def oracle_grads(b, scene, inputs=None):
    """The oracle's backward under the names and shapes of run_gpu's gradients."""
    g = dict(scene["gaussians"], **(inputs or {}))
    out = {}
    for k, n in _GRAD_NAMES.items():
        if k in ("means2D", "phase_offset", "dc_offset"):      # no input array of that name
            out[k] = b[n]
        elif g.get(k) is not None:
            out[k] = b[n].reshape(g[k].shape)
    return out


def path_variant(name):
    """The scenes of the path tests: (scene, inputs, upstream cases)."""
    if name == "base":
        return path_scene(), None, GPU_PATH_CASES
    if name in ("D1", "D2"):                       # degrees 1 and 2 of 16 coefficients: the higher columns are exact zeros
        return path_scene(D=int(name[1])), None, ("color",) + PHASOR_CASES
    if name == "no_vdp":                           # use_view_dependent_phase off: the SH phase is not used, the amplitude is
        return path_scene(vdp=False), None, PHASOR_CASES
    rng = np.random.default_rng(9)
    if name == "phasors_precomp":
        pp = np.stack([rng.uniform(-0.5, 0.5, 120), rng.uniform(0.05, 0.5, 120)], 1).astype(np.float32)
        return path_scene(), dict(shs_p=None, phasors_precomp=pp), PHASOR_CASES
    if name == "colors_precomp":
        return path_scene(), dict(shs=None, colors_precomp=rng.random((120, 3)).astype(np.float32)), ("color",)
    raise KeyError(name)


PATH_VARIANTS = ("base", "D1", "D2", "no_vdp", "phasors_precomp", "colors_precomp")
_F64_CACHE = {}


def path_reference(name, oracle, cases=None, margins=None):
    """path_variant(name) with the oracle's forward and the float64 gradients of its cases: (scene, inputs, f, ref)."""
    scene, inputs, own = path_variant(name) if name != "isolated" else (isolated_scene(), None, ("all",))
    if name == "base" and cases is None:
        cases = GPU_PATH_CASES + ("phasor",)      # (the whole phasor plane too: its shares are asserted on the CPU)
    f, _ = run_oracle(oracle, scene, backward=False, inputs=inputs)
    return scene, inputs, f, float64_case_grads(name, scene, f, cases or own, inputs=inputs, margins=margins)


def oracle_case_grads(oracle, scene, f, case, inputs=None):
    up = case_upstream(scene, case)
    return oracle_grads(oracle.backward(f, up["color"], up["phasor"], up["depth"], up["acc"], up["depth_distortion"]), scene, inputs)


def gpu_case_grads(scene, dev, case, inputs=None, **over):
    return run_gpu(dict(scene, grads=case_upstream(scene, case)), dev, inputs=inputs, optimize_offsets=True, **over)[1]


def float64_case_grads(key, scene, f, cases, inputs=None, margins=None):
    """The float64 gradients (tests/torch_ref.py, autograd) of `scene` for each upstream case of `cases` (names of
    PATH_CASES), blending the lists of the oracle's forward `f`.  Returns {case: grads}: grads[input] for every input that
    has a gradient, "means2D" [P, 2], "phase_offset" / "dc_offset" (the scalars) with "phase_offset_abs" / "dc_offset_abs"
    (the sums of the absolute per-Gaussian terms: the offsets are given to torch_ref per Gaussian), and "parts":
    {path: that path's term of dL/dmeans3D}, each equal to the full gradient minus the one with that use detached
    (settings["detach"]) but taken from the same backward: dL/d(use), carried on to means3D.
    key: results are computed once per key and shared; nobody writes to them.  margins: torch_ref's settings["margins"]."""
    import torch_ref
    key = (key, tuple(cases))
    if key in _F64_CACHE and margins is None:
        return _F64_CACHE[key]
    dt = torch.float64
    g = dict(scene["gaussians"], **(inputs or {}))
    P = g["means3D"].shape[0]
    params = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in g.items() if v is not None}
    for k in ("shs", "shs_p", "colors_precomp", "phasors_precomp", "cov3D_precomp", "scales", "rotations"):
        params.setdefault(k, None)
    params["phase_offset"] = torch.full((P,), scene["phase_offset"], dtype=dt, requires_grad=True)
    params["dc_offset"] = torch.full((P,), scene["dc_offset"], dtype=dt, requires_grad=True)
    out = torch_ref.render(params, f, oracle_kwargs(scene, split_uses=True, margins=margins))
    names = [k for k, v in params.items() if v is not None]
    uses = [(n, t) for n in torch_ref.PATHS for t in out["uses"].get(n, []) if t.requires_grad]
    res = {}
    for case in cases:
        up = case_upstream(scene, case)
        loss = sum((out[k] * torch.tensor(up[k], dtype=dt)).sum() for k in GRAD_KEYS)
        got = torch.autograd.grad(loss, [params[k] for k in names] + [out["ndc"]] + [t for _, t in uses],
                                  retain_graph=True, allow_unused=True)
        z = lambda gr, like: torch.zeros_like(like) if gr is None else gr
        r = {k: z(gr, params[k]).numpy() for k, gr in zip(names, got)}
        r["means2D"] = z(got[len(names)], out["ndc"]).numpy()
        for k in ("phase_offset", "dc_offset"):
            r[k + "_abs"] = float(np.abs(r[k]).sum())
            r[k] = np.array([r[k].sum()])
        parts = {n: np.zeros((P, 3)) for n in torch_ref.PATHS}
        for (n, t), gr in zip(uses, got[len(names) + 1:]):
            if gr is not None:
                parts[n] = parts[n] + torch.autograd.grad(t, params["means3D"], grad_outputs=gr, retain_graph=True)[0].numpy()
        r["parts"] = parts
        res[case] = r
    _F64_CACHE[key] = res
    return res


def check_path_case(tag, case, ref, got, paths, rtol, f=None, D=3, rows=False):
    """The measure of tests/test_gpu_grad_paths.py.  ref: float64_case_grads(...)[case]; got: gradients under run_gpu's names
    (a device's, or oracle_grads'); paths: the paths that exist (case_paths); f: the oracle's forward (the clamp bits).
      means3D    |got - ref|_inf <= rtol * min over `paths` of |that path's part|_inf
      shs, shs_p, colors_precomp per (coefficient, channel) column: <= rtol * the column's max over rows; columns whose reference is zero
                 everywhere (inactive degrees, a plane without that input) are exact zeros
      clamp bits where clamped[row, c]: dL/dshs[row, :, c] == 0; where clamped_p[row]: dL/dshs_p[row, :, 1] == 0; exactly
      scales, rotations, opacities, means2D, cov3D_precomp: <= rtol * the tensor's max-norm; means2D[:, 2] == 0
      phase_offset, dc_offset (where `got` has them): <= rtol * the sum of the absolute per-Gaussian terms; exact zeros
                 where every term is zero
    rows=True (isolated_scene): instead, every row of every tensor against rtol * its own max.
    Returns (ratios, failures): {quantity: worst error / its yardstick} (to be compared with rtol) and a list of messages."""
    ratios, bad = {}, []

    def ratio(name, err, scale):
        if scale == 0.0:
            if err != 0.0:
                bad.append("%s %s %s: %.3g where the reference is an exact zero" % (tag, case, name, err))
            return
        ratios[name] = max(ratios.get(name, 0.0), err / scale)
        if not err <= rtol * scale:
            bad.append("%s %s %s: error %.3g = %.3g of its yardstick %.3g (bound %.3g)" % (tag, case, name, err, err / scale, scale, rtol))

    def f64(a):
        a = np.asarray(a, np.float64)
        assert np.isfinite(a).all(), "%s %s: non-finite gradient" % (tag, case)
        return a

    m2 = f64(got["means2D"])
    if not (m2[:, 2] == 0).all():
        bad.append("%s %s means2D[:, 2] is not zero" % (tag, case))
    tensors = dict(means3D=(ref["means3D"], f64(got["means3D"])), means2D=(ref["means2D"], m2[:, :2]))
    for k in ("opacities", "scales", "rotations", "shs", "shs_p", "colors_precomp", "cov3D_precomp"):
        if ref.get(k) is not None and got.get(k) is not None:
            tensors[k] = (ref[k], f64(got[k]).reshape(ref[k].shape))
    if rows:
        for k, (r, g_) in tensors.items():
            r2, g2 = r.reshape(r.shape[0], -1), g_.reshape(r.shape[0], -1)
            for i in range(r2.shape[0]):
                ratio(k + " rows", float(np.abs(g2[i] - r2[i]).max()), float(np.abs(r2[i]).max()))
        return ratios, bad
    for k, (r, g_) in tensors.items():
        err = np.abs(g_ - r)
        if k == "means3D":
            ratio("means3D / smallest path", float(err.max()), min(float(np.abs(ref["parts"][p]).max()) for p in paths))
            ratios["means3D / max-norm"] = float(err.max()) / float(np.abs(r).max())
        elif k in ("shs", "shs_p", "colors_precomp"):
            r3, e3 = r.reshape(r.shape[0], -1, r.shape[-1]), err.reshape(r.shape[0], -1, r.shape[-1])
            for j in range(r3.shape[1]):
                for c in range(r3.shape[2]):
                    if j >= (D + 1) ** 2 and (np.abs(r3[:, j, c]).max() != 0.0):
                        bad.append("%s %s: the reference has a gradient at an inactive coefficient" % (tag, case))
                    ratio("%s columns" % k, float(e3[:, j, c].max()), float(np.abs(r3[:, j, c]).max()))
        else:
            ratio(k, float(err.max()), float(np.abs(r).max()))
    if f is not None and "shs" in tensors:
        cl = f.geom["clamped"].astype(bool)
        if tensors["shs"][1].transpose(0, 2, 1)[cl].any():
            bad.append("%s %s: dL/dshs is not zero at a clamped colour channel" % (tag, case))
    if f is not None and "shs_p" in tensors:
        if tensors["shs_p"][1][f.geom["clamped_p"].astype(bool), :, 1].any():
            bad.append("%s %s: dL/dshs_p's amplitude column is not zero at a clamped amplitude" % (tag, case))
    for k in ("phase_offset", "dc_offset"):
        if got.get(k) is not None:
            ratio(k, float(np.abs(f64(got[k]).reshape(-1)[0] - ref[k][0])), ref[k + "_abs"])
    return ratios, bad


# ---------------------------------------------------------------------------
# Degenerate Gaussians (tests/test_hostile_rows.py, tests/test_gpu_hostile.py): rows that training produces and
# synth.make_gaussians never does -- collapsed axes, unnormalised quaternions, raw opacities, clones, points behind the camera,
# a Gaussian that covers the frame -- each under a name, so that a test can hold every one of them to its own yardstick.
HOSTILE_W, HOSTILE_H, HOSTILE_P = 48, 32, 160
HOSTILE_ROWS = (
    "zero3", "zero1", "needle", "pancake", "giant",
    "q_small", "q_large", "q_zero", "q_negw",
    "op_zero", "op_one", "op_above_one", "op_negative", "thr_below", "thr_above", "thr_exact",
    "behind", "at_camera", "pixel_centre", "tile_corner", "off_one_tile_in", "off_miss", "beyond_clamp",
    "rect_lo_exact", "rect_hi_exact", "rect_hi_touch",
    "clone_a0", "clone_a1", "clone_a2", "pair_front", "pair_opaque", "pair_back",
)
ALPHA_MIN = np.float32(1.0) / np.float32(255.0)      # the blend's `alpha < 1.0f / 255.0f`
_HOSTILE = {}


def _focal(scene):
    return scene["cfg"]["W"] / (2.0 * scene["cam"]["tanfovx"])


def _mean_at(scene, px, py, z):
    """The camera-space (= world-space: identity pose) position that projects to pixel (px, py) at depth z, in float32."""
    W, H, f = scene["cfg"]["W"], scene["cfg"]["H"], _focal(scene)
    return np.array([(px - (W - 1) / 2.0) / f * z, (py - (H - 1) / 2.0) / f * z, z], np.float32)


def exact_means(oracle, scene, targets, reach=64):
    """For every (px, py, z) of `targets`, inside the frame: a float32 position whose projected mean in the ORACLE's arithmetic
    is (px, py) bit for bit.  The floats within `reach` steps of the analytic x and y are all projected once.  (Not every
    target can be hit: where ndc's ulp, times half the image size, is coarser than the pixel coordinate's, no float may
    land on it -- at W = 48 every centre from 12 to 35 can; at H = 32 the ndc of a centre is dyadic and every one can.)"""
    ks = np.arange(-reach, reach + 1)
    rows = []
    for px, py, z in targets:
        m = _mean_at(scene, px, py, z)
        c = np.repeat(m[None], ks.size, 0)
        c[:, 0] = m[0] + ks * np.spacing(m[0])
        c[:, 1] = m[1] + ks * np.spacing(m[1])
        rows.append(c)
    cand = np.concatenate(rows).astype(np.float32)
    probe = small_scene(P=cand.shape[0], W=scene["cfg"]["W"], H=scene["cfg"]["H"], w2c=None, scale_lo=0.02, scale_hi=0.03)
    probe["gaussians"]["means3D"] = cand
    f, _ = run_oracle(oracle, dict(probe, cam=scene["cam"]), backward=False)
    assert (f.radii > 0).all()
    m2 = f.geom["means2D"].reshape(len(targets), ks.size, 2)
    out = []
    for t, (px, py, z) in enumerate(targets):
        ix, iy = np.flatnonzero(m2[t, :, 0] == np.float32(px)), np.flatnonzero(m2[t, :, 1] == np.float32(py))
        assert ix.size and iy.size, "no float projects to (%s, %s) at depth %s" % (px, py, z)
        c = cand.reshape(len(targets), ks.size, 3)[t]
        out.append(np.array([c[ix[ix.size // 2], 0], c[iy[iy.size // 2], 1], c[0, 2]], np.float32))
    return out


def ewa_radius(scene, i):
    """float64 restatement of forward.cu's projected mean and 3 sigma radius of row i (scales and rotations; the oracle writes
    neither for a Gaussian whose tile rectangle is empty).  Returns (px, py, radius)."""
    cam, cfg, g = scene["cam"], scene["cfg"], scene["gaussians"]
    V = cam["viewmatrix"].astype(np.float64).reshape(4, 4)
    t = np.append(g["means3D"][i].astype(np.float64), 1.0) @ V
    hom = np.append(g["means3D"][i].astype(np.float64), 1.0) @ cam["projmatrix"].astype(np.float64).reshape(4, 4)
    ndc = hom[:2] / (hom[3] + 1e-7)
    px, py = ((ndc[0] + 1) * cfg["W"] - 1) * 0.5, ((ndc[1] + 1) * cfg["H"] - 1) * 0.5
    r, x, y, z = g["rotations"][i].astype(np.float64)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                  [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                  [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])
    Sigma = R @ np.diag(g["scales"][i].astype(np.float64) ** 2) @ R.T
    fx, fy = cfg["W"] / (2.0 * cam["tanfovx"]), cfg["H"] / (2.0 * cam["tanfovy"])
    tx = np.clip(t[0] / t[2], -1.3 * cam["tanfovx"], 1.3 * cam["tanfovx"]) * t[2]
    ty = np.clip(t[1] / t[2], -1.3 * cam["tanfovy"], 1.3 * cam["tanfovy"]) * t[2]
    J = np.array([[fx / t[2], 0, -fx * tx / t[2] ** 2], [0, fy / t[2], -fy * ty / t[2] ** 2]])
    A = J @ V[:3, :3].T
    c = A @ Sigma @ A.T
    a, b, d = c[0, 0] + 0.3, c[0, 1], c[1, 1] + 0.3
    mid, det = 0.5 * (a + d), a * d - b * b
    return px, py, float(np.ceil(3.0 * np.sqrt(mid + np.sqrt(max(0.1, mid * mid - det)))))


def giant_row(scene, i, px, py):
    """Row i becomes a Gaussian of scale 20 .. 30 at depth 5: a 3 sigma radius of hundreds of pixels (below 1e5: the
    oracle's and the device's float -> int conversions agree), faint, behind most of the scene."""
    g = scene["gaussians"]
    c2w = np.linalg.inv(scene["cam"]["w2c"].astype(np.float64))
    g["means3D"][i] = (np.append(_mean_at(scene, px, py, 5.0).astype(np.float64), 1.0) @ c2w.T)[:3].astype(np.float32)
    g["scales"][i] = np.array([30.0, 20.0, 25.0], np.float32)
    g["opacities"][i] = 0.05


def hostile_scene(oracle):
    """(scene, rows): 160 Gaussians on 48 x 32, identity pose, the centred camera, small_scene's upstream gradients, with the
    rows of HOSTILE_ROWS overwritten; rows[name] is the row's index.  Every input is finite.  What each name claims is
    asserted against the oracle in tests/test_hostile_rows.py::test_hostile_scene_conditions.  Computed once; nobody writes
    to it."""
    if "scene" in _HOSTILE:
        return _HOSTILE["scene"]
    sc = small_scene(P=HOSTILE_P, W=HOSTILE_W, H=HOSTILE_H, w2c=None, seed=11, scale_lo=0.01, scale_hi=0.12)
    g = sc["gaussians"]
    rows = {n: 2 + 5 * k for k, n in enumerate(HOSTILE_ROWS)}
    f = _focal(sc)
    iso = lambda sigma_px, z: np.full(3, sigma_px * z / f, np.float32)      # an isotropic scale of sigma_px pixels on the axis

    def put(name, px, py, z, scales=None, opacity=None):
        i = rows[name]
        g["means3D"][i] = _mean_at(sc, px, py, z)
        if scales is not None:
            g["scales"][i] = np.asarray(scales, np.float32)
        if opacity is not None:
            g["opacities"][i] = opacity
        return i

    # scales
    put("zero3", 8, 6, 2.0, (0, 0, 0), 0.7)
    put("zero1", 20, 25, 2.5, (0.06, 0.0, 0.09), 0.6)
    put("needle", 34, 8, 2.0, (0.3, 3e-5, 3e-5), 0.5)
    put("pancake", 12, 20, 3.0, (0.15, 0.15, 5e-7), 0.5)
    giant_row(sc, rows["giant"], 30, 20)
    # rotations
    put("q_small", 40, 25, 2.75, None, 0.5)
    g["rotations"][rows["q_small"]] *= np.float32(0.1)
    put("q_large", 6, 14, 3.5, (0.002, 0.003, 0.004), 0.5)
    g["rotations"][rows["q_large"]] *= np.float32(10.0)
    put("q_zero", 28, 4, 2.25, None, 0.5)
    g["rotations"][rows["q_zero"]] = 0.0
    i = put("q_negw", 18, 12, 3.75, None, 0.5)
    if g["rotations"][i][0] > 0:
        g["rotations"][i] = -g["rotations"][i]
    # opacities: raw values, as a caller hands over who passes _opacity instead of the activated tensor
    put("op_zero", 44, 12, 1.75, iso(2.0, 1.75), 0.0)
    put("op_one", 3, 22, 4.0, iso(2.0, 4.0), 1.0)
    put("op_above_one", 36, 28, 4.5, iso(2.5, 4.5), 1.5)
    put("op_negative", 22, 3, 1.25, iso(2.0, 1.25), -0.2)
    inf = np.float32(np.inf)
    # means: the exact ones are filled in below
    g["means3D"][rows["behind"]] = np.array([0.1, -0.2, -2.0], np.float32)
    g["means3D"][rows["at_camera"]] = 0.0
    put("off_one_tile_in", -10, 12, 2.0, iso(4.5, 2.0), 0.5)
    put("off_miss", -8.5, 16, 2.0, iso(2.24, 2.0), 0.5)
    put("beyond_clamp", 23.5 + 1.9 * 24, 16, 2.0, iso(9.0, 2.0), 0.5)
    exact = dict(
        # the only pixel that can blend them: sigma 0.17 px, alpha at a neighbouring centre 0.2 of the one at the mean; in
        # front of everything else (z 0.5 against 1 and more)
        thr_below=(14, 27, 0.5, iso(0.17, 0.5), np.nextafter(ALPHA_MIN, -inf)),
        thr_above=(33, 3, 0.5, iso(0.17, 0.5), np.nextafter(ALPHA_MIN, inf)),
        thr_exact=(24, 30, 0.5, iso(0.17, 0.5), ALPHA_MIN),       # alpha == 1/255 is blended: the test is `<`
        pixel_centre=(30, 10, 1.5, iso(1.5, 1.5), 0.5),
        tile_corner=(15.5, 15.5, 2.0, iso(1.5, 2.0), 0.5),
        # radius 5 (3 sqrt(1.38^2 + 0.3 + sqrt(0.1)) = 4.8): (21 - 5) / 16 = 1, (12 + 5 + 15) / 16 = 2, and a rectangle that
        # ends on pixel 16 in x and y, the first of the next tile: (11 + 5 + 15) / 16 = 1.94
        rect_lo_exact=(21, 9, 2.0, iso(1.38, 2.0), 0.5),
        rect_hi_exact=(12, 22, 2.0, iso(1.38, 2.0), 0.5),
        rect_hi_touch=(12, 12, 2.0, iso(0.86, 2.0), 0.5),
        # clones: bit-identical rows
        clone_a0=(38, 22, 3.25, None, 0.4),
        pair_front=(26, 14, 2.2, iso(1.2, 2.2), 0.5),
    )
    means = exact_means(oracle, sc, [v[:3] for v in exact.values()])
    for (name, v), m in zip(exact.items(), means):
        put(name, v[0], v[1], v[2], v[3], v[4])
        g["means3D"][rows[name]] = m
    for name in ("clone_a1", "clone_a2"):
        for k in g:
            g[k][rows[name]] = g[k][rows["clone_a0"]]
    for k in g:
        g[k][rows["pair_back"]] = g[k][rows["pair_front"]]
    # ... and between the pair, by id, at the same depth: an opaque row.  Equal keys keep their id order, so the first of the
    # pair is blended in front of it and the second behind it (T 0.01 .. 1 of what the first saw)
    i = rows["pair_opaque"]
    g["means3D"][i] = g["means3D"][rows["pair_front"]]
    g["scales"][i] = iso(2.0, 2.2)
    g["opacities"][i] = 1.0
    assert all(np.isfinite(v).all() for v in g.values())
    _HOSTILE["scene"] = (sc, rows)
    return _HOSTILE["scene"]


def hostile_inputs(oracle, variant):
    """The argument patterns of the hostile scene: None (scales and rotations, SH colours), "cov3D_precomp" (the hostile
    scales and rotations as 3-D covariances, in float32 by the oracle's own formula: the zero-scale row's is singular, a culled
    row's all zeros) or "colors_precomp" (values below 0 and above 1)."""
    if variant is None:
        return None
    sc, _ = hostile_scene(oracle)
    if variant == "cov3D_precomp":
        return dict(scales=None, rotations=None, cov3D_precomp=run_oracle(oracle, sc, backward=False)[0].geom["cov3D"].copy())
    assert variant == "colors_precomp"
    return dict(shs=None, colors_precomp=np.random.default_rng(5).uniform(-1.0, 2.0, (HOSTILE_P, 3)).astype(np.float32))


def hostile_reference(oracle, variant=None):
    """hostile_scene under hostile_inputs(variant), with the oracle's forward and the float64 gradients under every upstream
    plane together: (scene, rows, f, ref, inputs).  Computed once per variant."""
    sc, rows = hostile_scene(oracle)
    inputs = hostile_inputs(oracle, variant)
    if ("f", variant) not in _HOSTILE:
        _HOSTILE[("f", variant)] = run_oracle(oracle, sc, backward=False, inputs=inputs)[0]
    f = _HOSTILE[("f", variant)]
    return sc, rows, f, float64_case_grads(("hostile", variant), sc, f, ("all",), inputs=inputs)["all"], inputs


def frame_scene(W, H):
    """The scene of the extreme frame shapes: 200 Gaussians under small_scene's tilted pose, row 0 replaced by the giant."""
    sc = small_scene(P=200, W=W, H=H, scale_lo=0.02, scale_hi=0.2)
    giant_row(sc, 0, (W - 1) / 2.0, (H - 1) / 2.0)
    return sc


ROW_TENSORS = ("means3D", "means2D", "opacities", "scales", "rotations", "shs", "shs_p")
ROW_FLOOR = 1e-6


def row_errors(ref, got, rows):
    """The row-by-row measure of the hostile scene: {(name, tensor): (error, own, yardstick)} with, for every named row, its
    max-norm error, its own max-norm in `ref`, and the yardstick max(own, ROW_FLOOR * the whole tensor's max-norm); under the
    name "ordinary" all other rows as one block.  ref, got: gradients under run_gpu's names (means2D: its first two columns).
    The floor: a row may have no gradient of its own in a tensor -- thr_above is blended by the one pixel it is centred on,
    where dL/dmean2D, dL/dscales and dL/drotations are proportional to the offset from the pixel, an exact zero in fp32 and
    the rounding of the projection (1e-7 px) in float64 -- and a ratio of two roundings says nothing; 1e-6 of the tensor's
    size is ten fp32 roundings of it, far below anything that a whole-tensor bound of 3e-4 sees."""
    out = {}
    for k in ROW_TENSORS + ("colors_precomp", "cov3D_precomp"):
        if ref.get(k) is None or got.get(k) is None:
            continue
        r = np.asarray(ref[k], np.float64)
        r = r.reshape(r.shape[0], -1)
        q = np.asarray(got[k], np.float64).reshape(r.shape[0], -1)
        if k == "means2D":
            r, q = r[:, :2], q[:, :2]
        floor = ROW_FLOOR * float(np.abs(r).max())
        named = np.zeros(r.shape[0], bool)
        for name, i in rows.items():
            named[i] = True
            own = float(np.abs(r[i]).max())
            out[(name, k)] = (float(np.abs(q[i] - r[i]).max()), own, max(own, floor) if own else 0.0)
        own = float(np.abs(r[~named]).max())
        out[("ordinary", k)] = (float(np.abs(q[~named] - r[~named]).max()), own, own)
    return out


# Frames whose tile grid takes tile-pull binning's other paths (tests/pull_ref.py: supertiles of 4 x 4 .. 16 x 16 tiles, depth
# slabs, the staged scatter): frame_scene's 200 rows -- the giant reaches every tile, so every supertile has an entry, the last
# partial one included -- and a dense cluster on the image centre, which at 1025 x 1025 is the corner shared by four 4 x 4
# supertiles.  Under the planes 0.45 / 6.05 a depth bin is 2^13 float steps and a slab of 1024 bins one octave of depth: the
# cluster's z range chooses the slabs.  name -> (W, H, cluster); cluster: small_scene's P, spread, z_lo, z_hi.
# What each scene reaches is asserted on the oracle in tests/test_pull_ref.py.
BIG_GRIDS = {
    "all": (1025, 1025, dict(P=20000, spread=0.05, z_lo=0.46, z_hi=5.5)),
    "near": (1025, 1025, dict(P=12000, spread=0.06, z_lo=0.46, z_hi=1.6)),
    "mid": (1025, 1025, dict(P=12000, spread=0.06, z_lo=2.0, z_hi=3.4)),
    "far": (1025, 1025, dict(P=12000, spread=0.06, z_lo=3.7, z_hi=5.5)),
    "row": (32784, 16, dict(P=20000, spread=0.004, z_lo=0.46, z_hi=5.5)),
    "col": (16, 32784, dict(P=20000, spread=0.004, z_lo=0.46, z_hi=5.5)),
    "s8": (65552, 16, dict(P=20000, spread=0.002, z_lo=0.46, z_hi=5.5)),
    "s16": (131088, 16, dict(P=20000, spread=0.001, z_lo=0.46, z_hi=5.5)),
    # (P = 20000 as in "all" puts one pixel of one Gaussian on the blend's alpha threshold: the device blends it, the oracle does
    # not, in both binning modes, and dL/dscales is off by 3.5e-4 of its max-norm -- no yardstick for a bound of 3e-4)
    "edge": (1024, 1024, dict(P=18000, spread=0.05, z_lo=0.46, z_hi=5.5)),
    "fallback": (262160, 16, dict(P=5000, spread=0.001, z_lo=0.46, z_hi=5.5)),
}
BIG_GRID_LOW_OPACITY = ("all", "row")       # also drawn with every opacity 0.05: nothing saturates, every tile with a tail flags
_BIG_GRID = {}


def big_grid_scene(W, H, cluster, opacity=None):
    """frame_scene(W, H) and a cluster small_scene(scale_lo=0.004, scale_hi=0.03, **cluster), rows concatenated, one camera.
    opacity: every row's opacity."""
    sc = frame_scene(W, H)
    cl = small_scene(W=W, H=H, seed=23, scale_lo=0.004, scale_hi=0.03, **cluster)
    assert all(np.array_equal(sc["cam"][k], cl["cam"][k]) for k in ("viewmatrix", "projmatrix"))
    g = {k: np.concatenate([v, cl["gaussians"][k]]) for k, v in sc["gaussians"].items()}
    if opacity is not None:
        g["opacities"] = np.full_like(g["opacities"], opacity)
    return dict(sc, cfg=dict(sc["cfg"], P=g["means3D"].shape[0]), gaussians=g)


def big_grid(name):
    """The scene of BIG_GRIDS[name], or of "name@opacity".  Built once; nobody writes to it."""
    if name not in _BIG_GRID:
        base, _, op = name.partition("@")
        W, H, cluster = BIG_GRIDS[base]
        _BIG_GRID[name] = big_grid_scene(W, H, cluster, opacity=float(op) if op else None)
    return _BIG_GRID[name]


def big_grid_reference(oracle, name, backward=False):
    """(scene, the oracle's forward, its backward or None) of big_grid(name).  Computed once; nobody writes to it."""
    sc = big_grid(name)
    if ("f", name) not in _BIG_GRID:
        _BIG_GRID[("f", name)] = run_oracle(oracle, sc, backward=False)[0]
    f = _BIG_GRID[("f", name)]
    if backward and ("b", name) not in _BIG_GRID:
        gr = sc["grads"]
        _BIG_GRID[("b", name)] = oracle.backward(f, gr["color"], gr["phasor"], gr["depth"], gr["acc"], gr["depth_distortion"])
    return sc, f, _BIG_GRID.get(("b", name))
