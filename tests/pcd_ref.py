"""A numpy restatement of what the reference's ToF point-cloud code computes, written in its own terms from that code's
behaviour (cv2 and plyfile are not importable here, so ``scene/dataset_readers.py`` is not): the unprojection that
``scene/dataset_readers.py`` performs in three places (:537-574 ToRF phase initialisation, :905-962 F-ToRF, :1067-1118 proxy
clouds), the file ``storePly`` (:127-150) writes through plyfile, what ``fetchPly`` (:110-125) reads, and the tensors of
``GaussianModel.create_from_pcd`` (``scene/gaussian_model.py:180-236``).  tests/golden/pcd.npz and points3d_small.ply are
recorded from these functions (tests/golden/make_golden_pcd.py), not from a run of the reference.

The reference works on a 4-column array with in-place ufuncs and Python scalars; here every quantity is a vector of its own
and every scalar is typed, chosen so that each operation has the dtype and the rounding numpy gives the reference's: a Python
float beside a float32 array acts as a float32, ``np.square`` of a float32 distance stays float32, int16 pixel coordinates
times 2.0 are float64.

Three places say more than the reference's text does:
  * It inverts the float32 view matrix in float32 (LAPACK); here, as in the kernel, the same 16 values are inverted in float64
    (``inverse_view``).
  * The F-ToRF amplitude test (:940) compares a float32 scalar with the Python float 0.04: in float64 under the reference's
    numpy 1.x, in float32 under numpy 2.  ``amplitude_is_low`` spells the reference's out.
  * The candidate test (:933) compares a one-element float32 array with the Python floats znear and 10.5: in float32 under
    either numpy, so ``unwrap_ftorf`` compares with ``float32(znear)``.
"""
import math

import numpy as np

C0 = 0.28209479177387814                # utils/sh_utils.py:26


def to_sh(v):
    """RGB2SH and PA2SH (utils/sh_utils.py:114-121) in v's own precision"""
    t = v.dtype.type
    return (v - t(0.5)) / t(C0)


def from_sh(sh):
    """SH2RGB and SH2PA (:117-124) in sh's own precision"""
    t = sh.dtype.type
    return sh * t(C0) + t(0.5)


def depth_from_tof(tof, depth_range, phase_offset=0.0):
    """The distance of scene/torf_utils.py:53-57 for phasors [..., 3], as [..., 1] in the phasors' precision: the phase behind
    the offset, wrapped into [0, 2 pi), as a fraction of 4 pi of the depth range"""
    t = tof.dtype.type
    shifted = np.arctan2(tof[..., 1:2], tof[..., 0:1]) - t(phase_offset)
    wrapped = np.where(shifted < 0, shifted + t(2 * np.pi), shifted)
    return wrapped * t(depth_range) / t(4 * np.pi)


def depth_from_tof64(tof, depth_range, phase_offset=0.0):
    """the same expression with every value taken to float64 first: what a float32 result is measured against"""
    return depth_from_tof(tof.astype(np.float64), float(np.float32(depth_range)), float(np.float32(phase_offset)))


def inverse_view(view_mat):
    return np.linalg.inv(np.asarray(view_mat, dtype=np.float64))


def amplitude_is_low(a):
    return np.asarray(a, dtype=np.float64) < 0.04


def screen(H, W, stride):
    """The grid of :539-544: image coordinates (xs, ys) of the H' x W' grid pixels in row-major order, int16 as the reference
    keeps them, and (H', W')"""
    Hp, Wp = math.ceil(H / stride), math.ceil(W / stride)
    r, c = np.divmod(np.arange(Hp * Wp), Wp)
    return (c * stride).astype(np.int16), (r * stride).astype(np.int16), Hp, Wp


def unwrap_ftorf(z, depth_range, znear, tof_image, Hp, Wp):
    """The rule of :929-946 for float32 distances z [n]: of z and z + depth_range / 2 those in (znear, 10.5] are candidates; one
    candidate is taken, and between two the amplitude decides, read at the reference's own index (i // W', i % H') of the
    unstrided image.  IndexError where the reference raises one: no candidate, or that index outside the image."""
    t = z.dtype.type
    far = z + t(depth_range / 2.0)
    ok_near = (t(znear) < z) & (z <= t(10.5))
    ok_far = (t(znear) < far) & (far <= t(10.5))
    if not (ok_near | ok_far).all():
        raise IndexError("%d pixel(s) with no candidate" % int((~(ok_near | ok_far)).sum()))
    i = np.arange(z.shape[0])
    both, h_, w_ = ok_near & ok_far, i // Wp, i % Hp
    if (w_[both] >= tof_image.shape[1]).any():
        raise IndexError("%d amplitude index(es) outside the image" % int((w_[both] >= tof_image.shape[1]).sum()))
    low = np.zeros(z.shape[0], dtype=bool)
    low[both] = amplitude_is_low(tof_image[h_[both], w_[both], 2])
    return np.where(both, np.where(low, far, z), np.where(ok_near, z, far))


def unproject(tof_image, stride, znear, fov_x, fov_y, view_mat, depth_range, phase_offset, mode, rendered=None, dist=None):
    """One frame's points.  ``dist`` [rows] replaces the distances computed here, so that a caller can feed another
    implementation's.  Returns xyz (float64, before the file's f4 rounding), dist and the mode's amplitude-derived values."""
    H, W = tof_image.shape[:2]
    xs, ys, Hp, Wp = screen(H, W, stride)
    # the pixel on the near plane (:552-555), float64: int16 * 2.0 / size - 1.0, scaled by half the plane's extent in metres
    near_x = (xs * 2.0 / W - 1.0) * (znear * np.tan(fov_x / 2.0) * 2.0) / 2.0
    near_y = (ys * 2.0 / H - 1.0) * (znear * np.tan(fov_y / 2.0) * 2.0) / 2.0
    ray = np.sqrt(near_x * near_x + near_y * near_y + znear * znear)
    dir_x, dir_y = near_x / ray, near_y / ray
    z = depth_from_tof(tof_image[ys, xs, :], depth_range, phase_offset)[:, 0]
    if mode == "torf_init":
        # :545 lists the grid twice, and :559, which should shift the second half, adds to an empty slice: two equal halves
        z, dir_x, dir_y = np.tile(z, 2), np.tile(dir_x, 2), np.tile(dir_y, 2)
    elif mode == "ftorf_init":
        z = unwrap_ftorf(z, depth_range, znear, tof_image, Hp, Wp)
    else:
        z = np.concatenate([z, rendered[ys, xs]])               # :1092-1096: a float64 image makes the whole column float64
        dir_x, dir_y = np.tile(dir_x, 2), np.tile(dir_y, 2)
    if dist is not None:
        assert dist.shape == z.shape and dist.dtype == z.dtype, (dist.shape, dist.dtype, z.shape, z.dtype)
        z = dist
    cam_x, cam_y = dir_x * z, dir_y * z                         # float64 products with the distance (:565-566)
    z_sq = z * z                                                # in the distance's own precision, as np.square's (:567)
    cam_z = np.sqrt(z_sq - cam_x * cam_x - cam_y * cam_y)
    c2w = inverse_view(view_mat)
    out = {"xyz": np.stack([c2w[k, 0] * cam_x + c2w[k, 1] * cam_y + c2w[k, 2] * cam_z + c2w[k, 3] for k in range(3)], axis=1), "dist": z}
    if mode != "proxy":
        amp = tof_image[ys, xs, 2]
        amp = np.tile(amp, 2) if mode == "torf_init" else amp
        sh_color, sh_amp = to_sh(amp), to_sh(amp * z_sq)        # :572-573, float32
        out.update(amp=amp, sh_color=sh_color, color=np.repeat(from_sh(sh_color)[:, None], 3, axis=1), sh_amp=sh_amp,
                   amplitude=from_sh(sh_amp))
    return out


def zero_phasor(num):
    """:584-585: SH2PA(PA2SH(0)) in float32, [num, 1]"""
    return from_sh(to_sh(np.zeros((num, 1), dtype=np.float32)))


# ---- storePly / fetchPly ----------------------------------------------------------------------------------------------------

_PLY_TYPE = {"f4": "float", "u1": "uchar"}


def store_dtype(has_phasor, has_seg):
    dtype = [(n, "f4") for n in ("x", "y", "z", "nx", "ny", "nz")] + [(n, "u1") for n in ("red", "green", "blue")]
    if has_phasor:
        dtype += [("phase", "f4"), ("amplitude", "f4")]
    if has_seg:
        dtype += [(n, "u1") for n in ("seg_red", "seg_green", "seg_blue")]
    return dtype


def to_u1(column):
    """What numpy's assignment of a Python float to a uint8 field does (recorded with numpy 2.2; tests/test_pcd.py holds this
    function to numpy's own assignment): int(v), which truncates towards zero and raises ValueError for a NaN and OverflowError
    for an infinity, then OverflowError unless the integer is in [0, 255]"""
    column = np.asarray(column, dtype=np.float64)
    if np.isnan(column).any():
        raise ValueError("cannot convert float NaN to integer")
    whole = np.trunc(column)
    if ((whole < 0) | (whole > 255)).any():
        raise OverflowError("Python integer out of bounds for uint8")
    return whole.astype(np.uint8)


def store_bytes(xyz, colors, phases=None, amplitudes=None, seg_colors=None):
    """The file storePly writes, filled column by column: float64 positions rounded to f4, zero normals, the colour columns by
    ``to_u1``, the phasor columns only when both are given; behind the header plyfile emits for that dtype list"""
    has_phasor = phases is not None and amplitudes is not None
    dtype = store_dtype(has_phasor, seg_colors is not None)
    rows = np.zeros(xyz.shape[0], dtype=dtype)
    for k, name in enumerate(("x", "y", "z")):
        rows[name] = xyz[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        rows[name] = to_u1(colors[:, k])
    if has_phasor:
        rows["phase"], rows["amplitude"] = phases[:, 0], amplitudes[:, 0]
    if seg_colors is not None:
        for k, name in enumerate(("seg_red", "seg_green", "seg_blue")):
            rows[name] = to_u1(seg_colors[:, k])
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(rows)]
    lines += ["property %s %s" % (_PLY_TYPE[t], n) for n, t in dtype] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii") + rows.tobytes()


def fetch_bytes(data):
    """What fetchPly reads from a file's bytes, as a dict with BasicPointCloud's fields: float32 positions, normals and phasor
    columns ([P, 1]); the colours u1 / 255.0 in float64; the phasor columns only when both are there, the seg colours only all
    three"""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    words = [line.split() for line in data[:end].decode("ascii").split("\n")]
    count = next(int(w[2]) for w in words if w[:2] == ["element", "vertex"])
    fields = np.dtype([(w[2], {"float": "<f4", "uchar": "u1"}[w[1]]) for w in words if w[:1] == ["property"]])
    v = np.frombuffer(data, dtype=fields, count=count, offset=end)
    cols = lambda *names: np.stack([v[n] for n in names], axis=1)
    has = lambda *names: all(n in fields.names for n in names)
    return {"points": cols("x", "y", "z"), "normals": cols("nx", "ny", "nz"), "colors": cols("red", "green", "blue") / 255.0,
            "phases": cols("phase") if has("phase", "amplitude") else None,
            "amplitudes": cols("amplitude") if has("phase", "amplitude") else None,
            "seg_colors": cols("seg_red", "seg_green", "seg_blue") / 255.0 if has("seg_red", "seg_green", "seg_blue") else None}


# ---- inputs the tests and the fixture share -----------------------------------------------------------------------------------

DEPTH_RANGE, PHASE_OFFSET, ZNEAR = 7.5, 0.3, 0.45
# margins of the generated frames: the phase (after the offset) stays this far from the wrap at 0 and 2 pi; the amplitudes this
# far from 0.04; F-ToRF candidates this far from znear and 10.5
PHASE_MARGIN, AMP_MARGIN, DIST_MARGIN = 0.05, 0.005, 0.02


def make_frame(H, W, seed, depth_range=DEPTH_RANGE, phase_offset=PHASE_OFFSET, low_amp=0.5, dist_lo=1.0, dist_hi=3.2, dist=None):
    """A [H, W, 3] float32 ToF frame whose distances lie in [dist_lo, dist_hi] (so that, with depth_range 7.5, both F-ToRF
    candidates z and z + 3.75 lie in (znear, 10.5] by more than DIST_MARGIN) and whose amplitudes are below 0.04 - AMP_MARGIN for
    a fraction `low_amp` of the pixels and above 0.04 + AMP_MARGIN for the rest"""
    rng = np.random.default_rng(seed)
    drawn = rng.uniform(dist_lo, dist_hi, (H, W))
    dist = drawn if dist is None else dist
    phase = dist * 4 * np.pi / depth_range + phase_offset
    assert phase.min() - phase_offset > PHASE_MARGIN and phase.max() - phase_offset < 2 * np.pi - PHASE_MARGIN
    low = rng.random((H, W)) < low_amp
    amp = np.where(low, rng.uniform(0.005, 0.04 - AMP_MARGIN, (H, W)), rng.uniform(0.04 + AMP_MARGIN, 0.95, (H, W)))
    scale = rng.uniform(0.2, 2.0, (H, W))
    return np.stack([np.cos(phase) * scale, np.sin(phase) * scale, amp], axis=-1).astype(np.float32)


def make_cloud(P, seed):
    """storePly's arguments for P points: float64 positions, float32 colours and float64 seg colours times 255, float32 phasor
    columns; colour values cover 0, 255, fractions just below an integer and -0.5"""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(0.0, 2.0, (P, 3))
    colors = (rng.random((P, 3)).astype(np.float32) * np.float32(255.0))
    seg = rng.random((P, 3)) * 255.0
    edge = np.array([0.0, 255.0, 254.99999, 255.99, -0.5, 0.999999, 1.0, 128.5])
    colors.reshape(-1)[:min(len(edge), 3 * P)] = edge[:3 * P].astype(np.float32)
    seg.reshape(-1)[::-1][:min(len(edge), 3 * P)] = edge[:3 * P]
    phases = rng.random((P, 1)).astype(np.float32)
    amplitudes = (rng.random((P, 1)) * 3.0).astype(np.float32)
    return xyz, colors, phases, amplitudes, seg


def camera(W, H):
    """an off-centre, anisotropic sensor camera of helpers.CAMERAS behind a tilted, shifted pose, as the reader code sees it:
    getWorld2View2's float32 matrix, znear and the two fields of view"""
    import helpers
    from gftorf_amd import synth
    cam = helpers.sensor_camera("anisotropic", W, H, w2c=synth.look_at_w2c(0.15, -0.1, 0.05, (0.1, -0.05, 0.2)))
    return dict(view=np.float32(cam["w2c"]), znear=cam["znear"], fov_x=2 * math.atan(cam["tanfovx"]), fov_y=2 * math.atan(cam["tanfovy"]))


# ---- create_from_pcd ----------------------------------------------------------------------------------------------------------

def eager_create(cloud, max_sh_degree, isotropic, init_static_first, initial_opacity):
    """The tensors scene/gaussian_model.py:184-236 leaves on the model, formed with eager torch on the cloud's device from the
    same elementwise operations (``.float()``, ``(v - 0.5) / C0``, ``clamp_min``, ``sqrt``, ``log``, ``log(x / (1 - x))``), so that
    their bits are the reference's; the layout is written directly instead of through the reference's [P, c, (D + 1)^2] scratch
    tensors.  distCUDA2 is this package's."""
    import torch
    from gftorf_amd import distCUDA2
    dev, xyz = cloud.points.device, cloud.points.float()
    P, n = xyz.shape[0], (max_sh_degree + 1) ** 2 - 1
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    sh = lambda v: (v.float() - 0.5) / C0
    parts = (xyz[:P // 2], xyz[P // 2:]) if init_static_first else (xyz,)               # :193-199: the halves apart, or all at once
    dist2 = torch.cat([torch.clamp_min(distCUDA2(part.contiguous()), 0.0000001) for part in parts])
    scales = torch.log(torch.sqrt(dist2)).reshape(P, 1)
    rotation = zeros(P, 4)
    rotation[:, 0] = 1
    x = initial_opacity * torch.ones((P, 1), dtype=torch.float, device=dev)
    out = {"_xyz": xyz, "_features_dc_color": sh(cloud.colors).reshape(P, 1, 3), "_features_rest_color": zeros(P, n, 3),
           "_scaling": scales if isotropic else scales.repeat(1, 3), "_rotation": rotation, "_opacity": torch.log(x / (1 - x)),
           "max_radii2D": zeros(P)}
    # the coefficients beside the DC one are zeros for the phase too: the reference's `[:, 1:, 1:] = 1.0` selects nothing of a
    # one-channel tensor (:222)
    for key, column in (("phase", cloud.phases), ("amp", cloud.amplitudes)):
        if column is not None:
            out["_features_dc_" + key], out["_features_rest_" + key] = sh(column).reshape(P, 1, 1), zeros(P, n, 1)
    if cloud.seg_colors is not None:
        out["_features_seg_color"] = cloud.seg_colors.float().contiguous()
    return out
