"""Dense float64 PyTorch re-derivation of the ToF Gaussian rasterizer (test helper).

Independent of both the oracle (C) and the HIP kernels: the forward equations of
SURVEY.md Appendix A.2/A.3 written with differentiable torch ops in float64;
gradients come from autograd, not from the reference's hand-written backward.
Used to check that the oracle's backward (a restatement of
RAST/cuda_rasterizer/backward.cu) is the gradient of its forward.

Deliberate gradient conventions of the reference that autograd must mimic:
  * alpha = min(0.99, o*G): the clamp is ignored by the backward
    (backward.cu:752,869) -> straight-through.
  * t.x = clamp(t.x/t.z)*t.z: d/dt.x is gated by x_grad_mul, d/dt.z of the
    clamped value is dropped (backward.cu:293-297,383-385).
  * phase DC removal "- C0*sh_p[0].x" (forward.cu:115) is not differentiated
    (backward.cu:168-169).
  * with phasors_precomp the backward has no phasor chain at all: it stands inside "if (shs_p != nullptr)"
    (backward.cu:527-587), so the distance in the phase and in 1/dist^2 and the DC offset get no gradient there (the
    precomputed phasors themselves get none either: rasterize_points.cu returns no dL_dphasors).
Discrete decisions (culling, radii, tile lists, skips, termination) are taken
from the oracle's forward so both sides blend the same lists.
"""
import math

import numpy as np
import torch

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005,
      -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658,
      0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435]


def sh_poly(deg, sh, dirs):
    """sh [P,M,C], dirs [P,3] -> [P,C] (kernel layout [coeff][channel])."""
    x, y, z = dirs[:, 0:1], dirs[:, 1:2], dirs[:, 2:3]
    res = C0 * sh[:, 0]
    if deg > 0:
        res = res - C1 * y * sh[:, 1] + C1 * z * sh[:, 2] - C1 * x * sh[:, 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        res = (res + C2[0] * xy * sh[:, 4] + C2[1] * yz * sh[:, 5]
               + C2[2] * (2 * zz - xx - yy) * sh[:, 6] + C2[3] * xz * sh[:, 7]
               + C2[4] * (xx - yy) * sh[:, 8])
    if deg > 2:
        res = (res + C3[0] * y * (3 * xx - yy) * sh[:, 9] + C3[1] * xy * z * sh[:, 10]
               + C3[2] * y * (4 * zz - xx - yy) * sh[:, 11]
               + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12]
               + C3[4] * x * (4 * zz - xx - yy) * sh[:, 13]
               + C3[5] * z * (xx - yy) * sh[:, 14] + C3[6] * x * (xx - 3 * yy) * sh[:, 15])
    return res


def _depth_distortion_tile(ids, pix_x, pix_y, con_x, con_y, con_z, opac, d_ndc, pxf, pyf, chunk=256):
    """The depth_distortion sums of render()'s walk over one tile's list, forward only, `chunk` list entries at a time: the
    same float64 terms (transmittance as a running product, the exclusive sums A, D, D2 as running sums), so that a list
    of thousands of entries takes milliseconds.  Stops, like the walk, once every pixel has terminated."""
    n = pxf.numel()
    dt = pxf.dtype
    T = torch.ones(n, dtype=dt)
    done = torch.zeros(n, dtype=torch.bool)
    A, D1, D2, DD = (torch.zeros(n, dtype=dt) for _ in range(4))
    for c0 in range(0, ids.numel(), chunk):
        if bool(done.all()):
            break
        j = ids[c0:c0 + chunk]
        dx = pix_x[j][:, None] - pxf[None]
        dy = pix_y[j][:, None] - pyf[None]
        power = -0.5 * (con_x[j][:, None] * dx * dx + con_z[j][:, None] * dy * dy) - con_y[j][:, None] * dx * dy
        alpha = torch.clamp(opac[j][:, None] * torch.exp(power), max=0.99)
        skip = (power > 0) | (alpha < 1.0 / 255.0)
        a_eff = torch.where(skip, torch.zeros_like(alpha), alpha)
        incl = T[None] * torch.cumprod(1 - a_eff, 0)                 # test_T at every entry
        excl = torch.cat([T[None], incl[:-1]], 0)                    # T in front of it
        stop = (~skip) & (incl < 1e-4)
        stopped = torch.cumsum(stop.to(torch.int32), 0) > 0          # at or behind the entry that terminates the pixel
        act = (~skip) & (~stopped) & (~done[None])
        w = a_eff * excl * act.to(dt)
        z = d_ndc[j][:, None]
        wz, wzz = w * z, w * z * z
        A_ex = A[None] + torch.cumsum(w, 0) - w
        D1_ex = D1[None] + torch.cumsum(wz, 0) - wz
        D2_ex = D2[None] + torch.cumsum(wzz, 0) - wzz
        DD = DD + (w * (z * z * A_ex - 2 * z * D1_ex + D2_ex)).sum(0)
        A, D1, D2 = A + w.sum(0), D1 + wz.sum(0), D2 + wzz.sum(0)
        T = incl[-1]                                                  # (of no further use where the pixel has terminated)
        done = done | stopped[-1]
    return DD


# The uses of a Gaussian's position, by name (settings["detach"]): dL/dmeans3D is the sum of one term per use.
PATHS = ("mean2D", "cov_t", "dir_color", "dir_phasor", "dist_phase", "dist_factor", "dist_depth", "dist_ndc")


def render(params, fwd, settings, dd_only=False):
    """params: dict of float64 leaf tensors (means3D, opacities, shs|colors_precomp,
    shs_p|phasors_precomp, scales+rotations|cov3D_precomp, phase_offset, dc_offset).
    fwd: oracle ForwardResult (lists / masks).  settings: dict of scalars + matrices.
    Returns dict of output images (float64) + 'ndc' (retain_grad leaf-like).
    dd_only (forward only, call under torch.no_grad()): only the depth_distortion plane, by _depth_distortion_tile.
    settings["detach"] (optional, a set of names from PATHS; default empty = nothing changes): each name cuts exactly one use of
    means3D out of the graph, the forward values staying what they are -- mean2D: pix_x, pix_y; cov_t: the p_view that enters
    J and its clamp; dir_color / dir_phasor: the view direction into the colour / phasor SH; dist_phase, dist_factor,
    dist_depth, dist_ndc: the distance into the phase, into 1/dist^2, into the depth output, into d_ndc.  By the chain rule
    dL/dmeans3D minus the one computed with a name detached is that path's term.
    settings["split_uses"] (optional, default off = nothing changes): the tensor at each of these cuts becomes a node of its
    own (a view, no arithmetic: the outputs stay bit-identical, the gradients' sums may be taken in another order) and is
    returned in 'uses' (name -> list), so that dL/d(use) can be asked for and taken on to means3D, which gives every path's
    term from one backward.
    settings["margins"] (optional, a dict that is filled in): how far the walk's discrete decisions stand from their edges,
    over every (pixel, list entry) pair the walk looks at -- "alpha": min |alpha - 1/255| where power <= 0; "power": min
    |power| (the skip is power > 0); "test_T": min |test_T - 1e-4| over the pairs that are not skipped."""
    cut = frozenset(settings.get("detach", ()))
    assert cut <= set(PATHS), cut
    if params.get("phasors_precomp") is not None:
        cut = cut | {"dist_phase", "dist_factor"}      # the reference's convention (module docstring)
    split, uses = bool(settings.get("split_uses", False)), {}

    def dz(t, name):
        if name in cut:
            t = t.detach()
        elif split:
            t = t.view_as(t)
        uses.setdefault(name, []).append(t)
        return t
    dt = torch.float64
    W, H = settings["image_width"], settings["image_height"]
    V = torch.tensor(np.asarray(settings["viewmatrix"]).reshape(4, 4), dtype=dt)  # transposed storage
    PV = torch.tensor(np.asarray(settings["projmatrix"]).reshape(4, 4), dtype=dt)
    campos = torch.tensor(np.asarray(settings["campos"]).reshape(3), dtype=dt)
    tanfovx, tanfovy = settings["tanfovx"], settings["tanfovy"]
    focal_x, focal_y = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    near_n, far_n = settings["near_n"], settings["far_n"]
    D = settings["sh_degree"]
    mod = settings.get("scale_modifier", 1.0)
    dist2phase = 4.0 * math.pi / settings["depth_range"]
    vdp = settings["use_view_dependent_phase"]

    p = params["means3D"]
    P = p.shape[0]
    culled = torch.tensor(np.asarray(fwd.radii).reshape(-1) <= 0)
    if bool(culled.any()):
        # A Gaussian the oracle culled stands in no list: it contributes nothing, and its gradients are exact zeros.  Its
        # own position need not be one at which the formulas below are defined (the camera centre: a direction of length
        # zero, t.x / t.z = 0 / 0, 1 / dist^2), and 0 * NaN in the backward is NaN: the formulas are evaluated at a point
        # on the optical axis between the planes instead.  Every other row keeps its values and its graph.
        mid = torch.tensor([0.0, 0.0, 0.5 * (near_n + far_n)], dtype=dt)
        safe = torch.linalg.solve(V[:3, :3].T, mid - V[3, :3])
        p = torch.where(culled[:, None], safe[None, :], p)
    ones = torch.ones(P, 1, dtype=dt)
    ph = torch.cat([p, ones], 1)
    p_view = (ph @ V)[:, :3]           # stored-transposed: row-vector times matrix
    p_hom = ph @ PV
    p_w = 1.0 / (p_hom[:, 3:4] + 1e-7)
    ndc = p_hom[:, :2] * p_w
    if ndc.requires_grad:          # (a forward-only call under torch.no_grad() has no graph)
        ndc.retain_grad()
    pix_x = dz(((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, "mean2D")
    pix_y = dz(((ndc[:, 1] + 1.0) * H - 1.0) * 0.5, "mean2D")

    # cov3D
    if params.get("cov3D_precomp") is not None:
        c6 = params["cov3D_precomp"]
        Sigma = torch.stack([torch.stack([c6[:, 0], c6[:, 1], c6[:, 2]], -1),
                             torch.stack([c6[:, 1], c6[:, 3], c6[:, 4]], -1),
                             torch.stack([c6[:, 2], c6[:, 4], c6[:, 5]], -1)], -2)
    else:
        s = params["scales"] * mod
        q = params["rotations"]
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        Rm = torch.stack([
            torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
            torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
            torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], -2)
        Sigma = Rm @ torch.diag_embed(s * s) @ Rm.transpose(1, 2)

    # cov2D (EWA)
    pv_cov = dz(p_view, "cov_t")
    tx, ty, tz = pv_cov[:, 0], pv_cov[:, 1], pv_cov[:, 2]
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = tx / tz, ty / tz
    gx_mul = ((txtz >= -limx) & (txtz <= limx)).to(dt)
    gy_mul = ((tytz >= -limy) & (tytz <= limy)).to(dt)
    txc = torch.clamp(txtz, -limx, limx) * tz
    tyc = torch.clamp(tytz, -limy, limy) * tz
    txu = tx * gx_mul + (txc - tx * gx_mul).detach()
    tyu = ty * gy_mul + (tyc - ty * gy_mul).detach()
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([focal_x / tz, zero, -(focal_x * txu) / (tz * tz)], -1),
                     torch.stack([zero, focal_y / tz, -(focal_y * tyu) / (tz * tz)], -1)], -2)  # [P,2,3]
    Rv = V[:3, :3].T  # math W2C rotation
    A = J @ Rv
    cov2 = A @ Sigma @ A.transpose(1, 2)
    a = cov2[:, 0, 0] + 0.3
    b = cov2[:, 0, 1]
    c = cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    con_x, con_y, con_z = c / det, -b / det, a / det

    # colour
    dir_orig = p - campos
    dirs = dir_orig / dir_orig.norm(dim=1, keepdim=True)
    if params.get("shs") is not None:
        rgb = torch.clamp(sh_poly(D, params["shs"], dz(dirs, "dir_color")) + 0.5, min=0.0)
    else:
        rgb = params["colors_precomp"]

    dist = p_view.norm(dim=1)
    d_ndc = far_n / (far_n - near_n) * (1 - near_n / dz(dist, "dist_ndc"))
    dist_f = dz(dist, "dist_factor")
    factor = 1.0 / (dist_f * dist_f)
    dist_ph = dz(dist, "dist_phase")
    dist_out = dz(dist, "dist_depth")
    phase_offset, dc_offset = params["phase_offset"], params["dc_offset"]
    if params.get("phasors_precomp") is not None:
        pp = params["phasors_precomp"]
        dc_offset = dc_offset.detach()
        phase = dist_ph * dist2phase
        if vdp:
            phase = phase + pp[:, 0]
        amp = pp[:, 1]
    elif params.get("shs_p") is not None:
        sp = params["shs_p"]
        pa = sh_poly(D, sp, dz(dirs, "dir_phasor")) + 0.5
        phase_sh = pa[:, 0] - 0.5 - (C0 * sp[:, 0, 0]).detach()
        amp = torch.clamp(pa[:, 1], min=0.0)
        phase = dist_ph * dist2phase + phase_offset
        if vdp:
            phase = phase + phase_sh
    else:
        phase = None
    if phase is not None:
        cp, sn = torch.cos(phase), torch.sin(phase)
        ph7 = torch.stack([cp * amp * factor, sn * amp * factor, amp * factor,
                           (cp + dc_offset) * amp * factor, (-cp + dc_offset) * amp * factor,
                           (sn + dc_offset) * amp * factor, (-sn + dc_offset) * amp * factor], -1)
    else:
        ph7 = torch.zeros(P, 7, dtype=dt)
    opac = params["opacities"].reshape(-1)

    bg = torch.tensor(np.broadcast_to(np.asarray(settings["bg"], np.float64), (7, H, W)).copy(), dtype=dt)
    out_color = torch.zeros(3, H, W, dtype=dt)
    out_phasor = torch.zeros(7, H, W, dtype=dt)
    out_depth = torch.zeros(1, H, W, dtype=dt)
    out_acc = torch.zeros(1, H, W, dtype=dt)
    out_dd = torch.zeros(1, H, W, dtype=dt)
    colors_l, phasors_l, depth_l, acc_l, dd_l, idx_l = [], [], [], [], [], []

    gxn, gyn = (W + 15) // 16, (H + 15) // 16
    ranges = fwd.ranges
    plist = torch.tensor(fwd.point_list.astype(np.int64))
    for tile in range(gxn * gyn):
        r0, r1 = int(ranges[tile, 0]), int(ranges[tile, 1])
        tx0, ty0 = (tile % gxn) * 16, (tile // gxn) * 16
        ys, xs = torch.meshgrid(torch.arange(ty0, min(ty0 + 16, H)), torch.arange(tx0, min(tx0 + 16, W)), indexing="ij")
        xs, ys = xs.reshape(-1), ys.reshape(-1)
        n = xs.numel()
        pxf, pyf = xs.to(dt), ys.to(dt)
        if dd_only:
            out_dd[0, ys, xs] = _depth_distortion_tile(plist[r0:r1], pix_x, pix_y, con_x, con_y, con_z, opac, d_ndc, pxf, pyf)
            continue
        T = torch.ones(n, dtype=dt)
        done = torch.zeros(n, dtype=torch.bool)
        Cc = torch.zeros(n, 3, dtype=dt)
        Pp = torch.zeros(n, 7, dtype=dt)
        Dd = torch.zeros(n, dtype=dt)
        Aa = torch.zeros(n, dtype=dt)
        DD = torch.zeros(n, dtype=dt)
        DD_D = torch.zeros(n, dtype=dt)
        DD_D2 = torch.zeros(n, dtype=dt)
        for k in range(r0, r1):
            if bool(done.all()):
                break
            j = int(plist[k])
            dx = pix_x[j] - pxf
            dy = pix_y[j] - pyf
            power = -0.5 * (con_x[j] * dx * dx + con_z[j] * dy * dy) - con_y[j] * dx * dy
            G = torch.exp(power)
            a_raw = opac[j] * G
            alpha = a_raw + (torch.clamp(a_raw, max=0.99) - a_raw).detach()
            skip = (power > 0) | (alpha < 1.0 / 255.0)
            test_T = T * (1 - alpha)
            if settings.get("margins") is not None:
                mg, live = settings["margins"], ~done
                for name, val, where in (("alpha", alpha - 1.0 / 255.0, live & (power <= 0)), ("power", power, live),
                                         ("test_T", test_T - 1e-4, live & ~skip)):
                    if bool(where.any()):
                        mg[name] = min(mg.get(name, math.inf), float(val.detach().abs()[where].min()))
            newly_done = (~skip) & (~done) & (test_T < 1e-4)
            done = done | newly_done
            act = (~skip) & (~done)
            am = act.to(dt)
            w = alpha * T * am
            w_p = alpha * T * T * am
            Cc = Cc + w[:, None] * rgb[j][None, :]
            Pp = Pp + w_p[:, None] * ph7[j][None, :]
            Dd = Dd + w * dist_out[j]
            zz = d_ndc[j]
            DD = DD + w * (zz * zz * Aa - 2 * zz * DD_D + DD_D2)
            DD_D = DD_D + w * zz
            DD_D2 = DD_D2 + w * zz * zz
            Aa = Aa + w
            T = torch.where(act, test_T, T)
        colors_l.append(Cc + T[:, None] * bg[:3, ys, xs].T)
        phasors_l.append(Pp + T[:, None] * bg[:7, ys, xs].T)
        depth_l.append(Dd)
        acc_l.append(Aa)
        dd_l.append(DD)
        idx_l.append((ys, xs))
    for (ys, xs), cc, pp, dd_, aa, ddd in zip(idx_l, colors_l, phasors_l, depth_l, acc_l, dd_l):
        out_color[:, ys, xs] = cc.T
        out_phasor[:, ys, xs] = pp.T
        out_depth[0, ys, xs] = dd_
        out_acc[0, ys, xs] = aa
        out_dd[0, ys, xs] = ddd
    if dd_only:
        return dict(depth_distortion=out_dd)
    return dict(color=out_color, phasor=out_phasor, depth=out_depth, acc=out_acc,
                depth_distortion=out_dd, ndc=ndc, uses=uses)
