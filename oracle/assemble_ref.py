"""ORACLE (test infrastructure only) of the fused input assembly -- SURVEY section 8(f) row 1.

Two CPU restatements of the reference's glue, ``gaussian_renderer/__init__.py:81-105``:

* :func:`assemble_eager`: the reference's statements as they stand (torch.zeros + boolean-mask
  assignment, ``rotation_activation = torch.nn.functional.normalize``,
  ``scene/gaussian_model.py:43``), on CPU tensors; autograd of these eager ops is the oracle of
  the backward.
* :func:`assemble_loops`: plain numpy loops over Gaussians (independent of torch indexing
  semantics), used to pin the eager restatement on small cases.

:func:`parameters_eager` and :func:`parameters_loops` are the same two restatements for
``gftorf_amd.assemble_parameters``: the model's own tensors go in, and what ``pc.get_*`` computes from
them (``scene/gaussian_model.py:123-153``) is stated in front of the assembly.

Only tests/, __graft_entry__.smoke() and bench.py's baseline leg may import this module.
"""
import numpy as np
import torch


def assemble_eager(xyz, screenspace_points, opacity, scaling, rotation, rotation_raw, features_color,
                   features_phasor, motion_mask, d_xyz=0.0, d_rot=0.0, d_sh=0.0, d_sh_p=0.0,
                   render_regions=("static", "dynamic")):
    """gaussian_renderer/__init__.py:81-105, names as in the reference (pc.get_xyz -> xyz ...)."""
    means3D = torch.zeros(xyz.shape, device=xyz.device, dtype=xyz.dtype)                      # :81
    means2D = torch.zeros(screenspace_points.shape, device=xyz.device, dtype=xyz.dtype)       # :82
    out_opacity = torch.zeros(opacity.shape, device=xyz.device, dtype=xyz.dtype)              # :83
    scales = torch.zeros(scaling.shape, device=xyz.device, dtype=xyz.dtype)                   # :84
    rotations = torch.zeros(rotation.shape, device=xyz.device, dtype=xyz.dtype)               # :85
    shs = torch.zeros(features_color.shape, device=xyz.device, dtype=xyz.dtype)               # :86
    shs_p = torch.zeros(features_phasor.shape, device=xyz.device, dtype=xyz.dtype)            # :87
    m = motion_mask
    if "static" in render_regions:                                                             # :89-96
        means3D[~m] = xyz[~m]
        means2D[~m] = screenspace_points[~m]
        out_opacity[~m] = opacity[~m]
        scales[~m] = scaling[~m]
        rotations[~m] = rotation[~m]
        shs[~m] = features_color[~m]
        shs_p[~m] = features_phasor[~m]
    if "dynamic" in render_regions:                                                            # :97-104
        means3D[m] = xyz[m] + d_xyz
        means2D[m] = screenspace_points[m]
        out_opacity[m] = opacity[m]
        scales[m] = scaling[m]
        rotations[m] = torch.nn.functional.normalize(rotation_raw[m] + d_rot)
        shs[m] = features_color[m] + d_sh
        shs_p[m] = features_phasor[m] + d_sh_p
    return means3D, means2D, out_opacity, scales, rotations, shs, shs_p


def assemble_loops(xyz, ssp, opacity, scaling, rotation, rotation_raw, fc, fp, mask, d_xyz=0.0, d_rot=0.0,
                   d_sh=0.0, d_sh_p=0.0, render_regions=("static", "dynamic")):
    """Same statements, one Gaussian at a time (numpy float32)."""
    f = np.float32
    P = xyz.shape[0]
    outs = [np.zeros_like(np.asarray(a, f)) for a in (xyz, ssp, opacity, scaling, rotation, fc, fp)]
    row = lambda d, k: (np.asarray(d, f)[k] if isinstance(d, np.ndarray) else f(d))
    k = 0
    for i in range(P):
        if mask[i]:
            if "dynamic" in render_regions:
                outs[0][i] = xyz[i] + row(d_xyz, k)
                outs[1][i] = ssp[i]
                outs[2][i] = opacity[i]
                outs[3][i] = scaling[i]
                q = (rotation_raw[i] + row(d_rot, k)).astype(f)
                n = max(f(np.sqrt(np.sum(q * q, dtype=f))), f(1e-12))
                outs[4][i] = q / n
                outs[5][i] = fc[i] + row(d_sh, k)
                outs[6][i] = fp[i] + row(d_sh_p, k)
            k += 1
        elif "static" in render_regions:
            for o, s in zip(outs, (xyz, ssp, opacity, scaling, rotation, fc, fp)):
                o[i] = s[i]
    return outs


def parameters_eager(xyz, screenspace_points, opacity_raw, scaling_raw, rotation_raw, features_dc_color, features_rest_color,
                     phase_f_dc, phase_f_rest, amp_f_dc, amp_f_rest, motion_mask, d_xyz=0.0, d_rot=0.0, d_sh=0.0, d_sh_p=0.0,
                     render_regions=("static", "dynamic")):
    """The argument list of ``assemble_parameters``: pc.get_opacity, get_scaling, get_rotation, get_features_color and
    get_features_phasor from their formulas, then :func:`assemble_eager`.  In the dtype of its arguments: float64 is the
    reference of the activations, float32 the reference of what is copied or added once."""
    opacity = torch.sigmoid(opacity_raw)
    scaling = torch.exp(scaling_raw)
    rotation = torch.nn.functional.normalize(rotation_raw)
    features_color = torch.cat((features_dc_color, features_rest_color), dim=1)
    features_phasor = torch.cat((torch.cat((phase_f_dc, phase_f_rest), dim=1), torch.cat((amp_f_dc, amp_f_rest), dim=1)), dim=2)
    return assemble_eager(xyz, screenspace_points, opacity, scaling, rotation, rotation_raw, features_color, features_phasor,
                          motion_mask, d_xyz, d_rot, d_sh, d_sh_p, render_regions)


def parameters_loops(xyz, ssp, opacity_raw, scaling_raw, rotation_raw, f_dc, f_rest, phase_dc, phase_rest, amp_dc, amp_rest, mask,
                     d_xyz=0.0, d_rot=0.0, d_sh=0.0, d_sh_p=0.0, render_regions=("static", "dynamic")):
    """The same, one Gaussian and one coefficient at a time, the parts indexed where they lie (no concatenation); numpy, in
    the dtype of ``xyz``."""
    f = xyz.dtype.type
    P, M, M_p = xyz.shape[0], 1 + f_rest.shape[1], 1 + phase_rest.shape[1]
    means3D, means2D, opacity = np.zeros((P, 3), f), np.zeros((P, 3), f), np.zeros(opacity_raw.shape, f)
    scales, rotations = np.zeros((P, 3), f), np.zeros((P, 4), f)
    shs, shs_p = np.zeros((P, M, 3), f), np.zeros((P, M_p, 2), f)
    off = lambda d, k, *at: (d[(k,) + at] if isinstance(d, np.ndarray) else f(d))
    k = 0
    for i in range(P):
        dyn = bool(mask[i])
        if ("dynamic" if dyn else "static") in render_regions:
            for c in range(3):
                means3D[i, c] = xyz[i, c] + off(d_xyz, k, c) if dyn else xyz[i, c]
                means2D[i, c] = ssp[i, c]
                scales[i, c] = np.exp(scaling_raw[i, c])
            opacity[i] = f(1) / (f(1) + np.exp(-opacity_raw[i]))
            q = [rotation_raw[i, c] + off(d_rot, k, c) if dyn else rotation_raw[i, c] for c in range(4)]
            n = max(np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), f(1e-12))
            for c in range(4):
                rotations[i, c] = q[c] / n
            for j in range(M):
                for c in range(3):
                    v = f_dc[i, 0, c] if j == 0 else f_rest[i, j - 1, c]
                    shs[i, j, c] = v + off(d_sh, k, j, c) if dyn else v
            for j in range(M_p):
                ph = phase_dc[i, 0, 0] if j == 0 else phase_rest[i, j - 1, 0]
                am = amp_dc[i, 0, 0] if j == 0 else amp_rest[i, j - 1, 0]
                shs_p[i, j, 0] = ph + off(d_sh_p, k, j, 0) if dyn else ph
                shs_p[i, j, 1] = am + off(d_sh_p, k, j, 1) if dyn else am
        k += dyn
    return [means3D, means2D, opacity, scales, rotations, shs, shs_p]
