"""The per-Gaussian regularisers of the training loss as one autograd node (``csrc/k_reg.hip``, ``include/gftorf_reg.h``):
the motion term ``lambda_mlp_reg * torch.abs(d_xyz).mean()`` (``train.py:239-240``), the depth-distortion term
``lambda_dd * render_pkg["depth_distortion"].mean()`` (``:266-267``), the opacity entropy of the dynamic Gaussians
(``:270-272``) and the scale term of the visible ones (``:275-277``).  In eager PyTorch the four are ~20 small launches
forward and as many backward, and the two masked ones select their rows with ``t[bool_mask]``, which runs ``nonzero`` and
reads the row count back on the host -- they cannot be captured in a graph.  Here the masks are read on the device: two
launches forward (the sums, one workgroup that finishes them), one backward, no host read, no atomic and no memset, so the
call and its backward can be captured, and a replay follows the masks, the radii and a device weight vector as they are then.

With ``raw=True`` the opacity and scaling passed are the model's own tensors (``pc._opacity``, ``pc._scaling``); the
kernels apply ``sigmoid`` and ``exp`` themselves and the gradients are those of the raw tensors, so a caller on
``assemble_parameters`` never evaluates ``pc.get_opacity`` / ``pc.get_scaling``.

The one difference from the reference: an EMPTY selection -- no dynamic Gaussian, no visible one, a ``d_xyz`` of no rows --
gives 0 for its term and zero gradients, where the reference's mean of an empty tensor is NaN.  There is no CPU path.
"""
import collections

import torch

from . import _args, _lib
from ._args import ptr_nonempty as _ptr

TERMS = ("motion", "opacity_entropy", "scale", "depth_distortion")          # the order of the means and of `weights`

RegTerms = collections.namedtuple("RegTerms", ["means", "counts"])
RegTerms.__doc__ = """``means``: float32 [4], the unweighted means in the order of ``TERMS`` (0 for an absent term);
``counts``: int32 [2], the rows selected by the motion mask and by the visibility.  Detached device tensors."""


def _tensor(t, name, grad_ok=True):
    if not isinstance(t, torch.Tensor):
        raise TypeError("gftorf_amd.reg: %s must be a tensor, got %s" % (name, type(t).__name__))
    if t.requires_grad and not grad_ok:
        raise NotImplementedError("gftorf_amd.reg: gradients flow to d_xyz, opacity, scaling and depth_distortion only; "
                                  "%s requires grad" % name)
    return t


def _want(name, t, ok, want):
    if not ok:
        raise RuntimeError("gftorf_amd.reg: %s must be %s, got %s" % (name, want, list(t.shape)))


def _check(d_xyz, opacity, motion_mask, scaling, visible, dd, weights):
    """Shapes, dtypes and gradients first, then the devices: every tensor on the first one's HIP device."""
    named = []
    if d_xyz is not None:
        _want("d_xyz", _tensor(d_xyz, "d_xyz"), d_xyz.dim() == 2 and d_xyz.shape[1] == 3, "[*, 3]")
        named.append((d_xyz, "d_xyz", torch.float32))
    P = None
    if opacity is not None or motion_mask is not None:
        if opacity is None or motion_mask is None:
            raise ValueError("gftorf_amd.reg: opacity and motion_mask come together")          # (opacity without its mask)
        _tensor(opacity, "opacity"), _tensor(motion_mask, "motion_mask", grad_ok=False)
        _want("opacity", opacity, opacity.dim() == 1 or (opacity.dim() == 2 and opacity.shape[1] == 1), "[P, 1] or [P]")
        P = int(opacity.shape[0])
        _want("motion_mask", motion_mask, tuple(motion_mask.shape) == (P,), "[%d]" % P)
        named += [(opacity, "opacity", torch.float32), (motion_mask, "motion_mask", torch.bool)]
    if scaling is not None or visible is not None:
        if scaling is None or visible is None:
            raise ValueError("gftorf_amd.reg: scaling and visible come together")
        _tensor(scaling, "scaling"), _tensor(visible, "visible", grad_ok=False)
        _want("scaling", scaling, scaling.dim() == 2 and scaling.shape[1] in (1, 3) and P in (None, int(scaling.shape[0])),
              "[P, 3] or [P, 1]" if P is None else "[%d, 3] or [%d, 1]" % (P, P))
        P = int(scaling.shape[0])
        _want("visible", visible, tuple(visible.shape) == (P,), "[%d]" % P)
        named += [(scaling, "scaling", torch.float32), (visible, "visible", (torch.bool, torch.int32))]
    if dd is not None:
        named.append((_tensor(dd, "depth_distortion"), "depth_distortion", torch.float32))
    if weights is not None:
        _want("weights", _tensor(weights, "weights", grad_ok=False), tuple(weights.shape) == (4,), "[4]")
        named.append((weights, "weights", torch.float32))
    for t, name, dtype in named:
        if t.dtype != dtype and not (isinstance(dtype, tuple) and t.dtype in dtype):
            names = " or ".join(str(d) for d in (dtype if isinstance(dtype, tuple) else (dtype,)))
            raise TypeError("gftorf_amd.reg: %s must be %s, got %s" % (name, names, t.dtype))
    _args.devices("gftorf_amd.reg", "regulariser", named)


class _Regularizers(torch.autograd.Function):
    """(weighted total, result block) of the supplied terms: k_reg_fwd + k_reg_finish forward, k_reg_bwd backward."""

    @staticmethod
    def forward(ctx, d_xyz, opacity, scaling, dd, motion_mask, visible, weights, w, raw):
        lib = _lib.load()
        src = (d_xyz, opacity, scaling, dd)
        dev = next(t for t in src if t is not None).device
        cont = lambda t: None if t is None else t.detach().contiguous()
        a, o, s, d, m, v, wd = (cont(t) for t in (d_xyz, opacity, scaling, dd, motion_mask, visible, weights))
        rows = o if o is not None else s
        sizes = (a.numel() if a is not None else 0, int(rows.shape[0]) if rows is not None else 0, d.numel() if d is not None else 0)
        flags = (int(raw), int(s.shape[1]) if s is not None else 3, int(raw),
                 int(v is not None and v.dtype == torch.int32))
        res = torch.empty((int(lib.gft_reg_result_words()),), device=dev, dtype=torch.float32)
        blocks = int(lib.gft_reg_blocks(*sizes))
        if blocks == 0:             # nothing but empty tensors: every term is 0
            res.zero_()
        else:
            partials = torch.empty((blocks, _lib.REG_PARTIAL_WORDS), device=dev, dtype=torch.int32)
            with _lib.on_device(dev):
                _lib.check(lib.gft_reg_forward(_lib.raw_stream(dev), *sizes, _ptr(a), _ptr(o), _ptr(m) if _ptr(o) else None, flags[0],
                                               _ptr(s), flags[1], flags[2], _ptr(v) if _ptr(s) else None, flags[3], _ptr(d),
                                               _ptr(wd), *w, partials.data_ptr(), res.data_ptr()))
        ctx.call = (sizes, flags, w, blocks, tuple(None if t is None else tuple(t.shape) for t in src))
        ctx.save_for_backward(a, o, s, m, v, wd, res)
        ctx.mark_non_differentiable(res)
        return res[_lib.REG_TOTAL], res

    @staticmethod
    def backward(ctx, g, _g_res):
        lib = _lib.load()
        a, o, s, m, v, wd, res = ctx.saved_tensors
        sizes, flags, w, blocks, shapes = ctx.call
        dev = res.device
        need = ctx.needs_input_grad
        grads = [torch.empty(shape, device=dev, dtype=torch.float32) if shape is not None and need[k] else None
                 for k, shape in enumerate(shapes)]
        if blocks and any(_ptr(t) for t in grads):
            gp = g.detach().float()            # a 0-dim gradient: one float at data_ptr()
            with _lib.on_device(dev):
                _lib.check(lib.gft_reg_backward(_lib.raw_stream(dev), *sizes, _ptr(a), _ptr(o), _ptr(m) if _ptr(o) else None, flags[0],
                                                _ptr(s), flags[1], flags[2], _ptr(v) if _ptr(s) else None, flags[3], _ptr(wd), *w,
                                                res.data_ptr(), gp.data_ptr(), *(_ptr(t) for t in grads)))
        return (*grads, None, None, None, None, None)


def regularizers(d_xyz=None, w_mlp=0.0, opacity=None, motion_mask=None, w_oe=0.0, scaling=None, visible=None, w_scale=0.0,
                 depth_distortion=None, w_dd=0.0, raw=False, weights=None, return_terms=False):
    """``w_mlp * |d_xyz|.mean() + w_oe * entropy(opacity[motion_mask]).mean() + w_scale * (scaling[visible].mean(-1) ** 2).mean()
    + w_dd * depth_distortion.mean()`` -- the statements of ``train.py:240, 272, 277, 267`` -- as one 0-dim tensor of one
    autograd node.  The iteration windows of ``train.py:266, 270, 275`` stay with the caller::

        loss = loss + reg.regularizers(d_xyz=d_xyz, w_mlp=opt.lambda_mlp_reg,
                                       opacity=pc._opacity, motion_mask=pc.get_motion_mask, w_oe=opt.lambda_oe,
                                       scaling=pc._scaling, visible=radii, w_scale=opt.lambda_scale,
                                       depth_distortion=render_pkg["depth_distortion"], w_dd=opt.lambda_dd, raw=True)

    ``d_xyz`` [*, 3]; ``opacity`` [P, 1] or [P] with ``motion_mask`` bool [P]; ``scaling`` [P, 3] or [P, 1] (the reference's
    ``isotropic_gaussians``: the row mean is the value) with ``visible`` bool [P] or the rasterizer's int32 ``radii`` [P]
    (visible where > 0); ``depth_distortion`` of any shape.  All fp32 on one HIP device; gradients flow to the four tensors,
    never to a mask.  ``raw=False``: ``opacity`` / ``scaling`` are ``pc.get_opacity`` / ``pc.get_scaling`` and get the
    gradients; ``raw=True``: they are ``pc._opacity`` / ``pc._scaling``, activated inside the kernels.

    A term is absent when its tensor is None (its mask is then ignored), when ``d_xyz`` is a Python number (``train.py:164``'s ``0.0`` of a static
    scene), or when its weight is the float ``0.0``.  With ``weights`` -- a float32 device tensor ``[w_mlp, w_oe, w_scale,
    w_dd]`` -- in place of the four floats every supplied term is computed and the weights are read on the device when the
    kernels run: a zero weight gives a zero contribution and zero gradients, and a captured graph follows a window that
    opens or closes by a write into that tensor.  Without any term the result is the float ``0.0``.

    ``return_terms=True``: ``(loss, RegTerms(means, counts))`` with the four unweighted means and the two selected row
    counts as detached device tensors, for logging (nothing is read on the host).

    Unlike the reference, a term over an EMPTY selection (no True in the mask, nothing visible, ``d_xyz`` without rows) is
    0 with zero gradients, not NaN."""
    if not isinstance(d_xyz, torch.Tensor):
        d_xyz = None            # 0.0 of a static scene
    if weights is None:
        w = tuple(float(x) for x in (w_mlp, w_oe, w_scale, w_dd))
        if w[0] == 0.0:
            d_xyz = None
        if w[1] == 0.0:
            opacity = motion_mask = None
        if w[2] == 0.0:
            scaling = visible = None
        if w[3] == 0.0:
            depth_distortion = None
    else:
        w = (0.0, 0.0, 0.0, 0.0)
    if opacity is None:
        motion_mask = None          # a mask without its tensor: the term is absent
    if scaling is None:
        visible = None
    if all(t is None for t in (d_xyz, opacity, scaling, depth_distortion)):
        return (0.0, None) if return_terms else 0.0
    _check(d_xyz, opacity, motion_mask, scaling, visible, depth_distortion, weights)
    loss, res = _Regularizers.apply(d_xyz, opacity, scaling, depth_distortion, motion_mask, visible, weights, w, bool(raw))
    if not return_terms:
        return loss
    counts = res.view(torch.int32)[_lib.REG_COUNTS:_lib.REG_COUNTS + 2]
    return loss, RegTerms(res[_lib.REG_MEANS:_lib.REG_MEANS + 4], counts)


def motion_reg(d_xyz):
    """Drop-in for ``torch.abs(d_xyz).mean()`` (``train.py:240``)."""
    return regularizers(d_xyz=d_xyz, w_mlp=1.0)


def dd_loss(img):
    """Drop-in for ``render_pkg["depth_distortion"].mean()`` (``train.py:267``)."""
    return regularizers(depth_distortion=img, w_dd=1.0)


def opacity_entropy(opacity, motion_mask, raw=False):
    """Drop-in for ``train.py:271-272``: the mean over ``o = opacity[motion_mask]`` of
    ``-o * log(o + 1e-10) - (1 - o) * log(1 - o + 1e-10)``; 0 when the mask selects nothing."""
    return regularizers(opacity=opacity, motion_mask=motion_mask, w_oe=1.0, raw=raw)


def scale_loss(scaling, visible, raw=False):
    """Drop-in for ``train.py:276-277``: ``(scaling[visible].mean(dim=-1) ** 2).mean()``; 0 when nothing is visible."""
    return regularizers(scaling=scaling, visible=visible, w_scale=1.0, raw=raw)
