"""Per-Gaussian bookkeeping around the rasterizer (bookkeeping part).

Fused replacements of the boolean-mask tensor surgery of the reference's training loop -- in eager
PyTorch every ``t[mask]`` / ``t[mask] += ...`` is a ``nonzero()`` with a host synchronisation plus a
gather or scatter, which at 1 M Gaussians costs more per iteration than the rasterizer does:

* :func:`add_densification_stats` -- ``train.py:443`` + ``GaussianModel.add_densification_stats``
  (``scene/gaussian_model.py:648-654``) in one in-place pass.
* :func:`select_rows` -- ``[t[mask] for t in tensors]`` with one rank computation for all tensors.
* :func:`prune_optimizer`, :func:`cat_tensors_to_optimizer` -- ``GaussianModel._prune_optimizer`` /
  ``cat_tensors_to_optimizer`` (``scene/gaussian_model.py:473-492, 516-537``) on top of it: same
  ``param_groups`` / ``state`` surgery, same results (bit-identical: pure data movement).
* :func:`prune_points`, :func:`densification_postfix`, :func:`densify_and_clone`, :func:`densify_and_split`,
  :func:`densify_and_prune`, :func:`prune` -- the composites of ``scene/gaussian_model.py:494-514, 539-646`` as
  functions of the model object (``pc``: anything with the reference ``GaussianModel``'s attributes): the method
  bodies a maintainer replaces by one call each.  Selection masks are the reference's own torch expressions, the
  split's ``torch.normal`` draw is torch's (same generator, same samples); every ``t[mask]`` is a row compaction
  with one rank computation per mask.
* :func:`densify_and_prune_fused` -- the whole ``densify_and_prune`` event as one plan and one pass over every tensor (two
  host reads instead of four, every parameter and moment read once and written once), with the same result as the composite;
  its :class:`DensifyResult` carries the new motion mask, a ready ``DeformQuery`` and any caller tensor across the event.
* :func:`split_children` -- the positions of a split's children in one kernel (``gft_split_children``) instead of the
  reference's ``build_rotation`` + ``torch.normal`` + ``torch.bmm`` statements: the opt-in ``children="kernel"`` route of
  :func:`densify_and_prune_fused` and :func:`densify_and_split`, with a contract of its own for the children's ``xyz`` rows.

Kernels: ``csrc/k_densify.hip`` behind ``include/gftorf_densify.h``; no CPU path.
"""
import ctypes as C

import torch
from torch import nn

from . import _lib

_SKIP = ("phase_offset", "dc_offset")          # groups the reference leaves alone (gaussian_model.py:459,476,519)


def _dev_check(t, who):
    if t.device.type != "cuda":
        raise RuntimeError("gftorf_amd.densify.%s runs on a HIP device only (got a tensor on %s); there is no CPU path"
                           % (who, t.device))


def _mask_u8(mask, P, dev, who):
    if mask.dtype != torch.bool or mask.numel() != P:
        raise RuntimeError("%s: the mask must be a bool tensor with one entry per row (%d), got %s %s"
                           % (who, P, mask.dtype, tuple(mask.shape)))
    return mask.to(dev).contiguous().view(torch.uint8)


def add_densification_stats(xyz_gradient_accum, denom, max_radii2D, viewspace_grad, update_filter, pixels, radii,
                            apply_mask=None):
    """In place, for the rows of ``update_filter`` (``visibility_filter = radii > 0``):

        max_radii2D[f] = max(max_radii2D[f], radii[f])                                   (train.py:443)
        xyz_gradient_accum[f'] += norm(viewspace_grad[f', :2], dim=-1, keepdim=True) * pixels[f']
        denom[f'] += pixels[f']                                          (gaussian_model.py:648-654)

    with ``f' = f`` or, with ``apply_mask``, ``f & apply_mask`` (the reference's second branch; it only runs
    there when ``f`` is a subset of ``apply_mask``).  ``viewspace_grad`` is ``viewspace_point_tensor.grad``.
    ``max_radii2D`` / ``radii`` may be None to leave the radii alone."""
    lib = _lib.load()
    _dev_check(xyz_gradient_accum, "add_densification_stats")
    dev = xyz_gradient_accum.device
    P = xyz_gradient_accum.size(0)
    for t, n in ((xyz_gradient_accum, "xyz_gradient_accum"), (denom, "denom"), (max_radii2D, "max_radii2D")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != P or t.device != dev):
            raise RuntimeError("%s must be a contiguous float32 tensor with %d entries on %s" % (n, P, dev))
    g = viewspace_grad.detach()
    if g.dtype != torch.float32 or tuple(g.shape) != (P, 3):
        raise RuntimeError("viewspace_grad must be float32 [%d, 3]" % P)
    g = g.contiguous()
    px = pixels.detach().float().contiguous()
    if px.numel() != P:
        raise RuntimeError("pixels must hold one value per Gaussian")
    uf = _mask_u8(update_filter, P, dev, "add_densification_stats")
    am = _mask_u8(apply_mask, P, dev, "add_densification_stats") if apply_mask is not None else None
    rd = None
    if max_radii2D is not None:
        if radii is None or radii.dtype != torch.int32 or radii.numel() != P:
            raise RuntimeError("radii must be the rasterizer's int32 [P] tensor")
        rd = radii.contiguous()
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with _lib.on_device(dev):
        _lib.check(lib.gft_densify_stats(_lib.raw_stream(dev), P, ptr(g), ptr(px), ptr(rd), ptr(uf), ptr(am),
                                         ptr(xyz_gradient_accum), ptr(denom), ptr(max_radii2D)))


class RowSelection:
    """``mask`` turned into an output row per kept row, once; :meth:`take` then compacts any tensor whose
    first dimension is the mask's (``t[mask]``)."""

    def __init__(self, mask):
        lib = _lib.load()
        _dev_check(mask, "RowSelection")
        self.dev = mask.device
        self.P = mask.numel()
        self.mask = _mask_u8(mask.reshape(-1), self.P, self.dev, "RowSelection")
        self.rank = torch.empty((self.P,), device=self.dev, dtype=torch.int32)
        scratch = torch.empty((lib.gft_rows_rank_scratch_bytes(self.P),), device=self.dev, dtype=torch.uint8)
        n = C.c_int64(0)
        with _lib.on_device(self.dev):
            _lib.check(lib.gft_rows_rank(_lib.raw_stream(self.dev), self.P,
                                         self.mask.data_ptr() if self.P else None, self.rank.data_ptr() if self.P else None,
                                         scratch.data_ptr() if self.P else None, C.byref(n)))
        self.count = int(n.value)
        self._rows = None

    def rows(self):
        """The kept rows in increasing order (int32 [count]): ``mask.nonzero()`` without its host read."""
        if self._rows is None:
            self._rows = self.take(torch.arange(self.P, device=self.dev, dtype=torch.int32))
        return self._rows

    def take(self, t, out=None):
        """``t[mask]`` (into ``out[:count]`` when given)."""
        lib = _lib.load()
        if t.size(0) != self.P or t.device != self.dev:
            raise RuntimeError("RowSelection.take: tensor with %d rows on %s, mask has %d rows on %s"
                               % (t.size(0), t.device, self.P, self.dev))
        src = t.detach().contiguous()
        row_bytes = (src.numel() // max(self.P, 1)) * src.element_size()
        if row_bytes % 4:
            return t.detach()[self.mask.view(torch.bool)] if out is None else out[:self.count].copy_(t.detach()[self.mask.view(torch.bool)])
        dst = torch.empty((self.count,) + tuple(src.shape[1:]), device=self.dev, dtype=src.dtype) if out is None else out
        if out is not None and (not out.is_contiguous() or out.dtype != src.dtype or tuple(out.shape[1:]) != tuple(src.shape[1:])
                                or out.size(0) < self.count):
            raise RuntimeError("RowSelection.take: unsuitable output tensor")
        if self.count and row_bytes:
            with _lib.on_device(self.dev):
                _lib.check(lib.gft_rows_gather(_lib.raw_stream(self.dev), self.P, self.mask.data_ptr(),
                                               self.rank.data_ptr(), src.data_ptr(), dst.data_ptr(), row_bytes))
        return dst


    def take_many(self, tensors):
        """``[t[mask] for t in tensors]`` (one launch per tensor: measured faster than one launch over a
        table of tensors, whose workgroups first have to find their tensor)."""
        return [self.take(t) for t in tensors]


def select_rows(mask, *tensors):
    """``[t[mask] for t in tensors]``."""
    return RowSelection(mask).take_many(list(tensors))


def prune_optimizer(optimizer, mask, skip=_SKIP, return_selection=False):
    """``GaussianModel._prune_optimizer`` (scene/gaussian_model.py:473-492): keeps the rows of ``mask`` in every
    group's parameter and Adam moments; returns ``{group name: new nn.Parameter}`` like the reference.  With
    ``return_selection`` the pair ``(dict, RowSelection)``: the selection compacts further per-Gaussian tensors
    (the densification statistics) without ranking the mask again."""
    sel = RowSelection(mask)
    groups = [g for g in optimizer.param_groups if g["name"] not in skip]
    todo = []
    for group in groups:
        p = group["params"][0]
        state = optimizer.state.get(p, None)
        todo.append(p)
        if state is not None:
            todo += [state["exp_avg"], state["exp_avg_sq"]]
    kept = iter(sel.take_many(todo))
    out = {}
    for group in groups:
        p = group["params"][0]
        state = optimizer.state.get(p, None)
        new_p = nn.Parameter(next(kept).requires_grad_(True))
        if state is not None:
            state["exp_avg"] = next(kept)
            state["exp_avg_sq"] = next(kept)
            del optimizer.state[p]
            group["params"][0] = new_p
            optimizer.state[new_p] = state
        else:
            group["params"][0] = new_p
        out[group["name"]] = new_p
    return (out, sel) if return_selection else out


def cat_tensors_to_optimizer(optimizer, tensors_dict, skip=_SKIP):
    """``GaussianModel.cat_tensors_to_optimizer`` (scene/gaussian_model.py:516-537): appends the new rows to
    every group's parameter, zero rows to its Adam moments."""
    out = {}
    for group in optimizer.param_groups:
        if group["name"] in skip:
            continue
        assert len(group["params"]) == 1
        ext = tensors_dict[group["name"]]
        p = group["params"][0]
        state = optimizer.state.get(p, None)
        new_p = nn.Parameter(torch.cat((p.detach(), ext), dim=0).requires_grad_(True))
        if state is not None:
            for k in ("exp_avg", "exp_avg_sq"):
                grown = torch.zeros((p.size(0) + ext.size(0),) + tuple(p.shape[1:]), device=p.device, dtype=p.dtype)
                grown[:p.size(0)] = state[k]
                state[k] = grown
            del optimizer.state[p]
            group["params"][0] = new_p
            optimizer.state[new_p] = state
        else:
            group["params"][0] = new_p
        out[group["name"]] = new_p
    return out


# ---- the composites of scene/gaussian_model.py:494-646 ------------------------------------------------------------
# optimizer group name -> attribute of the model (gaussian_model.py:498-508)
GROUP_ATTR = {"xyz": "_xyz", "f_dc_color": "_features_dc_color", "f_rest_color": "_features_rest_color",
              "phase_f_dc": "_features_dc_phase", "phase_f_rest": "_features_rest_phase", "amp_f_dc": "_features_dc_amp",
              "amp_f_rest": "_features_rest_amp", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation",
              "f_seg_color": "_features_seg_color"}


def _adopt(pc, tensors):
    for name, attr in GROUP_ATTR.items():
        setattr(pc, attr, tensors[name])


def prune_points(pc, mask):
    """``GaussianModel.prune_points`` (gaussian_model.py:494-514): removes the Gaussians of ``mask``."""
    valid = ~mask
    tensors, sel = prune_optimizer(pc.optimizer, valid, return_selection=True)
    _adopt(pc, tensors)
    pc.xyz_gradient_accum = sel.take(pc.xyz_gradient_accum)
    pc.denom = sel.take(pc.denom)
    pc.max_radii2D = sel.take(pc.max_radii2D)


def densification_postfix(pc, new):
    """``GaussianModel.densification_postfix`` (gaussian_model.py:539-569); ``new``: group name -> rows to append."""
    _adopt(pc, cat_tensors_to_optimizer(pc.optimizer, new))
    n, dev = pc.get_xyz.shape[0], pc.get_xyz.device
    pc.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
    pc.denom = torch.zeros((n, 1), device=dev)
    pc.max_radii2D = torch.zeros((n,), device=dev)


def _rotation_matrices(r):
    """``build_rotation`` (utils/general_utils.py:91-112): (r, x, y, z) quaternions, normalised here, to 3x3."""
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def densify_and_clone(pc, grads, grad_threshold, scene_extent):
    """``GaussianModel.densify_and_clone`` (gaussian_model.py:603-622): small Gaussians with a large view-space
    gradient are duplicated."""
    mask = torch.where(torch.norm(grads, dim=-1) >= grad_threshold, True, False)
    mask = torch.logical_and(mask, torch.max(pc.get_scaling, dim=1).values <= pc.percent_dense * scene_extent)
    sel = RowSelection(mask)
    densification_postfix(pc, {name: sel.take(getattr(pc, attr)) for name, attr in GROUP_ATTR.items()})


def _children_route(children, who):
    if children not in ("torch", "kernel"):
        raise ValueError("%s: children must be 'torch' or 'kernel', got %r" % (who, children))
    return children == "kernel"


def split_children(pc, split_rows, n_split, N=2):
    """The children of the ``n_split`` rows ``split_rows`` (int32, increasing) of ``pc``: ``(new_xyz [N * n_split, 3],
    new_scaling [N * n_split, 3 or 1], child_max_scaling [N * n_split])``, child ``k * n_split + j`` belonging to row
    ``split_rows[j]`` as ``repeat(N, ...)`` lays them out.  The positions come from one kernel (``gft_split_children``): the
    standard normals are one ``torch.randn((N * n_split, 3))``, which consumes torch's generator as ``densify_and_split``'s
    ``torch.normal(mean=zeros, std=stds)`` does; rotation, activated scaling and position of the split rows are read from the
    model's tensors, no gathered copies, no rotation matrices in memory, no ``bmm``.  The scalings are the reference's own
    torch statements on one gather of the split rows (``log`` and ``exp`` stay torch's: their last bit is the build's).

    The positions' contract is the kernel's own (``include/gftorf_densify.h``), not ``torch.bmm``'s bits: the rotation of the
    same samples by the same R as an ascending chain of fused multiply-adds, within 16 eps (|s_0| + |s_1| + |s_2|) + 2 eps
    |exact| of the exact value, as the reference's own route is."""
    xyz = pc.get_xyz
    _dev_check(xyz, "split_children")
    lib = _lib.load()
    dev = xyz.device
    P, S, N = int(xyz.shape[0]), int(n_split), int(N)
    if N < 1:
        raise ValueError("split_children: N must be at least 1, got %d" % N)
    if split_rows.dtype != torch.int32 or split_rows.device != dev or not split_rows.is_contiguous() or split_rows.numel() < S or S > P:
        raise RuntimeError("split_children: split_rows must hold the %d split rows as contiguous int32 on %s" % (S, dev))
    isotropic = getattr(pc, "isotropic", False)
    with torch.no_grad():
        scaling = pc.get_scaling
        stds = scaling.expand(P, 3) if scaling.dim() == 2 and scaling.size(1) == 1 else scaling     # (a get_scaling of one column)
        xyz_c, rot, stds = xyz.detach().contiguous(), pc._rotation.detach().contiguous(), stds.detach().contiguous()
        for t, shape, name in ((xyz_c, (P, 3), "get_xyz"), (rot, (P, 4), "_rotation"), (stds, (P, 3), "get_scaling")):
            if t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != dev:
                raise RuntimeError("split_children: %s must be float32 %s on %s, got %s %s on %s"
                                   % (name, shape, dev, t.dtype, tuple(t.shape), t.device))
        z = torch.randn((N * S, 3), device=dev)
        new_xyz = torch.empty((N * S, 3), device=dev)
        ptr = lambda t: t.data_ptr() if t.numel() else None
        with _lib.on_device(dev):
            _lib.check(lib.gft_split_children(_lib.raw_stream(dev), P, S, N, ptr(split_rows), ptr(xyz_c), ptr(rot), ptr(stds), ptr(z),
                                              ptr(new_xyz)))
        if isotropic:
            sel = pc.scaling_activation(_remap(lib, dev, S, split_rows, pc._scaling))
        else:
            sel = _remap(lib, dev, S, split_rows, scaling)
        new_scaling = pc.scaling_inverse_activation(sel.repeat(N, 1) / (0.8 * N))
        child_max_scaling = pc.scaling_activation(new_scaling).max(dim=1).values.contiguous()
    return new_xyz, new_scaling, child_max_scaling


def densify_and_split(pc, grads, grad_threshold, scene_extent, N=2, children="torch"):
    """``GaussianModel.densify_and_split`` (gaussian_model.py:571-601): large Gaussians with a large gradient are
    replaced by N smaller ones sampled inside them (torch.normal: torch's generator decides the samples).
    ``children="kernel"``: positions and scalings of the children from :func:`split_children` (same samples, its own
    rounding of the rotation) instead of the reference's torch statements."""
    kernel = _children_route(children, "densify_and_split")
    n_init = pc.get_xyz.shape[0]
    dev = pc.get_xyz.device
    padded = torch.zeros((n_init,), device=dev)
    padded[:grads.shape[0]] = grads.squeeze()
    mask = torch.where(padded >= grad_threshold, True, False)
    mask = torch.logical_and(mask, torch.max(pc.get_scaling, dim=1).values > pc.percent_dense * scene_extent)
    sel = RowSelection(mask)
    rotation_sel = sel.take(pc._rotation)
    if kernel:
        new_xyz, new_scaling, _ = split_children(pc, sel.rows(), sel.count, N)
        new = {"xyz": new_xyz, "scaling": new_scaling}
    else:
        scaling_sel = sel.take(pc.get_scaling)
        stds = scaling_sel.repeat(N, 1)
        means = torch.zeros((stds.size(0), 3), device=dev)
        samples = torch.normal(mean=means, std=stds)
        rots = _rotation_matrices(rotation_sel).repeat(N, 1, 1)
        new = {"xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + sel.take(pc.get_xyz).repeat(N, 1)}
        if getattr(pc, "isotropic", False):
            new["scaling"] = pc.scaling_inverse_activation(pc.scaling_activation(sel.take(pc._scaling)).repeat(N, 1) / (0.8 * N))
        else:
            new["scaling"] = pc.scaling_inverse_activation(scaling_sel.repeat(N, 1) / (0.8 * N))
    new["rotation"] = rotation_sel.repeat(N, 1)
    for name in ("f_dc_color", "f_rest_color", "phase_f_dc", "phase_f_rest", "amp_f_dc", "amp_f_rest"):
        new[name] = sel.take(getattr(pc, GROUP_ATTR[name])).repeat(N, 1, 1)
    new["opacity"] = sel.take(pc._opacity).repeat(N, 1)
    new["f_seg_color"] = sel.take(pc._features_seg_color).repeat(N, 1)
    densification_postfix(pc, new)
    prune_filter = torch.cat((mask, torch.zeros(N * sel.count, device=dev, dtype=torch.bool)))
    prune_points(pc, prune_filter)


def densify_and_prune(pc, max_grad, min_opacity, extent, max_screen_size=20):
    """``GaussianModel.densify_and_prune`` (gaussian_model.py:624-640)."""
    grads = pc.xyz_gradient_accum / pc.denom
    grads[grads.isnan()] = 0.0
    densify_and_clone(pc, grads, max_grad, extent)
    densify_and_split(pc, grads, max_grad, extent)
    prune_mask = (pc.get_opacity < min_opacity).squeeze()
    if max_screen_size:
        big_points_vs = pc.max_radii2D > max_screen_size
        big_points_ws = pc.get_scaling.max(dim=1).values > 0.05 * extent
        small_points_ws = pc.get_scaling.max(dim=1).values < 0.001 * extent
        prune_mask = torch.logical_or(torch.logical_or(torch.logical_or(prune_mask, big_points_vs), big_points_ws), small_points_ws)
    prune_points(pc, prune_mask)


def prune(pc, min_opacity):
    """``GaussianModel.prune`` (gaussian_model.py:642-646)."""
    prune_points(pc, (pc.get_opacity < min_opacity).squeeze())


# ---- the whole event as one plan and one pass over every tensor ----------------------------------------------------------
def _remap(lib, dev, n_out, row_map, src, extra=None):
    """``gft_rows_remap``: a new tensor of ``n_out`` rows, row r = row ``row_map[r]`` of ``src``, row ``row_map[r] -
    src.size(0)`` of ``extra``, or zeros for -1."""
    src = src.detach().contiguous()
    rows = src.size(0)
    row_bytes = (src.numel() // rows if rows else int(torch.Size(src.shape[1:]).numel())) * src.element_size()
    if row_bytes % 4:
        raise RuntimeError("gftorf_amd.densify: rows of %d bytes (%s %s) are not a multiple of 4 bytes"
                           % (row_bytes, src.dtype, tuple(src.shape[1:])))
    if extra is not None:
        extra = extra.detach().contiguous()
        if extra.dtype != src.dtype or tuple(extra.shape[1:]) != tuple(src.shape[1:]):
            raise RuntimeError("gftorf_amd.densify: the extra rows are %s %s, the tensor's %s %s"
                               % (extra.dtype, tuple(extra.shape[1:]), src.dtype, tuple(src.shape[1:])))
    dst = torch.empty((n_out,) + tuple(src.shape[1:]), device=dev, dtype=src.dtype)
    if n_out and row_bytes:
        with _lib.on_device(dev):
            _lib.check(lib.gft_rows_remap(_lib.raw_stream(dev), n_out, row_map.data_ptr(), src.data_ptr() if rows else None, rows,
                                          extra.data_ptr() if extra is not None and extra.numel() else None, dst.data_ptr(),
                                          row_bytes))
    return dst


class DensifyResult:
    """What :func:`densify_and_prune_fused` did, and the means to carry further per-Gaussian tensors across it.

    ``P_before`` / ``P``: rows before and after; ``cloned`` / ``split``: rows selected for either; ``pruned``: rows the final
    prune removed beside the split originals (originals, clones and children).  Per row of the new model, on the device:
    ``source_row`` (int32: the original row it is, or was copied or split from), ``kind`` (uint8: 0 kept original, 1 clone,
    2 child), ``child`` (int32: the child's index k * split + j, -1 otherwise) and ``motion_mask`` (bool,
    ``pc.get_motion_mask`` of the new model; None for a model without seg colours).  After a call that went through the
    composite (``max_grad <= 0``) only the row counts are known: the per-row tensors and the other counts are None."""

    def __init__(self, P_before, P, cloned=None, split=None, pruned=None, source_row=None, kind=None, child=None, map_state=None,
                 motion_mask=None, motion_rank=None, dynamic=None):
        self.P_before, self.P, self.cloned, self.split, self.pruned = P_before, P, cloned, split, pruned
        self.source_row, self.kind, self.child, self.motion_mask = source_row, kind, child, motion_mask
        self._map_state, self._motion_rank, self._dynamic = map_state, motion_rank, dynamic

    def remap(self, t, new_rows="zero"):
        """A tensor with one row per Gaussian of the model BEFORE the event, carried across it (``gft_rows_remap``, one
        launch): kept originals keep their row; clones and children get zeros (``"zero"``, as the Adam moments do) or their
        parent's row (``"parent"``, as the parameters do)."""
        if new_rows not in ("zero", "parent"):
            raise ValueError("DensifyResult.remap: new_rows must be 'zero' or 'parent', got %r" % (new_rows,))
        if self.source_row is None:
            raise RuntimeError("DensifyResult.remap: this event went through the composite (max_grad <= 0) and has no row map")
        _dev_check(t, "DensifyResult.remap")
        if t.size(0) != self.P_before or t.device != self.source_row.device:
            raise RuntimeError("DensifyResult.remap: tensor with %d rows on %s, the model had %d rows on %s"
                               % (t.size(0), t.device, self.P_before, self.source_row.device))
        return _remap(_lib.load(), t.device, self.P, self.source_row if new_rows == "parent" else self._map_state, t)

    def deform_query(self):
        """The ``DeformQuery`` of the new model's motion mask, from the rank the layout pass already formed: no further
        ranking, no host read."""
        from .query import DeformQuery
        if self.motion_mask is None:
            raise RuntimeError("DensifyResult.deform_query: the model has no seg colours, so no motion mask")
        return DeformQuery.from_rank(self.motion_mask, self._motion_rank, self._dynamic)


def _children_torch(pc, lib, scaling, split_rows, n_split, N):
    """``densify_and_split``'s own statements (gaussian_model.py:577-585) on the ``n_split`` rows ``split_rows``."""
    dev = scaling.device
    with torch.no_grad():
        take = lambda t: _remap(lib, dev, n_split, split_rows, t)
        scaling_sel = take(scaling)
        stds = scaling_sel.repeat(N, 1)
        means = torch.zeros((stds.size(0), 3), device=dev)
        samples = torch.normal(mean=means, std=stds)
        rots = _rotation_matrices(take(pc._rotation)).repeat(N, 1, 1)
        new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + take(pc.get_xyz).repeat(N, 1)
        if getattr(pc, "isotropic", False):
            new_scaling = pc.scaling_inverse_activation(pc.scaling_activation(take(pc._scaling)).repeat(N, 1) / (0.8 * N))
        else:
            new_scaling = pc.scaling_inverse_activation(scaling_sel.repeat(N, 1) / (0.8 * N))
        child_max_scaling = pc.scaling_activation(new_scaling).max(dim=1).values.contiguous()
    return new_xyz, new_scaling, child_max_scaling


def _f32_positive(x):
    """``x`` rounded to float32, as a kernel argument and torch's comparison with a float32 tensor take it, is > 0."""
    return C.c_float(float(x)).value > 0.0


def densify_and_prune_fused(pc, max_grad, min_opacity, extent, max_screen_size=20, N=2, children="torch"):
    """``GaussianModel.densify_and_prune`` (gaussian_model.py:624-640) as one plan and one pass over every tensor: leaves
    ``pc`` and its optimizer exactly as :func:`densify_and_prune` does under the same torch generator state (every
    parameter, both moments of every group, ``step``, the order of ``param_groups``, the three statistics), and returns a
    :class:`DensifyResult`.  ``N``: children per split Gaussian (the reference's ``densify_and_split`` default, 2).

    The event is a function of per-row quantities.  ``gft_densify_classify`` marks the cloned and the split rows (the
    reference's two selections over ``grads``, ``torch.norm(grads, dim=-1)`` and ``get_scaling.max(1)``, which torch forms,
    against thresholds passed as float32, as torch compares them); the children's ``xyz`` and ``scaling`` are the
    reference's own torch statements on the S split rows (``torch.normal`` with the same shapes in the same order: same
    generator consumption, same bits); ``gft_densify_layout`` applies the final prune to the P + C + N * S virtual rows
    (originals, clones, children) and says where each survivor lands; ``gft_rows_remap`` then writes each new tensor in one
    launch.  By construction:

    * two blocking host reads per call: the numbers of cloned and split rows (``torch.normal`` needs the shape), then the
      new row count together with the number of dynamic rows;
    * every parameter and moment tensor is read once and written once (the S split rows of ``xyz``, ``rotation`` and the
      activated scaling are read once more, for the children);
    * the moments' new rows are written as zeros by the kernel that moves the kept ones: no ``torch.zeros`` plus copy;
    * the statistics are three ``zeros(P')``.

    A clone is never split because its padded gradient is 0, which needs ``max_grad > 0`` (as float32): for ``max_grad <=
    0`` the call goes through :func:`densify_and_prune` (``N`` must then be 2) and the result carries row counts only.

    ``children="kernel"`` (opt-in; the default ``"torch"`` is the route described above, bit for bit): the children's ``xyz``
    comes from one launch of ``gft_split_children`` (:func:`split_children`) instead of two of the three gathers, the ~45
    eager launches of the rotation matrices, ``torch.normal`` and the ``torch.bmm`` over N * S 3x3 matrices; the scaling
    statements stay torch's.  Same generator consumption, same samples, same R, every tensor but the children's ``xyz`` rows
    bit for bit what the default gives; those rows carry the kernel's own rounding of the three products (an ascending chain
    of fused multiply-adds) where the default carries ``torch.bmm``'s, both within the same bound of the exact value.  The
    composite route of ``max_grad <= 0`` ignores the keyword, as it ignores the plan."""
    kernel = _children_route(children, "densify_and_prune_fused")
    xyz = pc.get_xyz
    _dev_check(xyz, "densify_and_prune_fused")
    lib = _lib.load()
    dev = xyz.device
    P = int(xyz.shape[0])
    N = int(N)
    if N < 1:
        raise ValueError("densify_and_prune_fused: N must be at least 1, got %d" % N)
    if not _f32_positive(max_grad):
        if N != 2:
            raise ValueError("densify_and_prune_fused: max_grad <= 0 goes through densify_and_prune, which splits into 2 (N = %d)" % N)
        densify_and_prune(pc, max_grad, min_opacity, extent, max_screen_size)
        return DensifyResult(P, int(pc.get_xyz.shape[0]))
    with torch.no_grad():
        grads = pc.xyz_gradient_accum / pc.denom
        grads[grads.isnan()] = 0.0
        grad_norm = torch.norm(grads, dim=-1).contiguous()
        grads = grads.reshape(-1).contiguous()
        scaling = pc.get_scaling
        max_scaling = torch.max(scaling, dim=1).values.contiguous()
        opacity = pc.get_opacity.reshape(-1).contiguous()
    for t, name in ((grad_norm, "xyz_gradient_accum / denom"), (max_scaling, "get_scaling"), (opacity, "get_opacity")):
        if t.dtype != torch.float32 or t.numel() != P or t.device != dev:
            raise RuntimeError("densify_and_prune_fused: %s must give one float32 value per Gaussian (%d) on %s" % (name, P, dev))
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    stream = _lib.raw_stream(dev)
    counts = (C.c_int64 * 2)()

    # plan, first half: which rows are cloned, which are split (host read 1: C and S)
    row_class = torch.empty((P,), device=dev, dtype=torch.uint8)
    clone_rows = torch.empty((P,), device=dev, dtype=torch.int32)
    split_rows = torch.empty((P,), device=dev, dtype=torch.int32)
    scratch = torch.empty((lib.gft_densify_plan_scratch_bytes(P),), device=dev, dtype=torch.uint8)
    with _lib.on_device(dev):
        _lib.check(lib.gft_densify_classify(stream, P, ptr(grad_norm), ptr(grads), ptr(max_scaling), float(max_grad),
                                            float(pc.percent_dense * extent), ptr(row_class), ptr(clone_rows), ptr(split_rows),
                                            ptr(scratch), counts))
    n_clone, n_split = int(counts[0]), int(counts[1])

    # the children's positions and scalings: one kernel, or densify_and_split's statements on the split rows
    if kernel:
        new_xyz, new_scaling, child_max_scaling = split_children(pc, split_rows, n_split, N)
    else:
        new_xyz, new_scaling, child_max_scaling = _children_torch(pc, lib, scaling, split_rows, n_split, N)
    extra = {"xyz": new_xyz, "scaling": new_scaling}

    # plan, second half: the final prune over the virtual rows and every survivor's place (host read 2: P' and n')
    V = P + n_clone + N * n_split
    seg = getattr(pc, "_features_seg_color", None)
    if seg is not None and (seg.dim() != 2 or seg.size(0) != P or seg.dtype != torch.float32 or seg.size(1) < 1):
        seg = None
    seg_c = seg.detach().contiguous() if seg is not None else None
    i32 = lambda: torch.empty((V,), device=dev, dtype=torch.int32)
    u8 = lambda: torch.empty((V,), device=dev, dtype=torch.uint8)
    source_row, child, map_new, map_state, kind = i32(), i32(), i32(), i32(), u8()
    motion_mask, motion_rank = (u8(), i32()) if seg_c is not None else (None, None)
    scratch = torch.empty((lib.gft_densify_plan_scratch_bytes(V),), device=dev, dtype=torch.uint8)
    use_size = bool(max_screen_size)
    with _lib.on_device(dev):
        _lib.check(lib.gft_densify_layout(
            stream, P, n_clone, n_split, N, ptr(row_class), ptr(clone_rows), ptr(split_rows), ptr(opacity), ptr(max_scaling),
            ptr(child_max_scaling), float(min_opacity), int(use_size),
            int(use_size and C.c_float(0.0).value > C.c_float(float(max_screen_size)).value),      # max_radii2D is all zeros there
            float(0.05 * extent) if use_size else 0.0, float(0.001 * extent) if use_size else 0.0, ptr(seg_c),
            int(seg_c.size(1)) if seg_c is not None else 0, ptr(source_row), ptr(kind), ptr(child), ptr(map_new), ptr(map_state),
            ptr(motion_mask), ptr(motion_rank), ptr(scratch), counts))
    P_new, n_dynamic = int(counts[0]), int(counts[1])
    source_row, child, map_new, map_state, kind = (t[:P_new] for t in (source_row, child, map_new, map_state, kind))

    # one launch per tensor: parameters by their source row (xyz and scaling: children from their new values), moments by
    # the map whose new rows are -1
    tensors = {}
    for group in pc.optimizer.param_groups:
        name = group["name"]
        if name in _SKIP:
            continue
        assert len(group["params"]) == 1
        p = group["params"][0]
        state = pc.optimizer.state.get(p, None)
        if name in extra:
            moved = _remap(lib, dev, P_new, map_new, p, extra[name])
        else:
            moved = _remap(lib, dev, P_new, source_row, p)
        new_p = nn.Parameter(moved.requires_grad_(True))
        if state is not None:
            state["exp_avg"] = _remap(lib, dev, P_new, map_state, state["exp_avg"])
            state["exp_avg_sq"] = _remap(lib, dev, P_new, map_state, state["exp_avg_sq"])
            del pc.optimizer.state[p]
            group["params"][0] = new_p
            pc.optimizer.state[new_p] = state
        else:
            group["params"][0] = new_p
        tensors[name] = new_p
    _adopt(pc, tensors)
    pc.xyz_gradient_accum = torch.zeros((P_new, 1), device=dev)
    pc.denom = torch.zeros((P_new, 1), device=dev)
    pc.max_radii2D = torch.zeros((P_new,), device=dev)
    return DensifyResult(P, P_new, cloned=n_clone, split=n_split, pruned=V - n_split - P_new, source_row=source_row, kind=kind,
                         child=child, map_state=map_state,
                         motion_mask=motion_mask[:P_new].view(torch.bool) if motion_mask is not None else None,
                         motion_rank=motion_rank[:P_new] if motion_rank is not None else None,
                         dynamic=n_dynamic if motion_mask is not None else None)
