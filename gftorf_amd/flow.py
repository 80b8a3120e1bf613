"""The F-ToRF scene-flow term of the training loss as one launch forward and one backward (``csrc/k_flow.hip``,
``include/gftorf_flow.h``): ``train.py:243-261`` unprojects the rendered distance (``scene/torf_utils.py``
``distance_to_points3d``), projects it into the ToF camera (``project_points``), adds each rendered 3-D flow and projects
again (``project_flow``), and takes the mean of the squared difference to the ground-truth 2-D flow.  In eager PyTorch that
is ~100 small launches forward and backward, and its ``torch.inverse`` of the view matrix synchronises with the host.  Here
every camera matrix is read on the device (the inverse is formed inside each launch), nothing is read back to the host and
nothing issues a memset, so ``flow_loss`` and its backward can be captured in a graph.

The reference's semantics are kept as they are: the unprojection uses the colour camera's intrinsics and inverts
``world_view_transform`` as stored, the projection uses ``K_tof`` and ``world_view_transform_tof.T``, the divide is
``xy / (z + 1e-7)``.  Gradients flow to the 3-D flows only (the reference detaches the depth; the ground truth and the
cameras are data).  There is no CPU path.

The two ``render_flow`` calls that feed the term (``gaussian_renderer/__init__.py:141-204``) draw the same detached geometry
from the same ToF camera with two ``colors_precomp``: ``render_flow_pair`` / ``render_flows`` draw the frame once, blend the
second flow over it (``csrc/k_features.hip``, ``include/gftorf_features.h``) and return the gradient of both flows from one
walk over the frame, with no host read.
"""
import ctypes as C
import math

import torch

from . import _args, _lib
from . import reproducible as _reproducible
from ._args import ptr as _ptr


def _check(items):
    """items: (tensor, name, shape, grad_ok); a None in `shape` is any size.  Shapes and gradients are checked before
    devices, then every tensor must be on the first one's HIP device.  Returns the tensors as float32, contiguous."""
    for t, name, shape, grad_ok in items:
        if not isinstance(t, torch.Tensor):
            raise TypeError("gftorf_amd.flow: %s must be a tensor, got %s" % (name, type(t).__name__))
        if t.dim() != len(shape) or any(w is not None and int(n) != w for n, w in zip(t.shape, shape)):
            want = "[%s]" % ", ".join("HW"[i - 1] if w is None else str(w) for i, w in enumerate(shape))      # [C, H, W]
            raise RuntimeError("gftorf_amd.flow: %s must be %s, got %s" % (name, want, list(t.shape)))
        if t.requires_grad and not grad_ok:
            raise NotImplementedError("gftorf_amd.flow: gradients flow to the 3-D flows only; %s requires grad (detach it, "
                                      "as train.py detaches the depth)" % name)
    _args.devices("gftorf_amd.flow", "flow", items)
    return [t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous() for t, _, _, _ in items]


def _hw(t):
    return (int(t.shape[-2]), int(t.shape[-1])) if isinstance(t, torch.Tensor) and t.dim() >= 2 else (None, None)


class _SceneFlowL2(torch.autograd.Function):
    """(forward_flow_l2, backward_flow_l2): one launch + one column sum forward, one launch backward."""

    @staticmethod
    def forward(ctx, depth, K, w2v, K_tof, w2v_tof, f_fwd, gt_fwd, f_bwd, gt_bwd):
        lib = _lib.load()
        H, W = int(depth.shape[1]), int(depth.shape[2])
        blocks = int(lib.gft_flow_loss_blocks(H, W))
        partials = torch.empty((blocks, 2), device=depth.device, dtype=torch.float32)
        scale = 1.0 / (2.0 * H * W)
        with _lib.on_device(depth.device):
            _lib.check(lib.gft_flow_loss_forward(_lib.raw_stream(depth.device), H, W, depth.data_ptr(), K.data_ptr(),
                                                 w2v.data_ptr(), K_tof.data_ptr(), w2v_tof.data_ptr(), _ptr(f_fwd), _ptr(gt_fwd),
                                                 _ptr(f_bwd), _ptr(gt_bwd), scale, partials.data_ptr()))
        sums = partials.sum(0)
        ctx.sizes = (H, W, scale)
        ctx.save_for_backward(depth, K, w2v, K_tof, w2v_tof, f_fwd, gt_fwd, f_bwd, gt_bwd)
        ctx.set_materialize_grads(False)
        return sums[0], sums[1]

    @staticmethod
    def backward(ctx, g_fwd, g_bwd):
        lib = _lib.load()
        depth, K, w2v, K_tof, w2v_tof, f_fwd, gt_fwd, f_bwd, gt_bwd = ctx.saved_tensors
        H, W, scale = ctx.sizes
        grad_fwd = torch.empty_like(f_fwd) if f_fwd is not None and ctx.needs_input_grad[5] else None
        grad_bwd = torch.empty_like(f_bwd) if f_bwd is not None and ctx.needs_input_grad[7] else None
        if grad_fwd is None and grad_bwd is None:
            return (None,) * 9
        up = lambda g: None if g is None else g.detach().float()        # a 0-dim gradient: one float at data_ptr()
        gf, gb = up(g_fwd), up(g_bwd)
        with _lib.on_device(depth.device):
            _lib.check(lib.gft_flow_loss_backward(_lib.raw_stream(depth.device), H, W, depth.data_ptr(), K.data_ptr(),
                                                  w2v.data_ptr(), K_tof.data_ptr(), w2v_tof.data_ptr(), _ptr(f_fwd),
                                                  _ptr(gt_fwd), _ptr(f_bwd), _ptr(gt_bwd), _ptr(gf), _ptr(gb), scale,
                                                  _ptr(grad_fwd), _ptr(grad_bwd)))
        return None, None, None, None, None, grad_fwd, None, grad_bwd, None


def scene_flow_l2(depth, K, w2v, K_tof, w2v_tof, flow3d_fwd=None, gt_fwd=None, flow3d_bwd=None, gt_bwd=None):
    """``(forward_flow_l2, backward_flow_l2)`` of ``train.py:243-259`` from tensors alone, two 0-dim tensors of one autograd
    node: ``mean((project_flow(p2, p3, flow3d) - gt) ** 2)`` per direction, with ``p3 = distance_to_points3d(depth)`` and
    ``p2 = project_points(p3)``.  ``depth`` [1, H, W] (the rendered distance; no gradient), ``K`` / ``K_tof`` [3, 3],
    ``w2v`` / ``w2v_tof`` [4, 4] (the cameras' ``world_view_transform`` / ``world_view_transform_tof`` as stored),
    ``flow3d_*`` [3, H, W] (gradients flow here), ``gt_*`` [2, H, W].  A direction without its flow3d or its gt is 0.
    Nothing is read back to the host: with static tensors the call and its backward can be captured in a graph."""
    H, W = _hw(depth)
    items = [(depth, "depth", (1, None, None), False), (K, "K", (3, 3), False), (w2v, "world_view_transform", (4, 4), False),
             (K_tof, "K_tof", (3, 3), False), (w2v_tof, "world_view_transform_tof", (4, 4), False)]
    present = []
    for name, f, gt in (("forward", flow3d_fwd, gt_fwd), ("backward", flow3d_bwd, gt_bwd)):
        present.append(f is not None and gt is not None)
        if present[-1]:
            items += [(f, "flow3d_" + name, (3, H, W), True), (gt, "gt_" + name, (2, H, W), False)]
    t = iter(_check(items))
    d, cams = next(t), [next(t) for _ in range(4)]
    dirs = []
    for p in present:
        dirs += [next(t), next(t)] if p else [None, None]
    return _SceneFlowL2.apply(d, *cams, *dirs)


def flow_loss(depth, cam, flow3d_forward=None, flow3d_backward=None):
    """``(forward_flow_l2, backward_flow_l2)`` exactly as ``train.py:236-259`` builds them, from one autograd node: the
    caller writes ``loss += opt.lambda_flow * (f + b)`` and can still log each term.  ``depth`` is
    ``render_pkg["render_depth"].detach()``; ``cam`` anything with the reference ``ToFCamera``'s ``K``, ``K_tof``,
    ``world_view_transform``, ``world_view_transform_tof``, ``forward_flow`` and ``backward_flow``; ``flow3d_*`` the
    ``render_flow`` outputs.  A direction whose flow3d or ground truth is None gives 0."""
    return scene_flow_l2(depth, cam.K, cam.world_view_transform, cam.K_tof, cam.world_view_transform_tof,
                         flow3d_forward, getattr(cam, "forward_flow", None), flow3d_backward, getattr(cam, "backward_flow", None))


def distance_to_points3d(distance_map, viewpoint_cam):
    """Drop-in for ``scene.torf_utils.distance_to_points3d`` (no gradient to the distance)."""
    d, K, w2v = _check([(distance_map, "distance_map", (1, None, None), False), (viewpoint_cam.K, "K", (3, 3), False),
                        (viewpoint_cam.world_view_transform, "world_view_transform", (4, 4), False)])
    dev, (H, W) = d.device, _hw(d)
    out = torch.empty((3, H, W), device=dev, dtype=torch.float32)
    lib = _lib.load()
    with _lib.on_device(dev):
        _lib.check(lib.gft_flow_points(_lib.raw_stream(dev), H, W, d.data_ptr(), K.data_ptr(), w2v.data_ptr(), None, None,
                                       out.data_ptr(), None))
    return out


def project_points(points3d, viewpoint_cam):
    """Drop-in for ``scene.torf_utils.project_points`` (no gradient to the points)."""
    p3, K_tof, w2v_tof = _check([(points3d, "points3d", (3, None, None), False), (viewpoint_cam.K_tof, "K_tof", (3, 3), False),
                                 (viewpoint_cam.world_view_transform_tof, "world_view_transform_tof", (4, 4), False)])
    dev, (H, W) = p3.device, _hw(p3)
    out = torch.empty((2, H, W), device=dev, dtype=torch.float32)
    lib = _lib.load()
    with _lib.on_device(dev):
        _lib.check(lib.gft_flow_project(_lib.raw_stream(dev), H, W, K_tof.data_ptr(), w2v_tof.data_ptr(), p3.data_ptr(), None,
                                        None, out.data_ptr()))
    return out


class _ProjectFlow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p2, p3, flow3d, K_tof, w2v_tof):
        lib = _lib.load()
        H, W = int(p3.shape[1]), int(p3.shape[2])
        out = torch.empty((2, H, W), device=p3.device, dtype=torch.float32)
        with _lib.on_device(p3.device):
            _lib.check(lib.gft_flow_project(_lib.raw_stream(p3.device), H, W, K_tof.data_ptr(), w2v_tof.data_ptr(),
                                            p3.data_ptr(), flow3d.data_ptr(), p2.data_ptr(), out.data_ptr()))
        ctx.save_for_backward(p3, flow3d, K_tof, w2v_tof)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        p3, flow3d, K_tof, w2v_tof = ctx.saved_tensors
        H, W = int(p3.shape[1]), int(p3.shape[2])
        g = g.detach().float().contiguous()
        grad = torch.empty_like(flow3d)
        with _lib.on_device(p3.device):
            _lib.check(lib.gft_flow_project_backward(_lib.raw_stream(p3.device), H, W, K_tof.data_ptr(), w2v_tof.data_ptr(),
                                                     p3.data_ptr(), flow3d.data_ptr(), g.data_ptr(), grad.data_ptr()))
        return None, None, grad, None, None


def project_flow(points2d_curr, points3d_curr, flow3d, viewpoint_cam):
    """Drop-in for ``scene.torf_utils.project_flow``: ``project_points(points3d_curr + flow3d) - points2d_curr``,
    differentiable with respect to ``flow3d`` (the current points are data, as in ``train.py``)."""
    H, W = _hw(points3d_curr)
    p3, p2, f, K_tof, w2v_tof = _check([(points3d_curr, "points3d_curr", (3, None, None), False),
                                        (points2d_curr, "points2d_curr", (2, H, W), False), (flow3d, "flow3d", (3, H, W), True),
                                        (viewpoint_cam.K_tof, "K_tof", (3, 3), False),
                                        (viewpoint_cam.world_view_transform_tof, "world_view_transform_tof", (4, 4), False)])
    return _ProjectFlow.apply(p2, p3, f, K_tof, w2v_tof)


# ---- the two scene-flow renders (gaussian_renderer/__init__.py render_flow, train.py:249,256) ---------------------------

class _RenderFlows(torch.autograd.Function):
    """One rasterizer forward with ``colors_precomp = flow_a`` (its image is what that call returns), the second flow blended
    over the same frame by ``k_feat_fwd<3>``; backward: one ``k_feat_bwd`` over both images (``include/gftorf_features.h``) --
    in the reproducible mode (``gftorf_amd.reproducible``) ``k_feat_bwd_det`` and the fixed-order sum instead."""

    @staticmethod
    def forward(ctx, s, means3D, opacities, scales, rotations, flow_a, flow_b):
        from . import api
        lib = _lib.load()
        dev = means3D.device
        P = int(means3D.shape[0])
        H, W = int(s.image_height), int(s.image_width)
        r = api.native_forward(s, means3D, None, None, flow_a, None, opacities, scales, rotations, None, 0.0, 0.0, False, False,
                               nowait=True)
        bg_c, bsc, bsy, bsx = r["bg"]
        cfg = api._make_config(s, P, 0, 0, H, W, 0.0, 0.0, (bsc, bsy, bsx), False)
        geom, img, binning = r["geom"], r["img"], r["binning"]
        frame = (geom.data_ptr(), img.data_ptr(), binning.data_ptr() if binning.numel() else None, int(r["cap"]))
        image_b = None
        if flow_b is not None:
            image_b = torch.empty((3, H, W), device=dev, dtype=torch.float32)
            with _lib.on_device(dev):
                _lib.check(lib.gft_render_features(_lib.raw_stream(dev), C.byref(cfg), *frame, 3, flow_b.data_ptr(),
                                                   bg_c.data_ptr(), image_b.data_ptr()))
        ctx.frame = (cfg, frame)
        ctx.save_for_backward(geom, img, binning)
        ctx.set_materialize_grads(False)
        return r["outputs"][0], image_b

    @staticmethod
    def backward(ctx, g_a, g_b):
        lib = _lib.load()
        geom = ctx.saved_tensors[0]
        cfg, frame = ctx.frame
        want = [g is not None and ctx.needs_input_grad[5 + k] for k, g in enumerate((g_a, g_b))]
        if not any(want):
            return (None,) * 7
        # one walk serves both flows: their weights alpha_i T_i are the same
        g = torch.cat((g_a, g_b)) if all(want) else (g_a if want[0] else g_b)
        g = g.detach().float().contiguous()
        n = int(g.shape[0])
        dev = geom.device
        grad = torch.empty((cfg.P, n), device=dev, dtype=torch.float32)
        stream_args = (C.byref(cfg), *frame, n, g.data_ptr())
        with _lib.on_device(dev):
            if _reproducible.is_reproducible():
                # the fixed-order backward (read per call: a captured graph keeps the mode it was captured under): every
                # (entry, quadrant) row is stored and the rows are added in one order (include/gftorf_detsum.h)
                cap, W, H = frame[3], int(cfg.W), int(cfg.H)
                partials = torch.empty((lib.gft_feature_partials_bytes(cap, W, H) // 4,), device=dev, dtype=torch.float32)
                index = None
                if _reproducible.det_reduce() == "grid":
                    index = torch.empty((lib.gft_detsum_index_bytes(cfg.P, cap) // 4,), device=dev, dtype=torch.int32)
                _lib.check(lib.gft_render_features_backward_det(_lib.raw_stream(dev), *stream_args, _ptr(index),
                                                                partials.data_ptr() if cap else None, grad.data_ptr()))
            else:
                acc = torch.empty((cfg.P, 8), device=dev, dtype=torch.float32)
                _lib.check(lib.gft_render_features_backward(_lib.raw_stream(dev), *stream_args, acc.data_ptr(), grad.data_ptr()))
        if all(want):
            return None, None, None, None, None, grad[:, :3], grad[:, 3:]
        return (None, None, None, None, None) + ((grad, None) if want[0] else (None, grad))


def render_flows(raster_settings, means3D, opacities, scales, rotations, flow_a, flow_b=None):
    """``(image_a, image_b)``: the ``[3, H, W]`` images ``GaussianRasterizer(raster_settings)(colors_precomp=flow_a)`` and
    ``(colors_precomp=flow_b)`` return on the same geometry, from one rasterizer forward (``image_a`` is its colour output)
    and one blend of ``flow_b`` over the frame it drew; ``image_b`` is None without ``flow_b``.  Gradients flow to the flows
    only -- one walk over the frame for both -- so the geometry (``means3D`` [P, 3], ``opacities`` [P, 1], ``scales`` [P, 3],
    ``rotations`` [P, 4]) must not require grad.  Nothing is read back to the host once a frame of the shape has been drawn:
    the binning buffer is sized from earlier frames, as with ``api.no_host_read``, so with static
    tensors the call and its backward can be captured in a graph.  The price is that contract's: a frame with more
    instances than that buffer holds is not drawn -- both images are undefined and so are the gradients -- and the next call
    of the shape raises (and enlarges the buffer) instead of re-rendering as ``GaussianRasterizer`` does."""
    t = means3D if isinstance(means3D, torch.Tensor) else None
    P = int(t.shape[0]) if t is not None and t.dim() == 2 else None
    op_shape = (P, 1) if isinstance(opacities, torch.Tensor) and opacities.dim() == 2 else (P,)
    items = [(means3D, "means3D", (P, 3), False), (opacities, "opacities", op_shape, False), (scales, "scales", (P, 3), False),
             (rotations, "rotations", (P, 4), False), (flow_a, "flow_a", (P, 3), True)]
    if flow_b is not None:
        items.append((flow_b, "flow_b", (P, 3), True))
    checked = _check(items)
    return _RenderFlows.apply(raster_settings, *checked[:5], checked[5] if flow_b is not None else None)


def _gather(t, rank):
    """[P, k]: row rank[i] of t in every row i, clamped to t's rows (any index is in bounds).  A t of no rows -- a model
    without a dynamic Gaussian -- gives zeros, still connected to t so that its gradient is the empty one the reference's
    empty masked assignment gives."""
    rows = int(t.shape[0])
    if rows == 0:
        return t.sum(0, keepdim=True).expand(int(rank.shape[0]), *t.shape[1:])
    return torch.index_select(t, 0, rank.clamp(0, rows - 1))


def _assemble_flow_inputs(pc, d_xyz, d_rot, flows, render_regions):
    """render_flow's masked assignments (gaussian_renderer/__init__.py:165-185) on the device, without their host reads: the
    detached geometry and each flow [N_dynamic, 3] in its dynamic rows, with the same values bit for bit -- the dynamic rows'
    arithmetic (xyz + d_xyz, rotation_activation(_rotation + d_rot)) runs on the same operands, only the copies are
    gathers.  Row k of a d_* tensor belongs to the k-th True of the motion mask; the row counts are not checked against the
    mask (the reference's assignment raises on a mismatch, which takes a host read)."""
    mask = pc.get_motion_mask
    P = int(mask.shape[0])
    st, dy = "static" in render_regions, "dynamic" in render_regions
    m = mask[:, None]
    rank = torch.cumsum(mask, 0) - 1
    pick = lambda s, d: torch.where(m, d if dy else 0.0, s if st else 0.0)
    dyn = lambda t: _gather(t, rank) if isinstance(t, torch.Tensor) else t
    with torch.no_grad():
        xyz = pc.get_xyz
        means3D = pick(xyz, xyz + dyn(d_xyz))
        opacity = pick(pc.get_opacity, pc.get_opacity)
        scales = pick(pc.get_scaling, pc.get_scaling)
        if isinstance(d_rot, torch.Tensor):
            # the dynamic rows' positions, so that rotation_activation sees the [N_dynamic, 4] rows the reference gives it
            n = int(d_rot.shape[0])
            pos = torch.zeros((n + 1,), device=mask.device, dtype=torch.int64)
            pos.scatter_(0, torch.where(mask, rank.clamp(max=n), n), torch.arange(P, device=mask.device))
            rot_dyn = dyn(pc.rotation_activation(torch.index_select(pc._rotation, 0, pos[:n]) + d_rot))
        else:
            rot_dyn = pc.rotation_activation(pc._rotation + d_rot)
        rotations = pick(pc.get_rotation, rot_dyn)
    full = [torch.where(m, dyn(f.float()), 0.0) if dy else torch.zeros((P, 3), device=mask.device) for f in flows]
    return means3D, opacity, scales, rotations, full


def render_flow_pair(viewpoint_cam, pc, d_xyz, d_rot, flow3d_forward, flow3d_backward, bg_color,
                     render_regions=("static", "dynamic")):
    """Drop-in for the two ``render_flow`` calls of an ftorf flow iteration (``gaussian_renderer/__init__.py:141-204``,
    ``train.py:249,256``): ``(forward_image, backward_image)``, each what ``render_flow(viewpoint_cam, pc, d_xyz, d_rot,
    flow3d, bg_color, render_regions)["render_flow"]`` returns for that flow, or None where the flow is None.  The ToF
    camera's settings are built as there, the detached geometry is assembled on the device with render_flow's values bit for
    bit, each flow ``[N_dynamic, 3]`` goes to its dynamic rows and its gradient comes back from them on the device: no host
    read (a ``depth_range`` held in device memory is the one exception, as in the reference), and the call can be captured.
    A model without dynamic Gaussians (``[0, k]`` deformations and flows) gives zero flow images, as the reference does.
    The binning buffer is sized from earlier frames of the shape, with :func:`render_flows`' consequence: a frame that
    outgrows it gives undefined images and the next call raises."""
    from .api import GaussianRasterizationSettings
    flows = [f for f in (flow3d_forward, flow3d_backward) if f is not None]
    if not flows:
        return None, None
    dr = viewpoint_cam.depth_range
    settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_cam.tof_image_height), image_width=int(viewpoint_cam.tof_image_width),
        tanfovx=math.tan(viewpoint_cam.FoVx_tof * 0.5), tanfovy=math.tan(viewpoint_cam.FoVy_tof * 0.5), bg=bg_color,
        scale_modifier=1.0, viewmatrix=viewpoint_cam.world_view_transform_tof, projmatrix=viewpoint_cam.full_proj_transform_tof,
        sh_degree=pc.active_sh_degree, campos=viewpoint_cam.camera_center_tof, prefiltered=False, debug=False,
        near_n=viewpoint_cam.znear, far_n=viewpoint_cam.zfar, depth_range=float(dr.item() if isinstance(dr, torch.Tensor) else dr),
        use_view_dependent_phase=pc.use_view_dependent_phase, optimize_phase_offset=False, optimize_dc_offset=False)
    means3D, opacity, scales, rotations, full = _assemble_flow_inputs(pc, d_xyz, d_rot, flows, render_regions)
    image_a, image_b = render_flows(settings, means3D, opacity, scales, rotations, *full)
    if flow3d_forward is None:
        return None, image_a
    return image_a, image_b
