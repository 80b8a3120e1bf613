"""A rendered view's display images on the device (``csrc/k_present.hip``, ``include/gftorf_present.h``).

The reference's render program (``render.py:105-189`` ``render_set``; ``:43-54`` ``save_input`` for the ground truth; the
``pipe.debug`` block of ``train.py:287-378``) copies every rasterizer output of a view to the host as float32 -- over a dozen
blocking ``.cpu()`` calls, about 130 bytes per pixel -- and forms the images it writes in numpy: ``phasor2real_img_amp``,
``normalize_im_gt``, ``normalize_im``, ``depth_from_tof``, ``depth / acc``, ``cm.magma(1 - (d - znear) / (zfar - znear))`` and
``to8b``.  Here:

``view_images(...)``  the uint8 images of one view (and the two derived float depths) as views into one device buffer, the
    sheet: at most two launches, no host read, no atomic, no memset; 27 bytes per pixel leave the device.
``PhasorRanges``  ``save_input``'s ``np.min`` / ``np.max`` over the whole ground-truth sequence as six floats on the device.
``ViewSheets``  pinned staging: ``submit`` enqueues ``view_images`` and the sheet's asynchronous copy, ``ready`` hands out the
    finished views as numpy arrays, so the host encodes view i while view i + 1 renders.
``zplanes(depth_range)``  the colour map's planes of ``render.py:54``.
``quad_images(phasor, ...)``  the four quad images of the track program (``render_ftorf_viz_traj.py:237-244``): ``tof_to_image``,
    matplotlib's ``seismic`` map, in one launch.
``flow_images(flow, gt_flow)``  the three optical-flow images of a direction in the ``pipe.debug`` block (``train.py:380-398``;
    ``csrc/k_flowviz.hip``, ``include/gftorf_flowviz.h``): ``flow_to_image`` of (rendered, target), (target, target) and (target
    - rendered, target) with the in-place edits the three calls share, in two launches; ``ViewSheets.submit_flow`` stages them.
``debug_images(phasor, gt_phasor, depth, ...)``  the rest of the ``pipe.debug`` block, the ToF branch of ``train.py:295-378``
    (``csrc/k_debugviz.hip``, ``include/gftorf_debugviz.h``): the depth maps, ``amp`` and the three scattering-phase products with
    their errors, the colour images, ``dd`` and the quad images with the one normalised quad error, 19 images of 43 bytes per
    pixel in one sheet, in two launches instead of about twenty blocking ``.cpu()`` copies; ``ViewSheets.submit_debug`` stages
    them.  The two ToF depths are inputs, as the loop has them, so every statement is an IEEE one and every byte the
    reference's (tests/test_present_debug.py).

The uint8 images equal the reference's bit for bit wherever its statements are IEEE operations; the one exception is
``arctan2`` (in ``depth_tof`` and in the flow images' hue), whose last bits may differ (see tests/test_present.py and
tests/test_present_flow.py).  Nothing here has a gradient and there is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _args, _lib
from ._args import ptr as _ptr

_TAG = "gftorf_amd.present"
IMAGES = tuple(name for name, _, _, _ in _lib.PRESENT_IMAGES)       # the keys, in the order the images lie in a sheet
_EVERY = (_lib.PRESENT_HAS_COLOR | _lib.PRESENT_HAS_PHASOR | _lib.PRESENT_HAS_QUAD | _lib.PRESENT_HAS_DEPTH | _lib.PRESENT_HAS_ACC |
          _lib.PRESENT_HAS_DD)


def zplanes(depth_range):
    """``(0.05 * r * 0.9, 0.55 * r * 1.1)`` evaluated in float32, as ``render.py:54`` does with the camera's 0-d float32
    ``depth_range``: (znear, zfar) as Python floats."""
    r = np.asarray(depth_range, dtype=np.float32).reshape(())
    return float(0.05 * r * 0.9), float(0.55 * r * 1.1)


def magma_table():
    """``to8b(cm.magma(.))`` as the kernel holds it: uint8 [257, 4], rows 0..255 the map's entries, row 256 a NaN's colour"""
    ptr = _lib.load().gft_present_magma()
    return np.ctypeslib.as_array(ptr, shape=(_lib.PRESENT_MAGMA_ROWS, 4)).copy()


def seismic_table():
    """``(255 * seismic(.)).astype(uint8)`` as the kernel holds it: uint8 [257, 4], rows 0..255 the entries of matplotlib's
    ``seismic`` map, row 256 a NaN's colour; ``tof_to_image`` shows the first three bytes of a row"""
    ptr = _lib.load().gft_present_seismic()
    return np.ctypeslib.as_array(ptr, shape=(_lib.PRESENT_SEISMIC_ROWS, 4)).copy()


def blocks(pixels):
    """workgroups of a launch over an image of `pixels` = rows of its partials; 0 for no pixel"""
    return int(_lib.load().gft_present_blocks(int(pixels)))


def sheet_layout(H, W, groups):
    """(bytes of the sheet, {image name: byte offset}) of an H x W view with the ``_lib.PRESENT_HAS_*`` groups `groups`"""
    offsets = (C.c_int64 * len(IMAGES))()
    total = int(_lib.load().gft_present_sheet_bytes(int(H), int(W), int(groups), offsets))
    if total < 1:
        raise ValueError("gftorf_amd.present: no sheet for H=%d W=%d groups=%d" % (H, W, groups))
    return total, {name: int(offsets[k]) for k, name in enumerate(IMAGES) if offsets[k] >= 0}


def _planes(t, name, least, most, size=None):
    """``_args.planes`` (an exact plane count is worded as such); `size` = ((H, W), the name of the input that set it)"""
    t, stride = _args.planes(_TAG, t, name, least, most, want="%d" % least if least == most else None)
    H, W = int(t.shape[1]), int(t.shape[2])
    if size is not None and (H, W) != size[0]:
        raise RuntimeError("gftorf_amd.present: %s is %d x %d, %s %d x %d: the inputs of one call have one size"
                           % ((name, H, W, size[1]) + size[0]))
    return t, stride


def _views(sheet, offsets, H, W):
    out = {}
    for name, bpp, dtype, shape in _lib.PRESENT_IMAGES:
        if name in offsets:
            n = bpp * H * W
            part = sheet[offsets[name]:offsets[name] + n]
            out[name] = (part.view(torch.float32) if dtype == "float32" else part).view(shape(H, W))
    return out


def view_images(image=None, phasor=None, depth=None, acc=None, dd=None, *, ranges=None, zplanes=None, depth_range=None,
                phase_offset=0.0, tof_multiplier=1.0, quad=None, out=None, _partials=None):
    """The display images of one view, ``render.py:129-184``, as a dict of device tensors that are views into one uint8
    buffer (the sheet; every image starts on a 16-byte boundary of it).  All inputs are float32 on one HIP device and share
    one H x W; a group that is not given produces no key:

    ``image`` [3, H, W]: ``color`` uint8 [H, W, 3].
    ``phasor`` [>= 3, H, W] (planes read in place through their stride): ``real``, ``imag`` uint8 [H, W, 3] and ``amp`` uint8
        [H, W], of the planes times ``tof_multiplier`` normalised by ``ranges``; ``depth_tof`` uint8 [H, W, 4] and
        ``depth_tof_f`` float32 [H, W], numpy's ``depth_from_tof`` of planes 0 and 1 (not multiplied) with ``depth_range`` and
        ``phase_offset``; with exactly 7 planes also ``quad`` uint8 [4, H, W] (``quad=True`` demands it, ``quad=False``
        leaves it out).
    ``depth`` [1, H, W]: ``depth`` uint8 [H, W, 4]; with ``acc`` [1, H, W] also ``depth_norm`` and ``depth_norm_f``.
    ``dd`` [1, H, W]: ``dd`` uint8 [H, W], normalised by its own min and max.

    ``ranges``: the (lo, hi) of ``real``, ``imag`` and ``amp``: six numbers, or a float32 device tensor [6] read when the
    kernel runs (``PhasorRanges.tensor``).  ``zplanes`` = (znear, zfar) of the colour map, by value (``zplanes()``).
    ``depth_range``, ``phase_offset``: a number, or a one-element float32 device tensor read when the kernel runs.
    ``out``: a uint8 device tensor of at least the sheet's size, 16-byte aligned, to write into; else a new one.
    Nothing is read on the host; the call can be captured in a graph."""
    lib = _lib.load()
    named, size = [], None

    def take(t, name, least, most):
        nonlocal size
        t, stride = _planes(t, name, least, most, size)
        if size is None:
            size = ((int(t.shape[1]), int(t.shape[2])), name)
        named.append((t, name))
        return t, stride

    im = ph = d = a = dist = None
    im_stride = ph_stride = planes = 0
    if image is not None:
        im, im_stride = take(image, "image", 3, 3)
    if phasor is not None:
        ph, ph_stride = take(phasor, "phasor", 3, 1 << 30)
        planes = int(ph.shape[0])
    if quad and planes != 7:
        raise RuntimeError("gftorf_amd.present: quad needs a phasor of exactly 7 planes, got %s"
                           % ("none" if ph is None else list(ph.shape)))
    if acc is not None and depth is None:
        raise ValueError("gftorf_amd.present: acc is given without depth: depth_norm is depth / acc")
    if depth is not None:
        d = take(depth, "depth", 1, 1)[0]
    if acc is not None:
        a = take(acc, "acc", 1, 1)[0]
    if dd is not None:
        dist = take(dd, "dd", 1, 1)[0]
    if not named:
        raise ValueError("gftorf_amd.present: nothing to show: give image, phasor, depth or dd")
    rg_t, rg_host, dr_t, po_t = None, None, None, None
    dr = po = 0.0
    if ph is not None:
        if ranges is None:
            raise ValueError("gftorf_amd.present: real, imag and amp of phasor need ranges")
        if depth_range is None:
            raise ValueError("gftorf_amd.present: the ToF depth of phasor needs depth_range")
        if isinstance(ranges, torch.Tensor):
            rg_t = _args.tensor(_TAG, ranges, "ranges")
            if tuple(rg_t.shape) != (6,) or not rg_t.is_contiguous():
                raise RuntimeError("gftorf_amd.present: ranges must be six numbers or a contiguous tensor [6], got %s" % list(rg_t.shape))
            named.append((rg_t, "ranges"))
        else:
            vals = [float(x) for x in np.asarray(ranges, dtype=np.float32).reshape(-1)]
            if len(vals) != 6:
                raise RuntimeError("gftorf_amd.present: ranges must be six numbers or a contiguous tensor [6], got %d numbers" % len(vals))
            rg_host = (C.c_float * 6)(*vals)
        dr_t, dr = _args.scalar(_TAG, depth_range, "depth_range", named)
        po_t, po = _args.scalar(_TAG, phase_offset, "phase_offset", named)
    znear = zfar = 0.0
    if ph is not None or d is not None:
        if zplanes is None:
            raise ValueError("gftorf_amd.present: the colour map of a depth needs zplanes = (znear, zfar)")
        znear, zfar = (float(z) for z in zplanes)
    dev = _args.devices(_TAG, "display", named)
    (H, W) = size[0]
    groups = ((_lib.PRESENT_HAS_COLOR if im is not None else 0) | (_lib.PRESENT_HAS_PHASOR if ph is not None else 0) |
              (_lib.PRESENT_HAS_QUAD if planes == 7 and quad is not False else 0) | (_lib.PRESENT_HAS_DEPTH if d is not None else 0) |
              (_lib.PRESENT_HAS_ACC if a is not None else 0) | (_lib.PRESENT_HAS_DD if dist is not None else 0))
    # the C call shows quad for exactly 7 planes: fewer are declared when quad is left out
    planes_arg = 7 if groups & _lib.PRESENT_HAS_QUAD else min(planes, 3)
    total, offsets = sheet_layout(H, W, groups)
    if out is None:
        out = torch.empty((total,), device=dev, dtype=torch.uint8)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
            raise TypeError("gftorf_amd.present: out must be a contiguous one-dimensional torch.uint8 tensor")
        if out.device != dev:
            raise RuntimeError("gftorf_amd.present: the images are on %s, out on %s" % (dev, out.device))
        if out.numel() < total or out.data_ptr() % _lib.PRESENT_ALIGN:
            raise RuntimeError("gftorf_amd.present: out has %d bytes at an address %s 16-byte aligned, the sheet needs %d aligned bytes"
                               % (out.numel(), "that is not" if out.data_ptr() % _lib.PRESENT_ALIGN else "that is", total))
    partials = _partials
    if dist is not None and partials is None:
        partials = torch.empty((blocks(H * W), _lib.PRESENT_PARTIAL_WORDS), device=dev, dtype=torch.float32)
    with _lib.on_device(dev):
        _lib.check(lib.gft_present_view(_lib.raw_stream(dev), H, W, _ptr(im), im_stride, _ptr(ph), ph_stride, planes_arg, _ptr(d), _ptr(a),
                                        _ptr(dist), _ptr(rg_t), rg_host, _ptr(dr_t), dr, _ptr(po_t), po, znear, zfar,
                                        float(tof_multiplier), _ptr(partials) if dist is not None else None, out.data_ptr()))
    return _views(out, offsets, H, W)


def quad_images(phasor, permutation=(0, 1, 2, 3), has_gt=False, tonemap=False, out=None):
    """The four quad images of a view, ``render_ftorf_viz_traj.py:237-244``, as one uint8 device tensor [4, H, W, 3] written
    by one launch: image i is ``tof_to_image`` (``scene/torf_utils.py:43-50``: clip to [-0.5, 0.5], ``Normalize(-0.5, 0.5)``,
    matplotlib's ``seismic`` map, ``(255 * rgb).astype(uint8)``) of plane ``3 + permutation[i]`` of ``phasor`` [7, H, W]
    (float32 on a HIP device, planes read in place through their stride), after ``- 0.5`` when ``has_gt`` and ``x / (1 + x)``
    when ``tonemap`` (``args.quad_scale > 1``).  ``permutation``: the scene's ``tof_inverse_permutation``, four host integers
    in 0..3.  ``out``: a contiguous uint8 device tensor [4, H, W, 3] to write into; else a new one.  The bytes are the
    reference's; nothing is read on the host, so the call can be captured in a graph."""
    ph, stride = _planes(phasor, "phasor", 7, 7)
    try:
        perm = [int(k) for k in (permutation.tolist() if hasattr(permutation, "tolist") else permutation)]
    except (TypeError, ValueError):
        raise TypeError("gftorf_amd.present: permutation must be four integers, got %r" % (permutation,)) from None
    if len(perm) != 4 or any(not 0 <= k <= 3 for k in perm):
        raise ValueError("gftorf_amd.present: permutation must be four integers in 0..3, got %s" % perm)
    H, W = int(ph.shape[1]), int(ph.shape[2])
    named = [(ph, "phasor")]
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (4, H, W, 3) or not out.is_contiguous():
            raise TypeError("gftorf_amd.present: out must be a contiguous torch.uint8 tensor [4, %d, %d, 3]" % (H, W))
        named.append((out, "out"))
    dev = _args.devices(_TAG, "display", named)
    lib = _lib.load()
    if out is None:
        out = torch.empty((4, H, W, 3), device=dev, dtype=torch.uint8)
    with _lib.on_device(dev):
        _lib.check(lib.gft_present_quad(_lib.raw_stream(dev), H, W, ph.data_ptr(), stride, (C.c_int32 * 4)(*perm), int(bool(has_gt)),
                                        int(bool(tonemap)), out.data_ptr()))
    return out


def flow_wheel():
    """The Middlebury colour wheel of ``make_color_wheel`` (``scene/torf_utils.py:150-197``) as the kernel holds it: uint8
    [55, 3]"""
    ptr = _lib.load().gft_flowviz_wheel()
    return np.ctypeslib.as_array(ptr, shape=(_lib.FLOWVIZ_WHEEL_ROWS, 3)).copy()


def flow_blocks(pixels):
    """workgroups of ``flow_images``' launches over an image of `pixels`; its partials hold one float more; 0 for no pixel"""
    return int(_lib.load().gft_flowviz_blocks(int(pixels)))


def flow_images(flow, gt_flow, out=None, _partials=None):
    """The three optical-flow debug images of one direction, ``train.py:382-386``: ``flow_to_image`` (``scene/torf_utils.py:
    242-305``) of (rendered, target), (target, target) and (target - rendered, target) as the reference's sequence of calls
    leaves them -- ``flow_to_image`` zeroes the unknown (> 200) and NaN pixels of its arguments in place, so the later calls
    see the earlier ones' edits -- in two launches.  Returns ``{"flow": ..., "gt": ..., "error": ...}``, uint8 [H, W, 3] views
    into one device tensor [3, H, W, 3].

    ``flow`` [>= 2, H, W]: the rendered 2-D flow, planes 0 and 1 read in place through their stride (``render_flow``'s 3-plane
    output or a slice of it needs no copy).  ``gt_flow`` [2, H, W]: the target.  Both float32 on one HIP device; neither is
    written.  ``out``: a contiguous uint8 device tensor [3, H, W, 3] to write into; else a new one.
    The arithmetic is numpy >= 2's: the float32 ``maxrad * 1.1`` plus the float64 ``eps`` is a float64, and so is everything
    behind the division by it (numpy 1.x stays in float32 and gives other bytes).  Only ``arctan2``'s last bits may differ
    (tests/test_present_flow.py).  Nothing is read on the host; the call can be captured in a graph."""
    fl, fl_stride = _args.planes(_TAG, flow, "flow", 2, 1 << 30, keep=2)
    H, W = int(fl.shape[1]), int(fl.shape[2])
    gt, gt_stride = _planes(gt_flow, "gt_flow", 2, 2, ((H, W), "flow"))
    named = [(fl, "flow"), (gt, "gt_flow")]
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (_lib.FLOWVIZ_IMAGES, H, W, 3)
                or not out.is_contiguous()):
            raise TypeError("gftorf_amd.present: out must be a contiguous torch.uint8 tensor [3, %d, %d, 3]" % (H, W))
        named.append((out, "out"))
    dev = _args.devices(_TAG, "display", named)
    lib = _lib.load()
    rows = flow_blocks(H * W) + 1
    partials = _partials
    if partials is None:
        partials = torch.empty((rows,), device=dev, dtype=torch.float32)
    elif (not isinstance(partials, torch.Tensor) or partials.dtype != torch.float32 or partials.device != dev or partials.numel() < rows
          or not partials.is_contiguous()):
        raise RuntimeError("gftorf_amd.present: the partials of a %d x %d flow are %d contiguous float32 on %s" % (H, W, rows, dev))
    if out is None:
        out = torch.empty((_lib.FLOWVIZ_IMAGES, H, W, 3), device=dev, dtype=torch.uint8)
    with _lib.on_device(dev):
        _lib.check(lib.gft_flowviz_images(_lib.raw_stream(dev), H, W, fl.data_ptr(), fl_stride, gt.data_ptr(), gt_stride,
                                          partials.data_ptr(), out.data_ptr()))
    return {"flow": out[0], "gt": out[1], "error": out[2]}


DEBUG_IMAGES = tuple(name for name, _, _ in _lib.DEBUGVIZ_IMAGES)    # the keys, in the order the images lie in a debug sheet
_DEBUG_EVERY = (_lib.DEBUGVIZ_HAS_PHASOR | _lib.DEBUGVIZ_HAS_GT_PHASOR | _lib.DEBUGVIZ_HAS_DEPTH | _lib.DEBUGVIZ_HAS_PHASE_DEPTH |
                _lib.DEBUGVIZ_HAS_GT_PHASE_DEPTH | _lib.DEBUGVIZ_HAS_DD | _lib.DEBUGVIZ_HAS_COLOR | _lib.DEBUGVIZ_HAS_QUAD |
                _lib.DEBUGVIZ_HAS_GT_QUAD)


def debug_blocks(pixels):
    """workgroups of ``debug_images``' launches over an image of `pixels` = rows of its partials; 0 for no pixel"""
    return int(_lib.load().gft_debugviz_blocks(int(pixels)))


def debug_sheet_layout(H, W, groups):
    """(bytes of the sheet, {image name: byte offset}) of the debug images of an H x W view with the ``_lib.DEBUGVIZ_HAS_*``
    groups `groups`"""
    offsets = (C.c_int64 * len(DEBUG_IMAGES))()
    total = int(_lib.load().gft_debugviz_sheet_bytes(int(H), int(W), int(groups), offsets))
    if total < 1:
        raise ValueError("gftorf_amd.present: no debug sheet for H=%d W=%d groups=%d" % (H, W, groups))
    return total, {name: int(offsets[k]) for k, name in enumerate(DEBUG_IMAGES) if offsets[k] >= 0}


def _plane(t, name, size):
    """an [H, W] plane (``tof.depth_from_tof``'s result) as a [1, H, W] one, sized like the other inputs"""
    t = _args.tensor(_TAG, t, name)
    if t.dim() != 2:
        raise RuntimeError("gftorf_amd.present: %s must be [H, W], got %s" % (name, list(t.shape)))
    return _planes(t[None], name, 1, 1, size)[0]


def debug_images(phasor=None, gt_phasor=None, depth=None, phase_depth=None, gt_phase_depth=None, dd=None, image=None, gt_image=None,
                 gt_quad=None, *, permutation=(0, 1, 2, 3), quad_index=None, ranges=None, zplanes=None, tof_multiplier=1.0, out=None,
                 _partials=None):
    """The debug images of one training iteration, the ToF branch of ``train.py:295-378``, as a dict of uint8 device tensors
    that are views into one buffer (the sheet; every image starts on a 16-byte boundary of it).  All inputs are float32 on
    one HIP device and share one H x W; every one is optional, and an image is produced when every input its formula names
    is given.  With ``amp = phasor[2] * tof_multiplier``, ``gt_amp = gt_phasor[2]``, ``sp = amp * depth ** 2``, ``sp_tof = amp *
    phase_depth ** 2`` and ``gt_sp = gt_amp * gt_phase_depth ** 2``:

    ``depth`` [1, H, W]: ``depth`` [H, W, 4], the magma map of ``view_images``.
    ``phasor`` [>= 3, H, W] (plane 2 read in place through the stride): ``amp`` [H, W]; with ``gt_phasor`` [>= 3, H, W]
        ``amp_error``, normalised by its own min and max; with ``depth`` ``scattering_phase``, with ``phase_depth`` [H, W]
        ``scattering_phase_tof_depth``; with ``gt_phasor`` and ``gt_phase_depth`` [H, W] their unnormalised
        ``scattering_phase_error`` / ``scattering_phase_tof_depth_error``.
    ``gt_phasor`` and ``gt_phase_depth``: ``scattering_phase_gt``.
    ``phase_depth``, ``gt_phase_depth`` (``tof.depth_from_tof``'s, as ``train.py:188-189`` has them): ``phase_depth``,
        ``phase_depth_gt`` [H, W, 4]; together ``phase_depth_error``, and with ``depth`` ``depth_error``, each normalised by its
        own min and max.
    ``image``, ``gt_image`` [3, H, W], given together: ``color``, ``color_gt``, ``color_error`` [H, W, 3].
    ``dd`` [1, H, W]: ``dd`` [H, W], normalised by its own min and max.
    ``phasor`` of exactly 7 planes: ``quad`` [4, H, W]; with ``gt_quad`` [4, H, W] also ``quad_gt`` and ``quad_error``, whose plane
        i shows ``gt_quad[permutation[i]]`` and is all 0 unless ``permutation[i] == quad_index``.

    ``permutation``: ``scene.tof_permutation``, four host integers in 0..3.  ``quad_index``: ``frame_id % 4`` as an int, or a
    one-element int32 device tensor read when the kernel runs.  ``ranges``: eight numbers, or a contiguous float32 device
    tensor [8] read when the kernel runs -- the (lo, hi) of ``amp``, ``scattering_phase``, ``scattering_phase_tof_depth`` and
    ``scattering_phase_gt``, which ``train.py:317``'s zip makes ``np.min`` / ``np.max`` over the training sequence of ``gt_reals``,
    ``gt_imags``, ``gt_amps`` (``PhasorRanges.tensor``, in that order) and ``gt_scattering_phases``.  ``zplanes`` = (znear, zfar) of
    the colour map, by value (``zplanes()``).  ``out``: a uint8 device tensor of at least the sheet's size, 16-byte aligned, to
    write into; else a new one.  At most two launches; nothing is read on the host, so the call can be captured in a graph,
    and the bytes are the reference's."""
    lib = _lib.load()
    named, size = [], None

    def take(t, name, least, most):
        nonlocal size
        t, stride = _planes(t, name, least, most, size)
        if size is None:
            size = ((int(t.shape[1]), int(t.shape[2])), name)
        named.append((t, name))
        return t, stride

    def take_plane(t, name):
        nonlocal size
        t = _plane(t, name, size)
        if size is None:
            size = ((int(t.shape[1]), int(t.shape[2])), name)
        named.append((t, name))
        return t

    ph = gph = d = pd = gpd = dist = im = gim = gq = None
    ph_stride = gph_stride = im_stride = gim_stride = gq_stride = planes = 0
    if (image is None) != (gt_image is None):
        raise ValueError("gftorf_amd.present: image and gt_image are given together, got only %s"
                         % ("image" if gt_image is None else "gt_image"))
    if phasor is not None:
        ph, ph_stride = take(phasor, "phasor", 3, 1 << 30)
        planes = int(ph.shape[0])
    if gt_phasor is not None:
        gph, gph_stride = take(gt_phasor, "gt_phasor", 3, 1 << 30)
    if depth is not None:
        d = take(depth, "depth", 1, 1)[0]
    if phase_depth is not None:
        pd = take_plane(phase_depth, "phase_depth")
    if gt_phase_depth is not None:
        gpd = take_plane(gt_phase_depth, "gt_phase_depth")
    if dd is not None:
        dist = take(dd, "dd", 1, 1)[0]
    if image is not None:
        im, im_stride = take(image, "image", 3, 3)
        gim, gim_stride = take(gt_image, "gt_image", 3, 3)
    if gt_quad is not None:
        if planes != 7:
            raise RuntimeError("gftorf_amd.present: gt_quad needs a phasor of exactly 7 planes, got %s"
                               % ("none" if ph is None else list(ph.shape)))
        gq, gq_stride = take(gt_quad, "gt_quad", 4, 4)
    if not named:
        raise ValueError("gftorf_amd.present: nothing to show: give phasor, depth, phase_depth, gt_phase_depth, dd or image")
    groups = ((_lib.DEBUGVIZ_HAS_PHASOR if ph is not None else 0) | (_lib.DEBUGVIZ_HAS_GT_PHASOR if gph is not None else 0) |
              (_lib.DEBUGVIZ_HAS_DEPTH if d is not None else 0) | (_lib.DEBUGVIZ_HAS_PHASE_DEPTH if pd is not None else 0) |
              (_lib.DEBUGVIZ_HAS_GT_PHASE_DEPTH if gpd is not None else 0) | (_lib.DEBUGVIZ_HAS_DD if dist is not None else 0) |
              (_lib.DEBUGVIZ_HAS_COLOR if im is not None else 0) | (_lib.DEBUGVIZ_HAS_QUAD if planes == 7 else 0) |
              (_lib.DEBUGVIZ_HAS_GT_QUAD if gq is not None else 0))
    (H, W) = size[0]
    total, offsets = debug_sheet_layout(H, W, groups)
    perm, qi_t, qi = None, None, 0
    if gq is not None:
        try:
            vals = [int(k) for k in (permutation.tolist() if hasattr(permutation, "tolist") else permutation)]
        except (TypeError, ValueError):
            raise TypeError("gftorf_amd.present: permutation must be four integers, got %r" % (permutation,)) from None
        if len(vals) != 4 or any(not 0 <= k <= 3 for k in vals):
            raise ValueError("gftorf_amd.present: permutation must be four integers in 0..3, got %s" % vals)
        perm = (C.c_int32 * 4)(*vals)
        if quad_index is None:
            raise ValueError("gftorf_amd.present: quad_error of gt_quad needs quad_index = frame_id % 4")
        if isinstance(quad_index, torch.Tensor):
            qi_t = _args.tensor(_TAG, quad_index, "quad_index", (torch.int32,))
            if qi_t.numel() != 1:
                raise RuntimeError("gftorf_amd.present: quad_index must be an integer or a one-element tensor, got %s" % list(qi_t.shape))
            named.append((qi_t, "quad_index"))
        else:
            qi = int(quad_index)
    rg_t, rg_host = None, None
    if "amp" in offsets or "scattering_phase_gt" in offsets:
        words = _lib.DEBUGVIZ_RANGE_WORDS
        if ranges is None:
            raise ValueError("gftorf_amd.present: amp and the scattering phases need ranges")
        if isinstance(ranges, torch.Tensor):
            rg_t = _args.tensor(_TAG, ranges, "ranges")
            if tuple(rg_t.shape) != (words,) or not rg_t.is_contiguous():
                raise RuntimeError("gftorf_amd.present: ranges must be eight numbers or a contiguous tensor [8], got %s" % list(rg_t.shape))
            named.append((rg_t, "ranges"))
        else:
            vals = [float(x) for x in np.asarray(ranges, dtype=np.float32).reshape(-1)]
            if len(vals) != words:
                raise RuntimeError("gftorf_amd.present: ranges must be eight numbers or a contiguous tensor [8], got %d numbers" % len(vals))
            rg_host = (C.c_float * words)(*vals)
    znear = zfar = 0.0
    if d is not None or pd is not None or gpd is not None:
        if zplanes is None:
            raise ValueError("gftorf_amd.present: the colour map of a depth needs zplanes = (znear, zfar)")
        znear, zfar = (float(z) for z in zplanes)
    dev = _args.devices(_TAG, "display", named)
    if out is None:
        out = torch.empty((total,), device=dev, dtype=torch.uint8)
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous():
            raise TypeError("gftorf_amd.present: out must be a contiguous one-dimensional torch.uint8 tensor")
        if out.device != dev:
            raise RuntimeError("gftorf_amd.present: the images are on %s, out on %s" % (dev, out.device))
        if out.numel() < total or out.data_ptr() % _lib.DEBUGVIZ_ALIGN:
            raise RuntimeError("gftorf_amd.present: out has %d bytes at an address %s 16-byte aligned, the sheet needs %d aligned bytes"
                               % (out.numel(), "that is not" if out.data_ptr() % _lib.DEBUGVIZ_ALIGN else "that is", total))
    rows = debug_blocks(H * W)
    partials = _partials
    if partials is None:
        partials = torch.empty((rows, _lib.DEBUGVIZ_PARTIAL_WORDS), device=dev, dtype=torch.float32)
    elif (not isinstance(partials, torch.Tensor) or partials.dtype != torch.float32 or partials.device != dev
          or partials.numel() < rows * _lib.DEBUGVIZ_PARTIAL_WORDS or not partials.is_contiguous() or partials.data_ptr() % 16):
        raise RuntimeError("gftorf_amd.present: the partials of a %d x %d debug sheet are %d x %d contiguous float32 on %s, 16-byte aligned"
                           % (H, W, rows, _lib.DEBUGVIZ_PARTIAL_WORDS, dev))
    with _lib.on_device(dev):
        _lib.check(lib.gft_debugviz_images(_lib.raw_stream(dev), H, W, _ptr(ph), ph_stride, planes, _ptr(gph), gph_stride, _ptr(d), _ptr(pd),
                                           _ptr(gpd), _ptr(dist), _ptr(im), im_stride, _ptr(gim), gim_stride, _ptr(gq), gq_stride, perm,
                                           _ptr(qi_t), qi, _ptr(rg_t), rg_host, znear, zfar, float(tof_multiplier), partials.data_ptr(),
                                           out.data_ptr()))
    images = {}
    for name, bpp, shape in _lib.DEBUGVIZ_IMAGES:
        if name in offsets:
            images[name] = out[offsets[name]:offsets[name] + bpp * H * W].view(shape(H, W))
    return images


class PhasorRanges:
    """The normalisation ranges of ``real``, ``imag`` and ``amp``: ``save_input``'s ``np.min`` / ``np.max`` over the whole
    ground-truth sequence (``render.py:46-47, 61``) as a float32 device tensor [6] = (lo, hi) three times::

        ranges = present.PhasorRanges()
        for view in views:
            ranges.add(view.original_tof_image)               # no host read
        present.view_images(..., ranges=ranges.tensor)

    ``lo`` of ``real`` and ``imag`` is taken over the three channels of the red / blue images as the reference forms them (the
    green one is 0), so it is 0 for finite input.  A NaN stays, as in numpy."""

    def __init__(self, device=None):
        lib = _lib.load()
        self.device = _args.indexed_device(_TAG, "PhasorRanges", device)
        self.tensor = torch.empty((_lib.PRESENT_RANGE_WORDS,), device=self.device, dtype=torch.float32)
        # the scratch of the largest launch there is, once: a graph captured by an earlier add keeps its address
        self._partials = torch.empty((int(lib.gft_present_blocks(1 << 40)), _lib.PRESENT_RANGE_WORDS), device=self.device,
                                     dtype=torch.float32)
        self.reset()

    def reset(self):
        """(+inf, -inf) three times, by one kernel on the current stream"""
        with _lib.on_device(self.device):
            _lib.check(_lib.load().gft_present_ranges_reset(_lib.raw_stream(self.device), self.tensor.data_ptr()))

    def add(self, gt_tof):
        """Fold one ground-truth ToF image [>= 3, H, W] (planes 0..2 are read, in place) into the ranges: two launches"""
        t, stride = _planes(gt_tof, "gt_tof", 3, 1 << 30)
        if _args.devices(_TAG, "display", [(t, "gt_tof")]) != self.device:
            raise RuntimeError("gftorf_amd.present: gt_tof is on %s, the ranges on %s" % (t.device, self.device))
        with _lib.on_device(self.device):
            _lib.check(_lib.load().gft_present_ranges(_lib.raw_stream(self.device), int(t.shape[1] * t.shape[2]), t.data_ptr(), stride,
                                                      self._partials.data_ptr(), self.tensor.data_ptr()))

    def result(self):
        """the six values as a float32 numpy array: the one blocking read"""
        return self.tensor.cpu().numpy()


class ViewSheets:
    """Pinned staging for a render loop: the device forms view i + 1 while the host encodes view i::

        sheets = present.ViewSheets(slots=2)
        for vid, view in enumerate(views):
            pkg = render_eval(view, ...)
            sheets.submit(vid, image=pkg["render"], phasor=pkg["render_phasor"], ..., ranges=ranges.tensor, zplanes=zp, ...)
            for tag, images in sheets.ready():                # the views whose copy has completed, oldest first
                write_pngs(tag, images)                       # numpy arrays over pinned memory
        for tag, images in sheets.ready(wait=True):
            write_pngs(tag, images)

    ``submit`` never waits: with every slot in flight or handed out it raises.  The arrays ``ready`` yields belong to their
    slot, which is free again when the loop moves past them (or with the next ``ready`` call)."""

    def __init__(self, slots=2):
        _lib.load()
        if int(slots) < 1:
            raise ValueError("gftorf_amd.present: ViewSheets needs at least one slot, got %s" % slots)
        self._slots = [dict(state="free", device=None, host=None, partials=None, event=None) for _ in range(int(slots))]
        self._order = []          # slots in flight, oldest first
        self._lent = []           # slots whose arrays the caller holds

    def _release(self):
        for s in self._lent:
            s["state"] = "free"
        self._lent = []

    def submit(self, tag, **view):
        """``view_images(**view)`` into a free slot, the sheet's copy to pinned memory and an event, all on the current stream"""
        slot = next((s for s in self._slots if s["state"] == "free"), None)
        if slot is None:
            raise RuntimeError("gftorf_amd.present: all %d slots of this ViewSheets are in flight; take the finished views with ready()"
                               % len(self._slots))
        first = next((v for v in (view.get(k) for k in ("image", "phasor", "depth", "dd")) if isinstance(v, torch.Tensor)), None)
        if first is None or first.dim() != 3:
            raise ValueError("gftorf_amd.present: nothing to show: give image, phasor, depth or dd as [C, H, W] tensors")
        H, W = int(first.shape[1]), int(first.shape[2])
        # the largest sheet of this size: what the groups leave out is not copied
        full = sheet_layout(H, W, _EVERY)[0]
        if slot["device"] is None or slot["device"].numel() < full or slot["device"].device != first.device:
            slot["device"] = torch.empty((full,), device=first.device, dtype=torch.uint8)
            slot["host"] = torch.empty((full,), dtype=torch.uint8, pin_memory=True)
            slot["partials"] = torch.empty((max(1, blocks(H * W)), _lib.PRESENT_PARTIAL_WORDS), device=first.device, dtype=torch.float32)
            slot["event"] = torch.cuda.Event()
        images = view_images(out=slot["device"], _partials=slot["partials"], **view)
        last = max(images.values(), key=lambda t: t.data_ptr())
        used = last.data_ptr() - slot["device"].data_ptr() + last.numel() * last.element_size()
        slot["host"][:used].copy_(slot["device"][:used], non_blocking=True)
        slot["event"].record()
        host = slot["host"].numpy()
        base = slot["device"].data_ptr()
        arrays = {}
        for name, t in images.items():
            o = t.data_ptr() - base
            raw = host[o:o + t.numel() * t.element_size()]
            arrays[name] = (raw.view(np.float32) if t.dtype == torch.float32 else raw).reshape(tuple(t.shape))
        slot.update(state="flight", tag=tag, arrays=arrays)
        self._order.append(slot)

    def submit_flow(self, tag, flow, gt_flow):
        """``flow_images(flow, gt_flow)`` into a free slot, the three images' copy to pinned memory and an event, all on the
        current stream; ``ready`` yields the tag with ``{"flow", "gt", "error"}`` as uint8 [H, W, 3] arrays"""
        slot = next((s for s in self._slots if s["state"] == "free"), None)
        if slot is None:
            raise RuntimeError("gftorf_amd.present: all %d slots of this ViewSheets are in flight; take the finished views with ready()"
                               % len(self._slots))
        if not isinstance(flow, torch.Tensor) or flow.dim() != 3:
            raise ValueError("gftorf_amd.present: nothing to show: give flow as a [C, H, W] tensor")
        dev = _args.devices(_TAG, "display", [(flow, "flow")])
        H, W = int(flow.shape[1]), int(flow.shape[2])
        need = _lib.FLOWVIZ_IMAGES * H * W * 3
        if slot["device"] is None or slot["device"].numel() < need or slot["device"].device != dev:
            slot["device"] = torch.empty((need,), device=dev, dtype=torch.uint8)
            slot["host"] = torch.empty((need,), dtype=torch.uint8, pin_memory=True)
            # submit() takes a slot whose buffer is large enough with its partials: rows for as many pixels as there are bytes
            slot["partials"] = torch.empty((max(1, blocks(need)), _lib.PRESENT_PARTIAL_WORDS), device=dev, dtype=torch.float32)
            slot["event"] = torch.cuda.Event()
        rows = flow_blocks(H * W) + 1
        scratch = slot.get("flow_partials")
        if scratch is None or scratch.numel() < rows or scratch.device != dev:
            scratch = slot["flow_partials"] = torch.empty((rows,), device=dev, dtype=torch.float32)
        flow_images(flow, gt_flow, out=slot["device"][:need].view(_lib.FLOWVIZ_IMAGES, H, W, 3), _partials=scratch)
        slot["host"][:need].copy_(slot["device"][:need], non_blocking=True)
        slot["event"].record()
        host = slot["host"].numpy()[:need].reshape(_lib.FLOWVIZ_IMAGES, H, W, 3)
        slot.update(state="flight", tag=tag, arrays={"flow": host[0], "gt": host[1], "error": host[2]})
        self._order.append(slot)

    def submit_debug(self, tag, **debug):
        """``debug_images(**debug)`` into a free slot, the sheet's copy to pinned memory and an event, all on the current stream;
        ``ready`` yields the tag with the images ``debug_images`` returns, as uint8 arrays"""
        slot = next((s for s in self._slots if s["state"] == "free"), None)
        if slot is None:
            raise RuntimeError("gftorf_amd.present: all %d slots of this ViewSheets are in flight; take the finished views with ready()"
                               % len(self._slots))
        keys = ("phasor", "gt_phasor", "depth", "phase_depth", "gt_phase_depth", "dd", "image", "gt_image", "gt_quad")
        first = next((v for v in (debug.get(k) for k in keys) if isinstance(v, torch.Tensor)), None)
        if first is None or first.dim() not in (2, 3):
            raise ValueError("gftorf_amd.present: nothing to show: give phasor, depth, dd or image as [C, H, W] tensors, the ToF depths "
                             "as [H, W] ones")
        dev = _args.devices(_TAG, "display", [(first, next(k for k in keys if debug.get(k) is first))])
        H, W = int(first.shape[-2]), int(first.shape[-1])
        # the largest debug sheet of this size: what the groups leave out is not copied
        full = debug_sheet_layout(H, W, _DEBUG_EVERY)[0]
        if slot["device"] is None or slot["device"].numel() < full or slot["device"].device != dev:
            slot["device"] = torch.empty((full,), device=dev, dtype=torch.uint8)
            slot["host"] = torch.empty((full,), dtype=torch.uint8, pin_memory=True)
            # submit() takes a slot whose buffer is large enough with its partials: rows for as many pixels as there are bytes
            slot["partials"] = torch.empty((max(1, blocks(full)), _lib.PRESENT_PARTIAL_WORDS), device=dev, dtype=torch.float32)
            slot["event"] = torch.cuda.Event()
        rows = debug_blocks(H * W)
        scratch = slot.get("debug_partials")
        if scratch is None or scratch.shape[0] < rows or scratch.device != dev:
            scratch = slot["debug_partials"] = torch.empty((rows, _lib.DEBUGVIZ_PARTIAL_WORDS), device=dev, dtype=torch.float32)
        images = debug_images(out=slot["device"], _partials=scratch, **debug)
        last = max(images.values(), key=lambda t: t.data_ptr())
        used = last.data_ptr() - slot["device"].data_ptr() + last.numel()
        slot["host"][:used].copy_(slot["device"][:used], non_blocking=True)
        slot["event"].record()
        host = slot["host"].numpy()
        base = slot["device"].data_ptr()
        arrays = {name: host[t.data_ptr() - base:t.data_ptr() - base + t.numel()].reshape(tuple(t.shape)) for name, t in images.items()}
        slot.update(state="flight", tag=tag, arrays=arrays)
        self._order.append(slot)

    def ready(self, wait=False):
        """Yields (tag, {name: numpy array}) of the submitted views whose copy has completed, oldest first, and stops at the
        first that has not; ``wait=True`` waits for each instead, so every submitted view comes out."""
        self._release()
        while self._order:
            slot = self._order[0]
            if wait:
                slot["event"].synchronize()
            elif not slot["event"].query():
                return
            self._order.pop(0)
            slot["state"] = "lent"
            self._lent.append(slot)
            yield slot["tag"], slot["arrays"]
            self._release()
