"""The training views on the device (``csrc/k_views.hip``, ``include/gftorf_views.h``): the first statement of an iteration,
"make view v current", as one launch that a captured graph can hold.

The reference draws a camera on the host (``train.py:155-163``), copies its images to the device (``:184-187``) and indexes
the quad planes with a host integer (``:219-220``).  A captured iteration needs all of that in static tensors; by hand it is one
``copy_`` launch per ground-truth tensor and per table row in front of every replay, and the quad lines cannot be captured
at all.  Here:

``ViewStore(device, record=, ints=, **groups)``  every view's floats, integers and images uploaded once into one arena.
    ``draw(v)`` copies view v into the *current* buffer in one launch; ``draw()`` reads v from a device schedule
    (``schedule(order)``) that the launch itself advances, so it can be the first node of a graph and a replay needs no host
    work for the view.  ``current[name]``, ``record``, ``ints``, ``has(name)``, ``index`` are views into that buffer: their
    addresses never change.
``ViewStore.from_cameras(cams, device, ...)``  the store of the reference's ``ToFCamera`` objects: both cameras' matrices,
    the frame's time, the F-ToRF query times and coefficients of ``query.ftorf_schedule``, ``frame_id % 4`` and the images.
``select_plane(x, index, table=, modulo=)``  ``x[table[index % modulo]].unsqueeze(0)`` with ``index`` read on the device, and
    its backward: ``train.py:219-220`` is ``select_plane(gt_quad, store.quad)`` and ``select_plane(phasor[3:], store.quad,
    table=inv_perm)``.
``DrawOrder(frame_ids, start_id, rng)``  the reference's draw restated (pure Python): the view order for any number of
    iterations ahead, consuming ``rng`` exactly as ``train.py:155-163`` would.
``u8(array)``  marks a group kept as bytes ``[V, H, W, C]``; a draw writes ``float(x) / 255.0`` planar, the bits of
    ``PILtoTorch`` (``utils/general_utils.py:22-28``; the ``clamp`` and ``*= ones`` of ``scene/cameras.py:67-73`` are
    identities on them).

There is no CPU path for the store or ``select_plane``; ``DrawOrder`` and ``layout`` run anywhere.
"""
import ctypes as C
import random
from collections import namedtuple

import numpy as np
import torch

from . import _args, _lib
from .query import ftorf_schedule

_TAG = "gftorf_amd.views"
KINDS = _lib.VIEWS_KINDS

# the record ``from_cameras`` writes, in float columns: the colour camera's block and the ToF camera's (view 16, proj 16,
# campos 3 + 1 pad, as bench_loop.py's table), the frame's time, the three scalars, times[4], combine[4][4]
CAMERA_FLOATS = 36
REC_COLOR, REC_TOF, REC_TIME, REC_DEPTH_RANGE, REC_PHASE_OFFSET, REC_DC_OFFSET, REC_TIMES, REC_COMBINE, REC_FLOATS = 0, 36, 72, 73, 74, 75, 76, 80, 96
INT_FRAME, INT_QUAD, INT_K, INT_M, INT_COUNT = 0, 1, 2, 3, 4
# (group of the store, attribute of the camera)
CAMERA_GROUPS = (("color", "original_image"), ("phasor", "original_tof_image"), ("quad", "original_tofQuad_im"),
                 ("distance", "original_distance_image"), ("forward_flow", "forward_flow"), ("backward_flow", "backward_flow"))

Camera = namedtuple("Camera", ("world_view_transform", "full_proj_transform", "camera_center"))
Layout = namedtuple("Layout", ("slab_bytes", "current_bytes", "slab_offsets", "current_offsets", "slab_record", "current_record"))


class u8:
    """A group kept as bytes: uint8 ``[V, H, W, C]`` (or a length-V list of ``[H, W, C]``, None for a view without it), C <= 4"""

    def __init__(self, data):
        self.data = data


def _ints(values):
    return (C.c_int32 * len(values))(*values)


def layout(F, J, groups):
    """``gft_views_layout`` of a record of F float and J int32 columns and ``groups``, a sequence of ``(kind, C, H, W)`` with
    kind ``"f32"`` or ``"u8"``: a ``Layout`` (byte sizes of a slab and of the current buffer, the groups' byte offsets in
    both, the record's), or None for a request that cannot be laid out.  A host function: no device is needed."""
    groups = list(groups)
    n = len(groups)
    if n > _lib.VIEWS_MAX_GROUPS or any(g[0] not in KINDS for g in groups):
        return None
    cols = [_ints([KINDS.index(g[0]) for g in groups])] + [_ints([int(g[k]) for g in groups]) for k in (1, 2, 3)]
    current = C.c_int64(0)
    slab_off, cur_off = (C.c_int64 * (n + 1))(), (C.c_int64 * (n + 1))()
    slab = _lib.load().gft_views_layout(int(F), int(J), n, *cols, C.byref(current), slab_off, cur_off)
    if slab == 0:
        return None
    return Layout(int(slab), int(current.value), tuple(slab_off[:n]), tuple(cur_off[:n]), int(slab_off[n]), int(cur_off[n]))


def _host(a, name, dtype):
    """``a`` (numpy or torch, host or device) as a contiguous numpy array of ``dtype``, which it must already have"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype != dtype:
        raise TypeError("%s: %s must be %s, got %s" % (_TAG, name, np.dtype(dtype).name, a.dtype))
    return np.ascontiguousarray(a)


def _group_rows(data, name, dtype):
    """A group as (list of V arrays or None, shape of one): a [V, ...] array or a length-V list with None for a missing view"""
    if isinstance(data, (list, tuple)):
        rows = [None if d is None else _host(d, "%s[%d]" % (name, i), dtype) for i, d in enumerate(data)]
    else:
        whole = _host(data, name, dtype)
        if whole.ndim != 4:
            raise RuntimeError("%s: %s must be [V, %s], got %s" % (_TAG, name, "H, W, C" if dtype == np.uint8 else "C, H, W", list(whole.shape)))
        rows = list(whole)
    shapes = {r.shape for r in rows if r is not None}
    if len(shapes) != 1:
        raise RuntimeError("%s: the views of %s must share one shape and one must be present, got %s" % (_TAG, name, sorted(shapes)))
    shape = shapes.pop()
    if len(shape) != 3 or min(shape) < 1:
        raise RuntimeError("%s: a view of %s must be three-dimensional and not empty, got %s" % (_TAG, name, list(shape)))
    return rows, shape


class ViewStore:
    """Every training view on the device, and the current one.

    ``record`` float32 ``[V, F]`` and ``ints`` int32 ``[V, J]``: per-view numbers (numpy or torch, host or device).  Each
    keyword is a group: a float32 ``[V, C, H, W]`` tensor, a length-V list of ``[C, H, W]`` tensors with None for a view that
    lacks the image (stored as zeros, ``has(name)`` is 0 for it), or ``u8(...)`` of uint8 ``[V, H, W, C]``.  At most
    ``VIEWS_MAX_GROUPS`` groups.  Everything is uploaded once into one arena allocation and the current buffer is allocated
    once: every tensor the accessors hand out is a view into it, its ``data_ptr()`` fixed for the life of the store, its
    contents those of the view drawn last (zeros before the first draw)."""

    def __init__(self, device, record=None, ints=None, **groups):
        self.device = dev = _args.indexed_device(_TAG, "a ViewStore", device)
        if len(groups) > _lib.VIEWS_MAX_GROUPS:
            raise ValueError("%s: %d groups; a store takes at most %d" % (_TAG, len(groups), _lib.VIEWS_MAX_GROUPS))
        self.names = tuple(groups)
        parts, V = [], None
        for name, data in groups.items():
            kind = "u8" if isinstance(data, u8) else "f32"
            rows, shape = _group_rows(data.data if kind == "u8" else data, name, np.uint8 if kind == "u8" else np.float32)
            chw = (shape[2], shape[0], shape[1]) if kind == "u8" else shape
            if kind == "u8" and chw[0] > 4:
                raise ValueError("%s: %s has %d channels; a u8 group takes at most 4" % (_TAG, name, chw[0]))
            parts.append((name, kind, chw, rows))
            V = len(rows) if V is None else V
            if len(rows) != V:
                raise RuntimeError("%s: %s has %d views, %s has %d" % (_TAG, name, len(rows), self.names[0], V))
        record = None if record is None else _host(record, "record", np.float32)
        ints = None if ints is None else _host(ints, "ints", np.int32)
        for t, name in ((record, "record"), (ints, "ints")):
            if t is None:
                continue
            if t.ndim != 2:
                raise RuntimeError("%s: %s must be [V, columns], got %s" % (_TAG, name, list(t.shape)))
            V = t.shape[0] if V is None else V
            if t.shape[0] != V:
                raise RuntimeError("%s: %s has %d rows for %d views" % (_TAG, name, t.shape[0], V))
        if not V:
            raise ValueError("%s: a store needs at least one view, and a record or a group" % _TAG)
        self.V = V = int(V)
        self.F = F = 0 if record is None else int(record.shape[1])
        self.J_user = 0 if ints is None else int(ints.shape[1])
        self.J = J = self.J_user + len(parts)                 # the caller's columns, then one `has` flag per group
        self._spec = tuple((kind,) + tuple(int(x) for x in chw) for _n, kind, chw, _r in parts)
        self.layout = L = layout(F, J, self._spec)
        if L is None:
            raise ValueError("%s: the views cannot be laid out (record %d + %d columns, groups %s)" % (_TAG, F, J, list(self._spec)))
        host = np.zeros((V, L.slab_bytes), np.uint8)
        if F:
            host[:, L.slab_record:L.slab_record + 4 * F] = record.view(np.uint8).reshape(V, 4 * F)
        if J:
            full = np.zeros((V, J), np.int32)
            if self.J_user:
                full[:, :self.J_user] = ints
            for g, (_n, _k, _s, rows) in enumerate(parts):
                full[:, self.J_user + g] = [r is not None for r in rows]
            at = L.slab_record + 4 * F
            host[:, at:at + 4 * J] = full.view(np.uint8).reshape(V, 4 * J)
        for g, (_n, _k, _s, rows) in enumerate(parts):
            for v, r in enumerate(rows):
                if r is not None:
                    host[v, L.slab_offsets[g]:L.slab_offsets[g] + r.nbytes] = r.reshape(-1).view(np.uint8)
        with _lib.on_device(dev):
            self.arena = torch.from_numpy(host).to(dev)
            self._current = torch.from_numpy(np.zeros((L.current_bytes,), np.uint8)).to(dev)
            # cursor, ticket: reset by a copy of `_zeros`, never by a memset
            self._zeros = torch.from_numpy(np.zeros((2,), np.int32)).to(dev)
            self._sched = self._zeros.clone()
        self._order = None
        self._kinds, self._C, self._H, self._W = (_ints([KINDS.index(s[0]) for s in self._spec]),) + tuple(
            _ints([s[k] for s in self._spec]) for k in (1, 2, 3))

        def words(at, count, dtype):
            return self._current[at:at + 4 * count].view(dtype)

        self.current = {name: words(L.current_offsets[g], chw[0] * chw[1] * chw[2], torch.float32).view(*chw)
                        for g, (name, _k, chw, _r) in enumerate(parts)}
        self.record = words(L.current_record, F, torch.float32)
        all_ints = words(L.current_record + 4 * F, J, torch.int32)
        self.ints = all_ints[:self.J_user]
        self._has = {name: all_ints[self.J_user + g:self.J_user + g + 1] for g, name in enumerate(self.names)}
        head = words(0, _lib.VIEWS_HEADER_BYTES // 4, torch.int32)
        self.index = head[_lib.VIEWS_INDEX_WORD:_lib.VIEWS_INDEX_WORD + 1]
        self.cursor_used = head[_lib.VIEWS_CURSOR_WORD:_lib.VIEWS_CURSOR_WORD + 1]
        self._cameras = None

    # ---- the draw ---------------------------------------------------------------------------------------------------------

    def draw(self, index=None):
        """Makes a view current: one launch on the current stream, nothing read on the host.  ``index``: the view, checked
        here (ValueError outside ``[0, V)``); None: the view ``order[cursor % N]`` of the schedule, which the launch advances
        by one (RuntimeError without a schedule).  Can be captured; draws from one schedule belong on one stream."""
        order = cursor = ticket = None
        if index is None:
            if self._order is None:
                raise RuntimeError("%s: draw() without an index draws from the schedule; call schedule(order) first" % _TAG)
            order, cursor, ticket = self._order.data_ptr(), self._sched.data_ptr(), self._sched.data_ptr() + 4
            index = 0
        else:
            index = int(index)
            if not 0 <= index < self.V:
                raise ValueError("%s: index %d is not in [0, %d)" % (_TAG, index, self.V))
        dev = self.device
        with _lib.on_device(dev):
            _lib.check(_lib.load().gft_views_draw(_lib.raw_stream(dev), self.F, self.J, len(self._spec), self._kinds, self._C, self._H,
                                                  self._W, self.arena.data_ptr(), self._current.data_ptr(), self.V, index, order, cursor,
                                                  0 if order is None else int(self._order.numel()), ticket))
        return self

    def schedule(self, order):
        """Uploads the view order ``draw()`` follows cyclically (a sequence of indices, ValueError if empty or if any lies
        outside ``[0, V)``) and resets the cursor.  A schedule of another length needs a new capture: N is a launch argument."""
        order = np.asarray(order.detach().cpu().numpy() if isinstance(order, torch.Tensor) else order)
        if order.ndim != 1 or order.size == 0:
            raise ValueError("%s: the order must be a non-empty sequence of view indices, got shape %s" % (_TAG, list(order.shape)))
        if order.dtype.kind not in "iu":
            raise TypeError("%s: the order must hold integers, got %s" % (_TAG, order.dtype))
        if int(order.min()) < 0 or int(order.max()) >= self.V:
            raise ValueError("%s: the order holds indices outside [0, %d): min %d, max %d" % (_TAG, self.V, order.min(), order.max()))
        with _lib.on_device(self.device):
            new = torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(self.device)
            if self._order is not None and self._order.numel() == new.numel():
                self._order.copy_(new)                      # (the address a capture holds stays)
            else:
                self._order = new
            self._sched.copy_(self._zeros)
        return self

    def cursor(self):
        """The number of draws from the schedule since ``schedule()``: a blocking read, for tests and logs"""
        return int(self._sched[0].item())

    # ---- the current view ---------------------------------------------------------------------------------------------------

    def has(self, name):
        """int32 [1]: 1 when the current view has the group ``name``, 0 when its image was None (the group is zeros then)"""
        return self._has[name]

    def _named(self, what):
        if self._cameras is None:
            raise RuntimeError("%s: %s belongs to a store built by ViewStore.from_cameras" % (_TAG, what))

    def camera(self, which="color"):
        """The current view's ``"color"`` or ``"tof"`` camera: ``world_view_transform`` [4, 4], ``full_proj_transform`` [4, 4]
        and ``camera_center`` [3], in the reference's (transposed) layout"""
        self._named("camera()")
        return self._cameras[which]

    time = property(lambda self: self._rec("time", REC_TIME, 1))
    times = property(lambda self: self._rec("times", REC_TIMES, 4))
    combine = property(lambda self: self._rec("combine", REC_COMBINE, 16).view(4, 4))
    depth_range = property(lambda self: self._rec("depth_range", REC_DEPTH_RANGE, 1))
    phase_offset = property(lambda self: self._rec("phase_offset", REC_PHASE_OFFSET, 1))
    dc_offset = property(lambda self: self._rec("dc_offset", REC_DC_OFFSET, 1))
    frame_id = property(lambda self: self._int("frame_id", INT_FRAME))
    quad = property(lambda self: self._int("quad", INT_QUAD))
    K = property(lambda self: self._int("K", INT_K))
    M = property(lambda self: self._int("M", INT_M))

    def _rec(self, what, at, count):
        self._named(what)
        return self.record[at:at + count]

    def _int(self, what, at):
        self._named(what)
        return self.ints[at:at + 1]

    # ---- the reference's cameras ------------------------------------------------------------------------------------------

    @classmethod
    def from_cameras(cls, cams, device, total_num_views=None, sync=False, flow_window=True, color="u8"):
        """The store of ``ToFCamera`` objects (``scene/cameras.py``), duck-typed: ``world_view_transform``,
        ``full_proj_transform``, ``camera_center`` and their ``_tof`` twins, ``frame_id``, ``depth_range``, ``phase_offset``,
        ``dc_offset`` and the images ``original_image`` (group ``color``), ``original_tof_image`` (``phasor``),
        ``original_tofQuad_im`` (``quad``), ``original_distance_image`` (``distance``), ``forward_flow``, ``backward_flow``; an
        image no camera has gives no group, one some lack is zeros there with ``has(name) == 0``.

        The record: the colour camera's block at float ``REC_COLOR`` and the ToF camera's at ``REC_TOF`` (view 16, proj 16,
        camera centre 3 + 1 pad), ``time = frame_id / (total_num_views - 1)`` (``train.py:167``), the three scalars, and
        ``times[4]`` and ``combine[4][4]``, zero-padded, of ``query.ftorf_schedule(frame_id, total_num_views, sync,
        forward_flow is not None and flow_window, backward_flow is not None and flow_window)``; the ints: ``frame_id``,
        ``frame_id % 4`` (``quad``), K and M of that schedule.  ``total_num_views``: ``dataset.total_num_views``, by default
        the number of cameras.  ``sync``: ``iteration <= opt.optimize_sync_iters``; ``flow_window``: ``iteration >
        opt.flow_loss_iter_start`` -- a run that crosses either builds a store per phase, as it captures a graph per phase.
        ``color="u8"`` keeps the colour image as the bytes it was read from, a quarter of the float planes, and raises
        ValueError for an image that is not ``byte / 255.0`` exactly; ``"f32"`` keeps the floats."""
        cams = list(cams)
        if not cams:
            raise ValueError("%s: no cameras" % _TAG)
        if color not in KINDS:
            raise ValueError("%s: color must be \"u8\" or \"f32\", got %r" % (_TAG, color))
        V = len(cams)
        total = V if total_num_views is None else int(total_num_views)
        if total < 2:
            raise ValueError("%s: total_num_views must be at least 2 (the time is frame_id / (total_num_views - 1)), got %d" % (_TAG, total))
        rec = np.zeros((V, REC_FLOATS), np.float32)
        ints = np.zeros((V, INT_COUNT), np.int32)

        def arr(t):
            return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float32, copy=False)

        for v, cam in enumerate(cams):
            for at, tail in ((REC_COLOR, ""), (REC_TOF, "_tof")):
                rec[v, at:at + 16] = arr(getattr(cam, "world_view_transform" + tail)).reshape(16)
                rec[v, at + 16:at + 32] = arr(getattr(cam, "full_proj_transform" + tail)).reshape(16)
                rec[v, at + 32:at + 35] = arr(getattr(cam, "camera_center" + tail)).reshape(3)
            f = int(cam.frame_id)
            rec[v, REC_TIME] = cam.frame_id / (total - 1)
            for at, name in ((REC_DEPTH_RANGE, "depth_range"), (REC_PHASE_OFFSET, "phase_offset"), (REC_DC_OFFSET, "dc_offset")):
                rec[v, at] = arr(getattr(cam, name)).reshape(-1)[0]
            times, comb, _names = ftorf_schedule(f, total, sync, getattr(cam, "forward_flow", None) is not None and flow_window,
                                                 getattr(cam, "backward_flow", None) is not None and flow_window)
            rec[v, REC_TIMES:REC_TIMES + len(times)] = times
            for m, row in enumerate(comb):
                rec[v, REC_COMBINE + 4 * m:REC_COMBINE + 4 * m + len(row)] = row
            ints[v] = (f, f % 4, len(times), len(comb))
        groups = {}
        for name, attr in CAMERA_GROUPS:
            images = [getattr(cam, attr, None) for cam in cams]
            if all(i is None for i in images):
                continue
            images = [None if i is None else arr(i) for i in images]
            if name == "color" and color == "u8":
                as_bytes = []
                for v, i in enumerate(images):
                    if i is None:
                        as_bytes.append(None)
                        continue
                    b = np.clip(np.rint(i * np.float32(255.0)), 0, 255).astype(np.uint8)
                    if not np.array_equal(b.astype(np.float32) / np.float32(255.0), i):
                        raise ValueError("%s: original_image of camera %d is not byte / 255.0 exactly; build the store with "
                                         "color=\"f32\"" % (_TAG, v))
                    as_bytes.append(np.ascontiguousarray(b.transpose(1, 2, 0)))
                groups[name] = u8(as_bytes)
            else:
                groups[name] = images
        self = cls(device, record=rec, ints=ints, **groups)
        r = self.record
        self._cameras = {which: Camera(r[at:at + 16].view(4, 4), r[at + 16:at + 32].view(4, 4), r[at + 32:at + 35])
                         for which, at in (("color", REC_COLOR), ("tof", REC_TOF))}
        return self


# ---- select_plane -----------------------------------------------------------------------------------------------------------

def _plane_call(fn, C_, plane, src, index, table, modulo, dst, dev):
    index_dev = index if isinstance(index, torch.Tensor) else None
    with _lib.on_device(dev):
        _lib.check(fn(_lib.raw_stream(dev), C_, plane, src.data_ptr(), 0 if index_dev is not None else index, _args.ptr(index_dev),
                      modulo, _args.ptr(table), 0 if table is None else int(table.numel()), dst.data_ptr()))


class _SelectPlane(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, index, table, modulo):
        dev = x.device
        C_, H, W = (int(s) for s in x.shape)
        out = torch.empty((1, H, W), device=dev, dtype=torch.float32)
        _plane_call(_lib.load().gft_views_select_plane, C_, H * W, x.detach(), index, table, modulo, out, dev)
        ctx.call = (C_, H, W, index, table, modulo, dev)
        return out

    @staticmethod
    def backward(ctx, g_out):
        C_, H, W, index, table, modulo, dev = ctx.call
        g_x = torch.empty((C_, H, W), device=dev, dtype=torch.float32)
        _plane_call(_lib.load().gft_views_select_plane_backward, C_, H * W, g_out.float().contiguous(), index, table, modulo, g_x, dev)
        return g_x, None, None, None


def select_plane(x, index, table=None, modulo=None):
    """``x[p].unsqueeze(0)`` with ``p = table[i]`` (or ``i`` without a table) and ``i = index % modulo`` (or ``index``), read
    when the kernel runs: one launch, and one for the backward, which writes the whole gradient of ``x`` -- the plane, and
    zeros.  ``x``: contiguous float32 ``[C, H, W]`` on the device (``phasor[3:]`` serves); ``index``: a Python int (checked
    here: ValueError outside the table, or outside ``[0, C)`` without one) or an int32 device tensor of one element, whose
    value the kernel clamps into range; ``table``: None or an int32 device tensor ``[T]``, likewise clamped to ``[0, C)``;
    ``modulo``: None or a positive int.  The gradient goes to ``x`` only."""
    x_d = _args.tensor(_TAG, x, "x")
    if x_d.dim() != 3 or min(x_d.shape) < 1:
        raise RuntimeError("%s: x must be [C, H, W] and not empty, got %s" % (_TAG, list(x_d.shape)))
    if not x_d.is_contiguous():
        raise RuntimeError("%s: x must be contiguous (a slice along its first dimension is)" % _TAG)
    named = [(x_d, "x")]
    for t, name in ((index, "index"), (table, "table")):
        if isinstance(t, torch.Tensor):
            if t.requires_grad:
                raise NotImplementedError("%s: gradients flow to x only; %s requires grad" % (_TAG, name))
            if t.dtype != torch.int32:
                raise TypeError("%s: %s must be torch.int32, got %s" % (_TAG, name, t.dtype))
            named.append((t, name))
    if table is not None:
        if not isinstance(table, torch.Tensor):
            raise TypeError("%s: table must be an int32 device tensor or None, got %s" % (_TAG, type(table).__name__))
        if table.dim() != 1 or table.numel() < 1 or not table.is_contiguous():
            raise RuntimeError("%s: table must be a contiguous [T] tensor, got %s" % (_TAG, list(table.shape)))
    if modulo is not None and int(modulo) < 1:
        raise ValueError("%s: modulo must be positive, got %d" % (_TAG, modulo))
    modulo = 0 if modulo is None else int(modulo)
    if isinstance(index, torch.Tensor):
        if index.numel() != 1:
            raise RuntimeError("%s: index must be a Python int or a one-element tensor, got %s" % (_TAG, list(index.shape)))
    else:
        index = int(index)
        i = index % modulo if modulo else index
        limit = int(table.numel()) if table is not None else int(x_d.shape[0])
        if not 0 <= i < limit:
            raise ValueError("%s: index %d%s is not in [0, %d)" % (_TAG, index, " %% %d" % modulo if modulo else "", limit))
    _args.devices(_TAG, "view", named)
    return _SelectPlane.apply(x, index, table, modulo)


# ---- the draw order ---------------------------------------------------------------------------------------------------------

class DrawOrder:
    """The reference's draw of the iteration's view (``train.py:155-163``), pure Python: a stack of all views, refilled when
    empty; ``pop(randint(0, len - 1))``; drawn again -- refilling inside the loop -- while the view's ``frame_id`` is below
    ``start_id``.  ``frame_ids[v]``: the ``frame_id`` of training camera v in the order of ``scene.getTrainCameras()``;
    ``rng``: anything with ``randint(a, b)`` (the ``random`` module by default, as ``train.py`` uses it).  ValueError if no
    view has ``frame_id >= start_id``, where the reference would never leave the loop."""

    def __init__(self, frame_ids, start_id=0, rng=random):
        self.frame_ids = list(frame_ids)
        self.start_id = start_id
        self.rng = rng
        if not any(f >= start_id for f in self.frame_ids):
            raise ValueError("%s: no view has frame_id >= start_id = %s; the reference's draw would never end" % (_TAG, start_id))
        self._stack = []

    def _pop(self):
        if not self._stack:
            self._stack = list(range(len(self.frame_ids)))
        return self._stack.pop(self.rng.randint(0, len(self._stack) - 1))

    def next(self, n=1):
        """The next ``n`` view indices; the stack is kept between calls, so any split of a run gives the same order"""
        out = []
        for _ in range(int(n)):
            v = self._pop()
            while self.frame_ids[v] < self.start_id:
                v = self._pop()
            out.append(v)
        return out
