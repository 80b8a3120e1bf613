"""The input point cloud on the device (``csrc/k_pcd.hip``, ``include/gftorf_pcd.h``): ToF frames to world points, the cloud's
PLY file and the model's first tensors.

The reference turns ToF frames into points with one block of numpy statements in three places (the phase initialisation of a
ToRF scene, ``scene/dataset_readers.py:530-586``, of an F-ToRF scene, ``:904-973``, and the proxy clouds of the render
programme, ``:1067-1118``), writes them with ``storePly`` (``:127-150``: one Python tuple per point), reads them back with
``fetchPly`` (``:110-125``) and builds the model with ``GaussianModel.create_from_pcd`` (``scene/gaussian_model.py:180-236``:
about forty eager launches around ``distCUDA2``).  Here:

``unproject(tof_image, stride, znear, FovX_tof, FovY_tof, world_view, depth_range, phase_offset, mode, ...)``  one launch per
    frame: the grid pixels' world points (float32, what ``storePly``'s ``f4`` columns keep), the distance used and the
    amplitude-derived values of the mode.  ``mode``: ``"torf_init"`` (the grid twice; the reference's statement that should
    shift the second half slices an empty range, so both halves are equal), ``"ftorf_init"`` (the unwrapping rule of
    ``:929-946``) or ``"proxy"`` (the second half from a rendered depth image).
``store(path, xyz, colors, phases, amplitudes, seg_colors)`` / ``submit_store(...)``  ``storePly``'s file: the header, then
    rows of 27, 30, 35 or 38 bytes packed by one launch and streamed through ``gftorf_amd.ply``'s pinned double buffer.
``fetch(path)``  ``fetchPly``: a ``Cloud`` of device tensors.
``create_tensors(cloud, ...)`` / ``create_from_pcd(model, cloud, cameras_extent, scene_extent, args)``  the model's tensors by
    one launch behind ``distCUDA2``.
``phase_init_torf``, ``phase_init_ftorf``, ``proxy_clouds``  the three reader blocks: unproject, store, and the cloud
    ``fetchPly`` would read back, without reading it back.

Precisions.  The distance is numpy's float32 ``depth_from_tof``; everything behind it is float64 as numpy evaluates it, with
``np.square`` of a float32 distance a float32 product.  The reference inverts the float32 view matrix in float32 (LAPACK);
the kernel inverts the same 16 values in float64, which no float32 routine's roundings can be matched against and which is
the closer of the two to the matrix's true inverse.  The F-ToRF amplitude test ``tof_image[h, w, 2] < 0.04`` compares a
float32 scalar with a Python float, which the reference's numpy (1.x) does in float64: ``float32(0.04)`` is below 0.04.  The
candidate test ``znear < z_i <= 10.5`` (:933) compares a one-element float32 *array* with Python floats, which numpy 1.x and 2
alike do in float32, so the kernel compares with ``float(znear)``: both choices follow numpy's rules and neither is an oversight.

The ``u1`` columns.  ``storePly`` assigns Python floats to ``uint8`` fields.  numpy converts each with ``int(v)``, which
truncates towards zero, and then checks the range: a value in (-1, 256) becomes its truncation; any other number, the
infinities included, raises ``OverflowError`` and a NaN ``ValueError`` (recorded with numpy 2.2).  ``store`` does the same: it raises
the same exception, naming the count, and writes no file.

There is no CPU path.
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np
import torch

from . import _args, _lib, ply

_TAG = "gftorf_amd.pcd"
C0 = 0.28209479177387814                        # utils/sh_utils.py:26
MODES = _lib.PCD_MODES
FTORF_FAR = 10.5                                # dataset_readers.py:933

# BasicPointCloud's fields (utils/graphics_utils.py:18-24) as fetchPly fills them: points, normals [P, 3] float32; colors,
# seg_colors [P, 3] float64 (u1 / 255.0); phases, amplitudes [P, 1] float32; the optional ones None
Cloud = namedtuple("Cloud", ("points", "normals", "colors", "phases", "amplitudes", "seg_colors"))


def grid(H, W, stride=1):
    """(H', W') = (ceil(H / stride), ceil(W / stride))"""
    s = int(stride)
    if s < 1:
        raise ValueError("%s: stride must be at least 1, got %s" % (_TAG, stride))
    return (int(H) + s - 1) // s, (int(W) + s - 1) // s


def frame_rows(mode, H, W, stride=1):
    """rows one frame adds in ``mode``"""
    if mode not in MODES:
        raise ValueError("%s: mode must be one of %s, got %r" % (_TAG, ", ".join(MODES), mode))
    Hp, Wp = grid(H, W, stride)
    return Hp * Wp * (1 if mode == "ftorf_init" else 2)


# ---- the file's text side (pure Python) -------------------------------------------------------------------------------------

def properties(has_phasor=True, has_seg=True):
    """The vertex properties of ``storePly``'s file in order, in the form ``gftorf_amd.ply.header`` takes"""
    props = ["x", "y", "z", "nx", "ny", "nz", ("red", "uchar"), ("green", "uchar"), ("blue", "uchar")]
    if has_phasor:
        props += ["phase", "amplitude"]
    if has_seg:
        props += [("seg_red", "uchar"), ("seg_green", "uchar"), ("seg_blue", "uchar")]
    return props


def row_layout(props):
    """({name: (byte offset, type)}, bytes of a row) of properties in the form ``properties`` / ``parse_header`` give"""
    at, out = 0, {}
    for p in props:
        name, kind = (p, "float") if isinstance(p, str) else p
        out[name] = (at, kind)
        at += ply.PROPERTY_BYTES[kind]
    return out, at


def header(P, has_phasor=True, has_seg=True):
    """The header ``plyfile`` writes for ``storePly``'s dtype list, as bytes"""
    return ply.header(properties(has_phasor, has_seg), P)


_FIELD_KINDS = tuple("uchar" if n in ("red", "green", "blue", "seg_red", "seg_green", "seg_blue") else "float" for n in _lib.PCD_FIELDS)


def field_offsets(props):
    """gft_pcd_unpack's table: the byte offset of every field of ``_lib.PCD_FIELDS`` in a row of ``props``, -1 for one fetchPly
    does not read from this file (phase and amplitude only together, the seg colours only all three), and the row's bytes"""
    layout, row_bytes = row_layout(props)
    for name in _lib.PCD_FIELDS[:9]:
        if name not in layout:
            raise ValueError("%s: the file has no property `%s`, which fetchPly reads" % (_TAG, name))
    groups = (("phase", "amplitude"), ("seg_red", "seg_green", "seg_blue"))
    absent = {n for g in groups if not all(m in layout for m in g) for n in g}
    offsets = []
    for name, kind in zip(_lib.PCD_FIELDS, _FIELD_KINDS):
        if name in absent:
            offsets.append(-1)
            continue
        if layout[name][1] != kind:
            raise NotImplementedError("%s: the property `%s` is %s, storePly writes it as %s" % (_TAG, name, layout[name][1], kind))
        offsets.append(layout[name][0])
    return offsets, row_bytes


# ---- unproject --------------------------------------------------------------------------------------------------------------

_POINT_KEYS = ("amp", "sh_color", "color", "sh_amp", "amplitude")


def alloc_points(rows, device, mode="torf_init", wide=False):
    """The output tensors of ``rows`` points for ``unproject(out=...)``: ``xyz`` [rows, 3], ``dist`` [rows] (float64 for a
    proxy cloud from a float64 rendered image: ``wide``) and, except in proxy mode, ``amp``, ``sh_color``, ``sh_amp``,
    ``amplitude`` [rows] and ``color`` [rows, 3]"""
    f32 = dict(device=device, dtype=torch.float32)
    out = {"xyz": torch.empty((rows, 3), **f32), "dist": torch.empty((rows,), device=device, dtype=torch.float64 if wide else torch.float32)}
    if mode != "proxy":
        out.update({k: torch.empty((rows, 3) if k == "color" else (rows,), **f32) for k in _POINT_KEYS})
    return out


def _launch_unproject(tof_image, stride, znear, FovX_tof, FovY_tof, world_view, depth_range, phase_offset, mode, rendered, out, row,
                      status):
    tof = _args.tensor(_TAG, tof_image, "tof_image")
    if tof.dim() != 3 or tof.shape[2] != 3 or tof.shape[0] < 1 or tof.shape[1] < 1:
        raise RuntimeError("%s: tof_image must be [H, W, 3], got %s" % (_TAG, list(tof.shape)))
    tof = tof.contiguous()
    H, W = int(tof.shape[0]), int(tof.shape[1])
    rows = frame_rows(mode, H, W, stride)
    named = [(tof, "tof_image")]
    wide = False
    if mode == "proxy":
        rendered = _args.tensor(_TAG, rendered, "rendered", (torch.float32, torch.float64))
        if tuple(rendered.shape) != (H, W):
            raise RuntimeError("%s: rendered must be [%d, %d], got %s" % (_TAG, H, W, list(rendered.shape)))
        rendered = rendered.contiguous()
        wide = rendered.dtype == torch.float64
        named.append((rendered, "rendered"))
    elif rendered is not None:
        raise ValueError("%s: rendered belongs to the proxy mode" % _TAG)
    dr_dev, dr = _args.scalar(_TAG, depth_range, "depth_range", named)
    po_dev, po = _args.scalar(_TAG, phase_offset, "phase_offset", named)
    if out is None:
        out, row = alloc_points(rows, tof.device, mode, wide), 0
    row = int(row)
    views = {}
    for key in ("xyz", "dist") + (() if mode == "proxy" else _POINT_KEYS):
        t = out[key]
        want = torch.float64 if key == "dist" and wide else torch.float32
        if t.dtype != want or not t.is_contiguous() or row < 0 or row + rows > t.shape[0] or t.dim() != (2 if key in ("xyz", "color") else 1):
            raise RuntimeError("%s: out[%r] must be a contiguous %s tensor with rows %d .. %d" % (_TAG, key, want, row, row + rows - 1))
        views[key] = t[row:row + rows]
        named.append((t, "out[%r]" % key))
    dev = _args.devices(_TAG, "point cloud", named)
    view = np.ascontiguousarray(np.asarray(world_view.cpu() if isinstance(world_view, torch.Tensor) else world_view, dtype=np.float64))
    if view.shape != (4, 4):
        raise RuntimeError("%s: world_view must be the 4 x 4 world-to-view matrix, got %s" % (_TAG, list(view.shape)))
    znear = float(znear)
    width_m = float(znear * np.tan(float(FovX_tof) / 2.0) * 2.0)                 # :552-553
    height_m = float(znear * np.tan(float(FovY_tof) / 2.0) * 2.0)
    lib = _lib.load()
    with _lib.on_device(dev):
        _lib.check(lib.gft_pcd_unproject(
            _lib.raw_stream(dev), MODES.index(mode), H, W, int(stride), tof.data_ptr(), _args.ptr(rendered) if mode == "proxy" else None,
            int(wide), view.ctypes.data_as(C.POINTER(C.c_double)), width_m, height_m, znear, _args.ptr(dr_dev), dr, _args.ptr(po_dev), po,
            views["xyz"].data_ptr(), views["dist"].data_ptr(), *[_args.ptr(views.get(k)) for k in _POINT_KEYS], _args.ptr(status)))
    return views


def unproject(tof_image, stride, znear, FovX_tof, FovY_tof, world_view, depth_range, phase_offset=0.0, mode="torf_init",
              rendered=None, out=None, row=0):
    """The grid pixels of one ToF frame as world points: one launch on the current stream.

    ``tof_image`` [H, W, 3] float32 on the device, read in place; the grid is ``grid(H, W, stride)``.  ``world_view``: the
    4 x 4 world-to-view matrix of the ToF sensor (``getWorld2View2(R_tof, T_tof)``), host values.  ``depth_range`` and
    ``phase_offset``: numbers, or one-element float32 device tensors read by the kernel.  ``rendered`` [H, W] float32 or
    float64 (proxy mode).  With ``out`` (``alloc_points``) the frame's rows are written from row ``row`` on, so a frame list
    is a loop of launches into one output; the returned dict holds the frame's views of it.

    Nothing is read on the host in the ``torf_init`` and ``proxy`` modes.  ``ftorf_init`` reads one status block and raises
    ValueError where the reference would raise (a pixel with no distance candidate in (znear, 10.5], or the reference's own
    amplitude index outside the image), naming the counts."""
    if mode != "ftorf_init":
        return _launch_unproject(tof_image, stride, znear, FovX_tof, FovY_tof, world_view, depth_range, phase_offset, mode, rendered, out,
                                 row, None)
    if not isinstance(tof_image, torch.Tensor):
        raise TypeError("%s: tof_image must be a tensor, got %s" % (_TAG, type(tof_image).__name__))
    status = torch.zeros((_lib.PCD_STATUS_WORDS,), device=tof_image.device, dtype=torch.int32)
    views = _launch_unproject(tof_image, stride, znear, FovX_tof, FovY_tof, world_view, depth_range, phase_offset, mode, rendered, out,
                              row, status)
    empty, outside = (int(v) for v in status.cpu())
    if empty or outside:
        raise ValueError("%s: ftorf_init: %d pixel(s) with no distance candidate in (znear, %s] and %d whose amplitude index lies "
                         "outside the image; the reference raises IndexError there" % (_TAG, empty, FTORF_FAR, outside))
    return views


# ---- store ------------------------------------------------------------------------------------------------------------------

def _rows3(t, name, P, named):
    t = _args.tensor(_TAG, t, name, (torch.float32, torch.float64))
    if tuple(t.shape) != (P, 3):
        raise RuntimeError("%s: %s must be [%d, 3], got %s" % (_TAG, name, P, list(t.shape)))
    t = t.contiguous()
    named.append((t, name))
    return t


def _column(t, name, P, named):
    t = _args.tensor(_TAG, t, name, (torch.float32, torch.float64))
    if t.numel() != P or t.dim() not in (1, 2):
        raise RuntimeError("%s: %s must be [%d, 1], got %s" % (_TAG, name, P, list(t.shape)))
    t = t.reshape(P).to(torch.float32).contiguous()          # the f4 column's rounding
    named.append((t, name))
    return t


class StoreJob:
    """The packed rows of one ``submit_store``, held in a device buffer until ``finish`` has written them.  ``cloud``: what
    ``fetch`` would read back from the file (``want_cloud``), else None."""

    def __init__(self, path, head, body, nbytes, status, event, device, cloud):
        self.path, self.cloud = path, cloud
        self._head, self._body, self._nbytes, self._status, self._event, self._device = head, body, nbytes, status, event, device
        self._done = False

    def finish(self, chunk_bytes=None):
        """Reads the status block (ValueError / OverflowError for colours ``storePly`` would raise on: no file is written),
        then writes the header and streams the body in chunks through two pinned buffers, the copy of chunk i + 1 running while
        chunk i is written.  Waits for the device; a second call does nothing."""
        if self._done:
            return
        self._done = True
        body, nbytes = self._body, self._nbytes
        self._body = None
        with _lib.on_device(self._device):
            stream = torch.cuda.current_stream(self._device)
            stream.wait_event(self._event)
            if self._status is not None:
                numbers, other = (int(v) for v in self._status.cpu())
                if numbers:
                    raise OverflowError("%s: %d colour value(s) outside (-1, 256): out of bounds for uint8" % (_TAG, numbers))
                if other:
                    raise ValueError("%s: %d colour value(s) are NaN: cannot convert float NaN to integer" % (_TAG, other))
            step = max(4, int(chunk_bytes) if chunk_bytes is not None else ply.CHUNK_BYTES)
            bounds = [(a, min(a + step, nbytes)) for a in range(0, nbytes, step)]
            host, events = ply._stage(step)

            def copy(i):
                a, b = bounds[i]
                host[i & 1][:b - a].copy_(body[a:b], non_blocking=True)
                events[i & 1].record(stream)

            folder = os.path.dirname(self.path)
            if folder:
                os.makedirs(folder, exist_ok=True)
            with open(self.path, "wb") as f:
                f.write(self._head)
                if bounds:
                    copy(0)
                for i, (a, b) in enumerate(bounds):
                    if i + 1 < len(bounds):
                        copy(i + 1)
                    events[i & 1].synchronize()
                    f.write(memoryview(host[i & 1].numpy())[:b - a])


def submit_store(path, xyz, colors, phases=None, amplitudes=None, seg_colors=None, want_cloud=False):
    """``storePly``'s rows formed in a device buffer by one launch on the current stream; returns a ``StoreJob`` whose
    ``finish`` writes the file.  Nothing is read on the host and nothing is waited for here.  ``xyz`` [P, 3]; ``colors`` and
    ``seg_colors`` [P, 3], already multiplied by 255, float32 or float64; ``phases`` and ``amplitudes`` [P, 1] (written only
    when both are given, as ``storePly`` does).  Device memory: the file's body, 27 to 38 bytes per point, until ``finish``."""
    xyz = _args.tensor(_TAG, xyz, "xyz", (torch.float32, torch.float64))
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError("%s: xyz must be [P, 3], got %s" % (_TAG, list(xyz.shape)))
    P = int(xyz.shape[0])
    xyz = xyz.to(torch.float32).contiguous()
    named = [(xyz, "xyz")]
    colors = _rows3(colors, "colors", P, named)
    has_pa = phases is not None and amplitudes is not None
    if has_pa:
        phases, amplitudes = _column(phases, "phases", P, named), _column(amplitudes, "amplitudes", P, named)
    seg = None if seg_colors is None else _rows3(seg_colors, "seg_colors", P, named)
    dev = _args.devices(_TAG, "point cloud", named)
    lib = _lib.load()
    nbytes = P * lib.gft_pcd_row_bytes(int(has_pa), int(seg is not None))
    body = torch.empty(((nbytes + 3) // 4 * 4 + 4,), device=dev, dtype=torch.uint8)
    status = torch.zeros((_lib.PCD_STATUS_WORDS,), device=dev, dtype=torch.int32)
    back = seg_back = None
    if want_cloud:
        back = torch.empty((P, 3), device=dev, dtype=torch.float64)
        seg_back = None if seg is None else torch.empty((P, 3), device=dev, dtype=torch.float64)
    with _lib.on_device(dev):
        _lib.check(lib.gft_pcd_pack(_lib.raw_stream(dev), P, xyz.data_ptr(), colors.data_ptr(), int(colors.dtype == torch.float64),
                                    _args.ptr(phases) if has_pa else None, _args.ptr(amplitudes) if has_pa else None, _args.ptr(seg),
                                    int(seg is not None and seg.dtype == torch.float64), body.data_ptr(), _args.ptr(back),
                                    _args.ptr(seg_back), status.data_ptr()))
        event = torch.cuda.Event()
        event.record()
    cloud = None
    if want_cloud:
        cloud = Cloud(xyz, torch.zeros_like(xyz), back, phases.reshape(P, 1) if has_pa else None,
                      amplitudes.reshape(P, 1) if has_pa else None, seg_back)
    return StoreJob(path, header(P, has_pa, seg is not None), body, nbytes, status, event, dev, cloud)


def store(path, xyz, colors, phases=None, amplitudes=None, seg_colors=None, chunk_bytes=None):
    """``storePly(path, xyz, colors, phases, amplitudes, seg_colors)``"""
    submit_store(path, xyz, colors, phases, amplitudes, seg_colors).finish(chunk_bytes=chunk_bytes)


# ---- fetch ------------------------------------------------------------------------------------------------------------------

def fetch(path, device=None, chunk_rows=None):
    """``fetchPly(path)`` as a ``Cloud`` of device tensors: the positions, normals and phasor columns are the file's float32
    bits, the colours ``u1 / 255.0`` in float64 as numpy forms them.  Properties are found by name in any order; ``phases`` and
    ``amplitudes`` are None unless the file has both, ``seg_colors`` unless it has all three.  The body is streamed in chunks
    of ``chunk_rows`` through two pinned buffers; one launch per chunk scatters it."""
    dev = _args.indexed_device(_TAG, "a fetched cloud", device)
    lib = _lib.load()
    with open(path, "rb") as f:
        head = b""
        while b"end_header\n" not in head and len(head) < (1 << 20):
            piece = f.read(1 << 16)
            if not piece:
                break
            head += piece
        P, props, offset = ply.parse_header(head, uchar=True)
        offsets, row_bytes = field_offsets(props)
        if row_bytes > _lib.PCD_MAX_ROW_BYTES:
            raise ValueError("%s: the file has %d bytes per vertex; the loader takes at most %d" % (_TAG, row_bytes, _lib.PCD_MAX_ROW_BYTES))
        has_pa, has_seg = offsets[9] >= 0, offsets[11] >= 0
        f32, f64 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.float64)
        cloud = Cloud(torch.empty((P, 3), **f32), torch.empty((P, 3), **f32), torch.empty((P, 3), **f64),
                      torch.empty((P, 1), **f32) if has_pa else None, torch.empty((P, 1), **f32) if has_pa else None,
                      torch.empty((P, 3), **f64) if has_seg else None)
        table = (C.c_int32 * len(offsets))(*offsets)
        rows = max(1, int(chunk_rows) if chunk_rows is not None else ply.CHUNK_BYTES // row_bytes)
        room = (rows * row_bytes + 3) // 4 * 4                              # the kernel reads whole dwords
        f.seek(offset)
        with _lib.on_device(dev):
            host, events = ply._stage(room)
            chunks = [torch.empty((room,), device=dev, dtype=torch.uint8) for _ in range(2 if P > rows else 1)] if P else []
            used = [False, False]
            for i, r0 in enumerate(range(0, P, rows)):
                slot, nrows = i & 1, min(rows, P - r0)
                nbytes = nrows * row_bytes
                if used[slot]:
                    events[slot].synchronize()                              # the copy out of this buffer two chunks ago
                got = f.readinto(memoryview(host[slot].numpy())[:nbytes])
                if got != nbytes:
                    raise ValueError("%s: %s ends inside vertex %d of %d" % (_TAG, path, r0 + (got or 0) // row_bytes, P))
                chunks[slot][:nbytes].copy_(host[slot][:nbytes], non_blocking=True)
                events[slot].record()
                used[slot] = True
                _lib.check(lib.gft_pcd_unpack(_lib.raw_stream(dev), nrows, r0, row_bytes, chunks[slot].data_ptr(), table,
                                              cloud.points.data_ptr(), cloud.normals.data_ptr(), cloud.colors.data_ptr(),
                                              _args.ptr(cloud.phases), _args.ptr(cloud.amplitudes), _args.ptr(cloud.seg_colors)))
            for slot in range(2):
                if used[slot]:
                    events[slot].synchronize()
    return cloud


# ---- create_from_pcd --------------------------------------------------------------------------------------------------------

def _mean_dist2(points, out):
    """``distCUDA2(points)`` written into ``out``: the halves of ``init_static_first`` fill one tensor"""
    P = int(points.shape[0])
    if P == 0:
        return
    lib, dev = _lib.load(), points.device
    scratch = torch.empty((lib.gft_knn_scratch_bytes(P),), device=dev, dtype=torch.uint8)
    _lib.check(lib.gft_knn_mean_dist2(_lib.raw_stream(dev), P, points.data_ptr(), out.data_ptr(), scratch.data_ptr()))


def create_tensors(cloud, max_sh_degree, isotropic=False, init_static_first=False, initial_opacity=0.1):
    """The tensors ``create_from_pcd`` builds from ``cloud`` (a ``Cloud``, or any object with BasicPointCloud's fields as
    device tensors), as a dict keyed by the model's attribute names, each in its final contiguous layout: ``_xyz``,
    ``_features_dc_color`` / ``_features_rest_color``, ``_scaling`` ([P, 1] when ``isotropic``, else [P, 3]), ``_rotation``,
    ``_opacity``, ``max_radii2D`` and, with their columns, ``_features_dc_phase`` / ``_features_rest_phase``,
    ``_features_dc_amp`` / ``_features_rest_amp`` and ``_features_seg_color``.  One ``distCUDA2`` call (two with
    ``init_static_first``: the halves ``[:P // 2]`` and ``[P // 2:]``), then one launch.  ``log(sqrt(clamp_min(dist2, 1e-7)))``
    and the one opacity value are torch's own elementwise kernels: with ``logf(sqrtf(.))`` in the kernel 22 % of 600 000
    ``_scaling`` values differed from torch's in the last place on an MI355X."""
    named = []
    xyz = _args.tensor(_TAG, cloud.points, "cloud.points", (torch.float32, torch.float64))
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError("%s: cloud.points must be [P, 3], got %s" % (_TAG, list(xyz.shape)))
    P = int(xyz.shape[0])
    xyz = xyz.to(torch.float32).contiguous()
    named.append((xyz, "cloud.points"))
    colors = _rows3(cloud.colors, "cloud.colors", P, named)
    phases = None if cloud.phases is None else _column(cloud.phases, "cloud.phases", P, named)
    amplitudes = None if cloud.amplitudes is None else _column(cloud.amplitudes, "cloud.amplitudes", P, named)
    seg = None if cloud.seg_colors is None else _rows3(cloud.seg_colors, "cloud.seg_colors", P, named)
    dev = _args.devices(_TAG, "point cloud", named)
    n = (int(max_sh_degree) + 1) ** 2 - 1
    cols = 1 if isotropic else 3
    f32 = dict(device=dev, dtype=torch.float32)
    out = {"_xyz": torch.empty((P, 3), **f32), "_features_dc_color": torch.empty((P, 1, 3), **f32),
           "_features_rest_color": torch.empty((P, n, 3), **f32), "_scaling": torch.empty((P, cols), **f32),
           "_rotation": torch.empty((P, 4), **f32), "_opacity": torch.empty((P, 1), **f32), "max_radii2D": torch.empty((P,), **f32)}
    if phases is not None:
        out.update(_features_dc_phase=torch.empty((P, 1, 1), **f32), _features_rest_phase=torch.empty((P, n, 1), **f32))
    if amplitudes is not None:
        out.update(_features_dc_amp=torch.empty((P, 1, 1), **f32), _features_rest_amp=torch.empty((P, n, 1), **f32))
    if seg is not None:
        out["_features_seg_color"] = torch.empty((P, 3), **f32)
    lib = _lib.load()
    with _lib.on_device(dev):
        dist2 = torch.empty((P,), **f32)
        for a, b in (((0, P // 2), (P // 2, P)) if init_static_first else ((0, P),)):
            _mean_dist2(xyz[a:b], dist2[a:b])
        log_scale = torch.log(torch.sqrt(torch.clamp_min(dist2, 0.0000001)))
        x = initial_opacity * torch.ones((1, 1), dtype=torch.float, device=dev)
        opacity = torch.log(x / (1 - x))                                        # utils/general_utils.py:19-20
        # torch's `t / C0` on the device is t times the reciprocal, formed in double and rounded to float: a property of torch's
        # division by a Python scalar that tests/test_pcd.py::test_create_tensors pins with torch.equal (GPU tests only)
        inv_c0 = float(np.float32(1.0 / C0))
        ptr = _args.ptr_nonempty
        _lib.check(lib.gft_pcd_create(
            _lib.raw_stream(dev), P, n, xyz.data_ptr(), colors.data_ptr(), int(colors.dtype == torch.float64), _args.ptr(phases),
            _args.ptr(amplitudes), _args.ptr(seg), int(seg is not None and seg.dtype == torch.float64), log_scale.data_ptr(),
            opacity.data_ptr(), inv_c0, cols, out["_xyz"].data_ptr(), out["_features_dc_color"].data_ptr(),
            ptr(out["_features_rest_color"]), ptr(out.get("_features_dc_phase")), ptr(out.get("_features_rest_phase")),
            ptr(out.get("_features_dc_amp")), ptr(out.get("_features_rest_amp")), out["_scaling"].data_ptr(),
            out["_rotation"].data_ptr(), out["_opacity"].data_ptr(), ptr(out.get("_features_seg_color")), out["max_radii2D"].data_ptr()))
    return out


# the model's parameters and the flag the reference hands `requires_grad_` before it wraps the tensor (`_rotation`: False when
# the Gaussians are isotropic).  nn.Parameter's own requires_grad=True then wins, there as here: every parameter takes a gradient
_GRAD = {"_xyz": True, "_features_dc_color": True, "_features_rest_color": True, "_scaling": True, "_opacity": True,
         "_features_dc_phase": True, "_features_rest_phase": True, "_features_dc_amp": True, "_features_rest_amp": True,
         "_features_seg_color": False}


def create_from_pcd(model, cloud, cameras_extent, scene_extent, args):
    """``GaussianModel.create_from_pcd(pcd, cameras_extent, scene_extent, args)``: the same attributes, ``requires_grad`` flags
    and zero offsets on ``model``.  ``args``: ``isotropic_gaussians``, ``init_static_first``, ``initial_opacity``."""
    model.isotropic = args.isotropic_gaussians
    model.cameras_extent = cameras_extent
    model.scene_extent = scene_extent
    t = create_tensors(cloud, model.max_sh_degree, isotropic=bool(model.isotropic), init_static_first=bool(args.init_static_first),
                       initial_opacity=args.initial_opacity)
    for name, grad in dict(_GRAD, _rotation=not model.isotropic).items():
        if name in t:
            setattr(model, name, torch.nn.Parameter(t[name].requires_grad_(grad)))
    model.max_radii2D = t["max_radii2D"]
    if "_features_dc_phase" in t:
        dev = t["_xyz"].device
        model._phase_offset = torch.nn.Parameter(torch.zeros((1,), device=dev).requires_grad_(True))
        model._dc_offset = torch.nn.Parameter(torch.zeros((1,), device=dev).requires_grad_(True))


# ---- the three reader blocks --------------------------------------------------------------------------------------------------

def _zero_phasor():
    """``SH2PA(PA2SH(np.zeros(..., float32)))``: one float32 value (:584-585)"""
    return float(((np.zeros((1,), np.float32) - 0.5) / C0 * C0 + 0.5)[0])


def _fill(rows, device, rgb):
    return torch.tensor(rgb, dtype=torch.float64, device=device).repeat(rows, 1)


def _init_frames(frames, stride, depth_range, phase_offset, mode):
    rows = [frame_rows(mode, f["tof_image"].shape[0], f["tof_image"].shape[1], stride) for f in frames]
    out = alloc_points(sum(rows), frames[0]["tof_image"].device, mode)
    at = 0
    for f, r in zip(frames, rows):
        unproject(f["tof_image"], stride, f["znear"], f["FovX_tof"], f["FovY_tof"], f["world_view"], depth_range, phase_offset,
                  mode=mode, out=out, row=at)
        at += r
    return out


def phase_init_torf(frames, stride, depth_range, phase_offset, path):
    """The phase initialisation of a ToRF scene (:530-593) from the frames it selects (``args.total_num_views // 2`` alone for a
    dynamic scene, else every training frame), each a dict with ``tof_image``, ``znear``, ``FovX_tof``, ``FovY_tof`` and
    ``world_view``: one launch per frame into one output, the file at ``path``, and the cloud ``fetchPly(path)`` reads."""
    out = _init_frames(frames, stride, depth_range, phase_offset, "torf_init")
    P, dev = out["xyz"].shape[0], out["xyz"].device
    phases = torch.full((P, 1), _zero_phasor(), device=dev, dtype=torch.float32)
    job = submit_store(path, out["xyz"], out["color"] * 255.0, phases, out["amplitude"], _fill(P, dev, (1.0, 0.0, 0.0)) * 255.0,
                       want_cloud=True)
    job.finish()
    return job.cloud


def phase_init_ftorf(frames, stride, depth_range, phase_offset, path):
    """The phase initialisation of an F-ToRF scene (:904-990) without ``init_static_dynamic_separation`` (whose random half is
    numpy's generator and stays with the caller): only ``frames[0]`` is used, as the reference's loop ends in ``break``; the
    colour columns are the seg colours.  ValueError where the reference raises; no file is written then."""
    out = _init_frames(frames[:1], stride, depth_range, phase_offset, "ftorf_init")
    P, dev = out["xyz"].shape[0], out["xyz"].device
    phases = torch.full((P, 1), _zero_phasor(), device=dev, dtype=torch.float32)
    seg = _fill(P, dev, (1.0, 0.0, 0.0)) * 255.0
    job = submit_store(path, out["xyz"], seg, phases, out["amplitude"], seg, want_cloud=True)
    job.finish()
    return job.cloud


def proxy_clouds(frames, depth_range, phase_offset, paths):
    """The proxy clouds of the render programme (:1067-1118): for frame i (a dict as ``phase_init_torf`` takes, with
    ``rendered``, the [H, W] depth image) the input frame's points, coloured red, then the rendered depth's, blue, at full
    sensor resolution, written to ``paths[i]``.  Yields each frame's cloud.  Two slots: frame i + 1's unproject and pack are
    queued before frame i's file is written, so the host never waits for a launch it has yet to make; frame i's copies to pinned
    memory run on the same stream behind those launches, so only their tenth of a millisecond is hidden and the device is idle
    while the host writes.  Both frames' packed bodies (38 bytes per point each) are resident at once."""
    z = _zero_phasor()
    pending = None
    for f, path in zip(frames, paths):
        pts = unproject(f["tof_image"], 1, f["znear"], f["FovX_tof"], f["FovY_tof"], f["world_view"], depth_range, phase_offset,
                        mode="proxy", rendered=f["rendered"])
        P, dev = pts["xyz"].shape[0], pts["xyz"].device
        colors = torch.cat([_fill(P // 2, dev, (1.0, 0.0, 0.0)), _fill(P // 2, dev, (0.0, 0.0, 1.0))]).to(torch.float32) * 255.0
        phasor = torch.full((P, 1), z, device=dev, dtype=torch.float32)
        job = submit_store(path, pts["xyz"], colors, phasor, phasor, torch.zeros((P, 3), device=dev, dtype=torch.float64), want_cloud=True)
        if pending is not None:
            pending.finish()
            yield pending.cloud
        pending = job
    if pending is not None:
        pending.finish()
        yield pending.cloud
