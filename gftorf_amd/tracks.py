"""The F-ToRF motion tracks on the device (``csrc/k_tracks.hip``, ``include/gftorf_tracks.h``).

The program the reference's README sends a user to, ``render_ftorf_viz_traj.py``, ends its ``render_set`` (``:262-347``) by
integrating the Gaussians' flow over the sequence, projecting every Gaussian into every view (``project_points_subset``,
``scene/torf_utils.py:108-114``), picking the Gaussians to draw with five quantiles and walking a Python double loop over
frames and drawn Gaussians that reads three single elements from the device per visit.  Here:

``sequence_flows(deform, xyz, frame_ids, denom)``  the network once per distinct integer frame of the sequence instead of
    twice per view (``:223-228``): the distinct flows, each frame's row of them, and ``d_xyz(t)``.
``integrate(...)``  the positions, projections, motion and mean depth of every Gaussian over the whole sequence, in one
    launch without a host read: it can be captured in a graph.
``select(tr, ...)``  the sampling mask of ``:278-290``, the reference's statements in torch on the device.
``table(tr, mask)``  the selected rows in one contiguous device buffer (one gather launch, one blocking count);
    ``TrackTable.to_host()`` is the sequence's one transfer.
``walk(table_host, ...)``  the greedy loop of ``:297-347`` in Python over the host copy; it never touches the device.

``pos_last`` and the world z behind ``mean_z`` are the reference's sequential float32 additions bit for bit; the projection is
a fixed float32 sequence, which a BLAS matmul is not, so ``xy`` agrees with the reference to rounding, not to the bit (see
DESIGN.md).  Nothing here has a gradient and there is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _args, _lib
from ._args import ptr as _ptr
from .query import DeformQuery

_TAG = "gftorf_amd.tracks"
BIG_BIG_MOTION_QUANTILE = 0.95          # render_ftorf_viz_traj.py:279


class Tracks:
    """What ``integrate`` returns, device tensors: ``xy`` [T, P, 2] (``all_2D_pos``), ``pos_last`` [P, 3], ``motion`` [P]
    (``mean_t sum_c flow[t]^2``, ``:278``), ``mean_z`` [P] (``mean_t`` of the world z of ``all_3D_pos``, ``:283``), ``step_ok``
    uint8 [T, P]; ``size`` = (H, W)."""

    def __init__(self, xy, pos_last, motion, mean_z, step_ok, size):
        self.xy, self.pos_last, self.motion, self.mean_z, self.step_ok, self.size = xy, pos_last, motion, mean_z, step_ok, size
        self.T, self.P = int(xy.shape[0]), int(xy.shape[1])


def _shaped(t, name, shape, want, dtypes=(torch.float32,)):
    t = _args.tensor(_TAG, t, name, dtypes)
    if t.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(t.shape, shape)):
        raise RuntimeError("%s: %s must be %s, got %s" % (_TAG, name, want, list(t.shape)))
    return t.contiguous()


def _size(size):
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise TypeError("%s: size must be (H, W), got %r" % (_TAG, size)) from None
    if not (1 <= H < 1 << 24 and 1 <= W < 1 << 24):
        raise ValueError("%s: size must be (H, W) with 1 <= H, W < 2^24, got (%d, %d)" % (_TAG, H, W))
    return H, W


def integrate(initial_pos, flow, flow_index, K, world_view, size, motion_mask=None):
    """``all_3D_pos`` and ``all_2D_pos`` of ``render_ftorf_viz_traj.py:264-274`` and the two per-Gaussian means of ``:278, 283``
    for the whole sequence in one launch; float32 tensors on one HIP device.

    ``initial_pos`` [P, 3]: the positions at the first frame (``:231-235``).  ``flow`` [U, n, 3]: the distinct per-frame flows
    ``(d_xyz_next - d_xyz_curr) * 0.25`` (``:228``); ``flow_index`` int32 [T] on the device: the row of ``flow`` frame t uses
    (``sequence_flows`` gives both).  ``K`` [T, 3, 3], ``world_view`` [T, 4, 4]: each view's ``K_tof`` and
    ``world_view_transform_tof`` as the camera stores them, stacked over the views.  ``size`` = (H, W) of the ToF image.

    ``motion_mask``: None means ``n == P``, the one case the reference's ``all_3D_pos[vid-1] + gs_xyz_flow[vid-1]`` works for.
    A bool tensor [P] with n set entries, or the ``DeformQuery`` of one (which holds its ranks already: a bare tensor costs
    one blocking count here), lets row i move by the flow row of its rank and the static rows by exactly zero; with every
    entry set the results are those without a mask, bit for bit.

    Returns a ``Tracks``.  Nothing is read on the host (a bare mask tensor apart): the call can be captured in a graph."""
    pos = _shaped(initial_pos, "initial_pos", (None, 3), "[P, 3]")
    P = int(pos.shape[0])
    if P < 1:
        raise RuntimeError("%s: initial_pos must be [P, 3] with P >= 1, got %s" % (_TAG, list(pos.shape)))
    fl = _shaped(flow, "flow", (None, None, 3), "[U, n, 3]")
    U, n = int(fl.shape[0]), int(fl.shape[1])
    if U < 1:
        raise RuntimeError("%s: flow must be [U, n, 3] with U >= 1, got %s" % (_TAG, list(fl.shape)))
    Ks = _shaped(K, "K", (None, 3, 3), "[T, 3, 3]")
    T = int(Ks.shape[0])
    if T < 1:
        raise RuntimeError("%s: K must be [T, 3, 3] with T >= 1, got %s" % (_TAG, list(Ks.shape)))
    views = _shaped(world_view, "world_view", (T, 4, 4), "[%d, 4, 4]" % T)
    index = _shaped(flow_index, "flow_index", (T,), "[%d], one row of flow per frame" % T, dtypes=(torch.int32,))
    H, W = _size(size)
    named = [(pos, "initial_pos"), (fl, "flow"), (index, "flow_index"), (Ks, "K"), (views, "world_view")]
    mask = rank = None
    if isinstance(motion_mask, DeformQuery):
        if motion_mask.mask is not None:
            if motion_mask.P != P:
                raise RuntimeError("%s: the DeformQuery's mask has %d rows, initial_pos %d" % (_TAG, motion_mask.P, P))
            if motion_mask.n != n:
                raise RuntimeError("%s: the motion mask has %d set entries, flow has n = %d rows" % (_TAG, motion_mask.n, n))
            mask, rank = motion_mask.mask, motion_mask.rank
            named.append((mask, "motion_mask"))
    elif motion_mask is not None:
        m = _shaped(motion_mask, "motion_mask", (P,), "[%d]" % P, dtypes=(torch.bool,))
        count = int(m.sum())                                # the one blocking count of a bare mask
        if count != n:
            raise RuntimeError("%s: the motion mask has %d set entries, flow has n = %d rows" % (_TAG, count, n))
        mask = m.view(torch.uint8)
        named.append((mask, "motion_mask"))
    if mask is None and n != P:
        raise RuntimeError("%s: without a motion mask flow must have n = P = %d rows, got %d" % (_TAG, P, n))
    dev = _args.devices(_TAG, "track", named)
    lib = _lib.load()
    if mask is not None and rank is None:
        rank = (torch.cumsum(mask, 0, dtype=torch.int32) - mask.to(torch.int32)).contiguous()
    xy = torch.empty((T, P, 2), device=dev, dtype=torch.float32)
    pos_last = torch.empty((P, 3), device=dev, dtype=torch.float32)
    motion = torch.empty((P,), device=dev, dtype=torch.float32)
    mean_z = torch.empty((P,), device=dev, dtype=torch.float32)
    step_ok = torch.empty((T, P), device=dev, dtype=torch.uint8)
    with _lib.on_device(dev):
        _lib.check(lib.gft_tracks_integrate(_lib.raw_stream(dev), P, n, T, U, pos.data_ptr(), _args.ptr_nonempty(fl), index.data_ptr(),
                                            Ks.data_ptr(), views.data_ptr(), _ptr(mask), _ptr(rank), H, W, xy.data_ptr(),
                                            pos_last.data_ptr(), motion.data_ptr(), mean_z.data_ptr(), step_ok.data_ptr()))
    return Tracks(xy, pos_last, motion, mean_z, step_ok, (H, W))


def select(tr, opacity, scaling, big_motion_quantile=0.9, z_distr_quantile=0.5, opacity_quantile=0.5, small_size_quantile=0.1,
           big_size_quantile=0.9):
    """The Gaussians to draw, ``render_ftorf_viz_traj.py:278-290``, as the reference states them in torch, over ``tr.motion``
    and ``tr.mean_z``: ``(mask, big_big_motion_threshold)``, the bool mask [P] and the 0.95 quantile of the motion as a 0-dim
    device tensor.  ``opacity`` [P, 1] and ``scaling`` [P, 3] are the model's ``get_opacity`` / ``get_scaling``; the defaults are
    the program's.  Five quantiles and a few masked indexings: not the hot part, and it keeps the reference's host reads."""
    if not isinstance(tr, Tracks):
        raise TypeError("%s: select takes the Tracks of integrate, got %s" % (_TAG, type(tr).__name__))
    motion, mean_z = tr.motion, tr.mean_z
    opacity, scaling = opacity.detach(), scaling.detach()
    # large motion
    big_motion_threshold = torch.quantile(motion, big_motion_quantile)
    big_big_motion_threshold = torch.quantile(motion, BIG_BIG_MOTION_QUANTILE)
    mask = motion > big_motion_threshold
    # ... and near
    z_distr_threshold = torch.quantile(mean_z[mask], z_distr_quantile)
    mask = mask * (mean_z < z_distr_threshold)
    # ... and not transparent
    opacity_threshold = torch.quantile(opacity[mask], opacity_quantile)
    mask = mask * (opacity > opacity_threshold).squeeze()
    # ... and of middle size
    small_size_threshold = torch.quantile(torch.mean(scaling[mask], dim=-1), small_size_quantile)
    big_size_threshold = torch.quantile(torch.mean(scaling[mask], dim=-1), big_size_quantile)
    size = torch.mean(scaling, dim=-1)
    mask = mask * ((small_size_threshold < size) * (size < big_size_threshold)).squeeze()
    return mask, big_big_motion_threshold


class HostTable:
    """``TrackTable.to_host()``: numpy arrays over one pinned buffer -- ``xy`` float32 [T, S, 2], ``step_ok`` uint8 [T, S],
    ``motion`` float32 [S], ``index`` int64 [S] -- and ``size`` = (H, W).  Any object with these attributes serves ``walk``."""

    def __init__(self, xy, step_ok, motion, index, size):
        self.xy, self.step_ok, self.motion, self.index, self.size = xy, step_ok, motion, index, size
        self.T, self.S = int(xy.shape[0]), int(xy.shape[1])


class TrackTable:
    """The selected Gaussians' rows, in index order, as views into one contiguous uint8 device buffer: ``xy`` [T, S, 2],
    ``step_ok`` uint8 [T, S], ``motion`` [S], ``index`` int64 [S]."""

    def __init__(self, buffer, offsets, T, S, size):
        self.buffer, self.T, self.S, self.size = buffer, T, S, size
        self._offsets = offsets
        self.index, self.xy, self.motion, self.step_ok = self._views(buffer)

    def _views(self, buf):
        T, S, o = self.T, self.S, self._offsets
        part = lambda k, nbytes: buf[o[k]:o[k] + nbytes]
        return (part("index", 8 * S).view(torch.int64), part("xy", 8 * T * S).view(torch.float32).view(T, S, 2),
                part("motion", 4 * S).view(torch.float32), part("step_ok", T * S).view(T, S))

    def to_host(self):
        """One copy of the whole buffer into pinned memory, waited for: the sequence's one transfer.  A ``HostTable``."""
        host = torch.empty((self.buffer.numel(),), dtype=torch.uint8, pin_memory=True)
        if self.buffer.numel():
            host.copy_(self.buffer, non_blocking=True)
            torch.cuda.current_stream(self.buffer.device).synchronize()
        index, xy, motion, step_ok = self._views(host)
        return HostTable(xy.numpy(), step_ok.numpy(), motion.numpy(), index.numpy(), self.size)


def table_layout(T, S):
    """(bytes of the table of S rows over T frames, {part: byte offset})"""
    offsets = (C.c_int64 * len(_lib.TRACKS_PARTS))()
    total = int(_lib.load().gft_tracks_table_bytes(int(T), int(S), offsets))
    return total, {name: int(offsets[k]) for k, name in enumerate(_lib.TRACKS_PARTS)}


def table(tr, mask):
    """``tr.xy[:, mask]``, ``tr.step_ok[:, mask]``, ``tr.motion[mask]`` and the selected indices as one ``TrackTable``: the
    mask is ranked on the device, its count is the one blocking read (the buffer's size hangs on it, as with
    ``RowSelection``), and one launch gathers every part.  No selected row (S = 0) is valid."""
    if not isinstance(tr, Tracks):
        raise TypeError("%s: table takes the Tracks of integrate, got %s" % (_TAG, type(tr).__name__))
    m = _shaped(mask, "mask", (tr.P,), "[%d]" % tr.P, dtypes=(torch.bool,))
    dev = _args.devices(_TAG, "track", [(tr.xy, "tr.xy"), (m, "mask")])
    lib = _lib.load()
    P, T = tr.P, tr.T
    m8 = m.view(torch.uint8)
    rank = torch.empty((P,), device=dev, dtype=torch.int32)
    scratch = torch.empty((lib.gft_rows_rank_scratch_bytes(P),), device=dev, dtype=torch.uint8)
    count = torch.empty((1,), device=dev, dtype=torch.int32)
    with _lib.on_device(dev):
        _lib.check(lib.gft_rows_rank_dev(_lib.raw_stream(dev), P, m8.data_ptr(), rank.data_ptr(), scratch.data_ptr(), count.data_ptr()))
        S = int(count.item())                               # the one blocking read
        total, offsets = table_layout(T, S)
        buf = torch.empty((total,), device=dev, dtype=torch.uint8)
        if S:
            _lib.check(lib.gft_tracks_table(_lib.raw_stream(dev), P, T, S, m8.data_ptr(), rank.data_ptr(), tr.xy.data_ptr(),
                                            tr.step_ok.data_ptr(), tr.motion.data_ptr(), buf.data_ptr()))
    return TrackTable(buf, offsets, T, S, tr.size)


def color_array(S):
    """``generate_color_array(S)`` followed by ``np.random.shuffle`` (``render_ftorf_viz_traj.py:41-46, 294-295``): uint8
    [S, 3].  The reference seeds numpy's global generator with 42; the same stream is drawn from a generator of its own here,
    so the caller's random state stays as it is."""
    rs = np.random.RandomState(42)
    r = rs.randint(0, 128, S)
    g = rs.randint(128, 256, S)
    b = rs.randint(128, 256, S)
    colors = np.stack([r, g, b], axis=1).astype(np.uint8)
    rs.shuffle(colors)
    return colors


def walk(table_host, radius=1, keep=None):
    """The drawing loop of ``render_ftorf_viz_traj.py:297-347`` over a ``HostTable``: yields ``(vid, trajectories, colors)``
    for every frame, the two dicts exactly as the reference has them when it draws frame ``vid`` (they are the loop's own
    running dicts: copy what has to outlive the next step).  Pure Python on the host copy; the device is not touched.

    Per frame the candidates are visited in index order: one whose first position is outside the image, or within ``radius``
    pixels of one already used in this frame, is passed over; at frame 0 a track starts, later it grows by the frame's
    position when ``step_ok`` holds (or starts late, if it has none yet); only a visit that got that far marks its pixel used.
    ``keep``: None, a bool [S], or a callable ``vid -> bool [S]``; a row it drops is passed over as the reference's scene-name
    branches (``:300-329``) do -- ``table_host.motion``, the threshold ``select`` returns and ``table_host.xy[0]`` are what
    those branches read."""
    T, S = table_host.T, table_host.S
    radius = int(radius)
    xy = table_host.xy
    first_inside = np.asarray(table_host.step_ok[0], dtype=bool) if T else np.zeros((0,), bool)
    pixels = [(int(xy[0, i, 0]), int(xy[0, i, 1])) if first_inside[i] else None for i in range(S)]
    all_colors = color_array(S)
    trajectories, colors = {}, {}
    for vid in range(T):
        kept = keep(vid) if callable(keep) else keep
        if kept is not None:
            kept = np.asarray(kept, dtype=bool)
            if kept.shape != (S,):
                raise ValueError("%s: keep must give a bool [%d], got %s" % (_TAG, S, list(kept.shape)))
        ok = table_host.step_ok[vid]
        used_pixels = set()
        for i in range(S):
            if kept is not None and not kept[i]:
                continue
            if pixels[i] is None:
                continue
            px, py = pixels[i]
            if any((px + dx, py + dy) in used_pixels for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1)):
                continue
            if vid == 0:
                trajectories[i] = [[float(xy[0, i, 0]), float(xy[0, i, 1])]]
                colors[i] = tuple(map(int, all_colors[i]))
            else:
                if not ok[i]:
                    continue
                point = [float(xy[vid, i, 0]), float(xy[vid, i, 1])]
                if i in trajectories:
                    trajectories[i].append(point)
                else:
                    trajectories[i] = [point]
                    colors[i] = tuple(map(int, all_colors[i]))
            used_pixels.add((px, py))
        yield vid, trajectories, colors


class SequenceFlows:
    """What ``sequence_flows`` returns: ``flow`` [U, n, 3], ``flow_index`` int32 [T] on the device, ``d_xyz(t)`` and
    ``evaluations``, the number of times the network ran."""

    def __init__(self, flow, flow_index, frame_ids, d_by_fid, evaluations):
        self.flow, self.flow_index, self.frame_ids, self.evaluations = flow, flow_index, frame_ids, evaluations
        self._d = d_by_fid

    def d_xyz(self, t):
        """The deformation of frame t, the lerp of ``render_ftorf_viz_traj.py:227`` from the sequence's evaluations.  On an
        integer frame that statement is ``0.25 * (0 * next + 4 * curr)``, and it is kept as such, so the bits are the
        reference's."""
        frame_id = self.frame_ids[t]
        curr_int_fid = (frame_id // 4) * 4
        next_int_fid = (frame_id // 4 + 1) * 4
        d_xyz_curr, d_xyz_next = self._d[curr_int_fid], self._d[next_int_fid]
        return 0.25 * ((frame_id - curr_int_fid) * d_xyz_next + (next_int_fid - frame_id) * d_xyz_curr)


def sequence_flows(deform, xyz_normalized_dynamic, frame_ids, denom):
    """The deformation queries of the whole sequence, ``render_ftorf_viz_traj.py:223-228``, each distinct time once.

    The reference queries the network twice per view, at ``(fid // 4) * 4`` and ``(fid // 4 + 1) * 4`` over ``denom``
    (``time_steps_denom``), though four consecutive frames share both.  Here every distinct integer frame of ``frame_ids``
    (the sorted views' ``frame_id``, Python ints) is evaluated once, under ``no_grad``, as ``deform(xyz, t)`` with the time
    ``query_dmlp`` forms (``scene/gaussian_model.py:171``): the same network on the same rows, so each result has the bits of
    the per-frame call.  ``deform``: the model's ``DeformNetwork``; ``xyz_normalized_dynamic`` [n, 3]:
    ``get_xyz_normalized[get_motion_mask]``.  Returns a ``SequenceFlows``: ``flow[flow_index[t]]`` is frame t's
    ``(d_xyz_next - d_xyz_curr) * 0.25``."""
    frame_ids = [int(f) for f in frame_ids]
    if not frame_ids:
        raise ValueError("%s: sequence_flows needs at least one frame" % _TAG)
    xyz = _shaped(xyz_normalized_dynamic, "xyz_normalized_dynamic", (None, 3), "[n, 3]")
    currs = sorted(set((f // 4) * 4 for f in frame_ids))
    fids = sorted(set(currs) | set(c + 4 for c in currs))
    n = int(xyz.shape[0])
    d = {}
    with torch.no_grad():
        for fid in fids:
            t = torch.full((n, 1), float(np.float32(fid / denom)), device=xyz.device, dtype=torch.float32)
            d[fid] = deform(xyz, t)[0]
        flow = torch.stack([(d[c + 4] - d[c]) * 0.25 for c in currs], dim=0)
    row = {c: u for u, c in enumerate(currs)}
    flow_index = torch.tensor([row[(f // 4) * 4] for f in frame_ids], dtype=torch.int32).to(xyz.device)
    return SequenceFlows(flow, flow_index, frame_ids, d, len(fids))
