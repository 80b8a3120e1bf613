"""The ToF depth and the training iteration's log on the device (``csrc/k_tof.hip``, ``include/gftorf_tof.h``).

The reference's log (``train.py:188-200, 402-433``) builds ``phase_depth`` / ``gt_phase_depth`` with
``depth_from_tof_torch`` (``scene/torf_utils.py:59-64``; ``depth_range`` and the phase offset read with ``.item()``), copies
five images to the host, forms the scattering-phase maps and their errors in numpy, reduces them to scalars, adds two means
over ``get_features_phasor[:, 0, 1]`` (one through ``[visibility_filter]``, a host read of the row count) and five
``.item()`` s of loss terms: ~40 small launches, five image-sized copies and ~10 blocking reads per iteration, none of which
can be captured in a graph.  Here:

``depth_from_tof(tof, depth_range, phase_offset)``  the drop-in for ``depth_from_tof_torch``: one launch, and a
    ``depth_range`` / ``phase_offset`` given as a one-element device tensor (``pc.get_phase_offset``) is read when the
    kernel runs; a number or a 0-d numpy value (the camera's own ``depth_range`` / ``phase_offset``) is taken by value.
``train_log_row(...)``  every scalar of the log as one row: two launches, no host read, no atomic, no memset.
``TrainLog``  a ring of such rows with a device cursor: ``record`` can be captured once and every replay lands in the next
    slot; ``drain`` brings the rows to the host through pinned memory without blocking.

The one difference from the reference for ``depth_from_tof``: there is no backward, the result is detached even when
``tof`` requires grad (the reference's only differentiable use, ``phase_depth``, never reaches a loss; ``gt_phase_depth``,
the depth loss's target at ``train.py:232``, has no gradient there either).  For the log: the mean over an EMPTY visible
selection is 0, where the reference's is NaN.  There is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _args, _lib
from ._args import ptr_nonempty as _ptr

_TAG = "gftorf_amd.tof"
FLOATS = _lib.TOF_LOG_FLOATS                     # names of the float words of a row, in order
MAX_EXTRAS = _lib.TOF_LOG_MAX_EXTRAS


def _tensor(t, name, dtypes=(torch.float32,)):
    return _args.tensor(_TAG, t, name, dtypes)


def _planes(t, name, n):
    """A [C >= n, H, W] image (n >= 2) as (tensor, plane stride, H, W): taken in place when every plane is contiguous, else
    its first n planes copied."""
    t, stride = _args.planes(_TAG, t, name, least=n, keep=n)
    return t, stride, int(t.shape[1]), int(t.shape[2])


def _image(t, name, H, W):
    t = _tensor(t, name)
    if tuple(t.shape) != (1, H, W):
        raise RuntimeError("gftorf_amd.tof: %s must be [1, %d, %d], got %s" % (name, H, W, list(t.shape)))
    return t.contiguous()


def depth_from_tof(tof, depth_range, phase_offset=0.0):
    """Drop-in for ``depth_from_tof_torch(tof, depth_range, phase_offset)`` (``scene/torf_utils.py:59-64``): ``tof``
    [C >= 2, H, W] float32 on a HIP device (planes 0 and 1 are read; a view whose planes are contiguous, such as the
    rasterizer's ``phasor[:3]``, is read in place), the result [H, W].  ``depth_range`` and ``phase_offset`` are each a number, taken
    by value through ``float()`` (the reference's ``viewpoint_cam.depth_range`` / ``.phase_offset``, 0-d numpy float32
    arrays, go this way as they are), or a one-element float32 device tensor, read when the kernel runs (the learnable
    ``pc.get_phase_offset``, the only one of them the reference keeps on the device) -- no ``.item()`` either way.  No
    backward: the result is detached."""
    t, stride, H, W = _planes(tof, "tof", 2)
    named = [(t, "tof")]
    dr_t, dr = _args.scalar(_TAG, depth_range, "depth_range", named)
    po_t, po = _args.scalar(_TAG, phase_offset, "phase_offset", named)
    dev = _args.devices(_TAG, "ToF", named)
    out = torch.empty((H, W), device=dev, dtype=torch.float32)
    with _lib.on_device(dev):
        _lib.check(_lib.load().gft_tof_depth(_lib.raw_stream(dev), H * W, t.data_ptr(), stride, _ptr(dr_t), dr, _ptr(po_t), po,
                                             out.data_ptr()))
    return out


def _launch(rows, slots, cursor, partials, phasor, depth, gt_phasor, depth_range, phase_offset=0.0, tof_multiplier=1.0,
            gt_depth=None, depth_distortion=None, features_phasor=None, amp_f_dc=None, visible=None, extras=()):
    """Check the arguments and enqueue gft_tof_log_row; `partials` is the caller's scratch (rows of TOF_PARTIAL_WORDS
    int32 words, on the images' device) or None for a fresh one of this call's size."""
    lib = _lib.load()
    ph, ph_stride, H, W = _planes(phasor, "phasor", 3)
    gt, gt_stride, gH, gW = _planes(gt_phasor, "gt_phasor", 3)
    if (gH, gW) != (H, W):
        raise RuntimeError("gftorf_amd.tof: gt_phasor must be [>=3, %d, %d], got %s" % (H, W, list(gt_phasor.shape)))
    d = _image(depth, "depth", H, W)
    named = [(ph, "phasor"), (gt, "gt_phasor"), (d, "depth")]
    gd = dd = amp = vis = None
    if gt_depth is not None:
        gd = _image(gt_depth, "gt_depth", H, W)
        named.append((gd, "gt_depth"))
    if depth_distortion is not None:
        dd = _image(depth_distortion, "depth_distortion", H, W)
        named.append((dd, "depth_distortion"))
    if features_phasor is not None and amp_f_dc is not None:
        raise ValueError("gftorf_amd.tof: features_phasor and amp_f_dc are two forms of the same coefficients, give one")
    if features_phasor is not None:
        f = _tensor(features_phasor, "features_phasor")
        if f.dim() != 3 or f.shape[1] < 1 or f.shape[2] != 2:
            raise RuntimeError("gftorf_amd.tof: features_phasor must be [P, M, 2], got %s" % list(f.shape))
        amp = f[:, 0, 1]                    # read in place by stride
        named.append((amp, "features_phasor"))
    elif amp_f_dc is not None:
        f = _tensor(amp_f_dc, "amp_f_dc")
        if f.dim() != 3 or tuple(f.shape[1:]) != (1, 1):
            raise RuntimeError("gftorf_amd.tof: amp_f_dc must be [P, 1, 1], got %s" % list(f.shape))
        amp = f[:, 0, 0]
        named.append((amp, "amp_f_dc"))
    P = 0
    if amp is not None:
        P = int(amp.shape[0])
        if P > 1 and not 1 <= amp.stride(0) <= 1 << 20:
            amp = amp.contiguous()
    if visible is not None:
        if amp is None:
            raise ValueError("gftorf_amd.tof: visible selects among the amplitude coefficients; give features_phasor or amp_f_dc")
        vis = _tensor(visible, "visible", (torch.bool, torch.int32))
        if tuple(vis.shape) != (P,):
            raise RuntimeError("gftorf_amd.tof: visible must be [%d], got %s" % (P, list(vis.shape)))
        vis = vis.contiguous()
        named.append((vis, "visible"))
    extras = tuple(extras)
    if len(extras) > MAX_EXTRAS:
        raise ValueError("gftorf_amd.tof: at most %d extras fit a row, got %d" % (MAX_EXTRAS, len(extras)))
    ex = []
    for k, e in enumerate(extras):
        e = _tensor(e, "extras[%d]" % k)
        if e.numel() != 1:
            raise RuntimeError("gftorf_amd.tof: extras[%d] must be 0-dim or one-element, got %s" % (k, list(e.shape)))
        ex.append(e)
        named.append((e, "extras[%d]" % k))
    dr_t, dr = _args.scalar(_TAG, depth_range, "depth_range", named)
    po_t, po = _args.scalar(_TAG, phase_offset, "phase_offset", named)
    dev = _args.devices(_TAG, "ToF", named)
    if _ptr(amp) is None:
        P = 0
    blocks = int(lib.gft_tof_log_blocks(H * W, P))
    if partials is None:
        partials = torch.empty((blocks, _lib.TOF_PARTIAL_WORDS), device=dev, dtype=torch.int32)
    if partials.device != dev or partials.shape[0] < blocks:
        raise RuntimeError("gftorf_amd.tof: the images are on %s, the TrainLog's %d rows of scratch on %s"
                           % (dev, partials.shape[0], partials.device))
    ex_ptrs = (C.c_void_p * max(1, len(ex)))(*(e.data_ptr() for e in ex))
    with _lib.on_device(dev):
        _lib.check(lib.gft_tof_log_row(_lib.raw_stream(dev), H * W, P, ph.data_ptr(), ph_stride, d.data_ptr(), gt.data_ptr(), gt_stride,
                                       _ptr(dr_t), dr, _ptr(po_t), po, float(tof_multiplier), _ptr(gd), _ptr(dd), _ptr(amp),
                                       int(amp.stride(0)) if P > 1 else 1, _ptr(vis) if P else None,
                                       int(vis is not None and vis.dtype == torch.int32), ex_ptrs, len(ex), partials.data_ptr(),
                                       rows.data_ptr(), slots, None if cursor is None else cursor.data_ptr()))


def train_log_row(phasor, depth, gt_phasor, depth_range, phase_offset=0.0, tof_multiplier=1.0, gt_depth=None,
                  depth_distortion=None, features_phasor=None, amp_f_dc=None, visible=None, extras=()):
    """The scalars of ``train.py:402-433``'s log for one iteration as one float32 device tensor of
    ``_lib.TOF_LOG_WORDS`` words (``include/gftorf_tof.h`` ``GFT_TOF_LOG_*``; ``unpack`` names them).

    ``phasor`` [>=3, H, W] (the rasterizer's ``render_phasor``, its first three planes read in place), ``depth`` [1, H, W],
    ``gt_phasor`` [>=3, H, W]; ``depth_range`` / ``phase_offset`` as for ``depth_from_tof``; ``tof_multiplier`` the float
    of ``train.py:191-193``.  Optional: ``gt_depth`` and ``depth_distortion`` [1, H, W]; the amplitude coefficients as
    ``features_phasor`` [P, M, 2] (``pc.get_features_phasor``: element ``[:, 0, 1]`` is read in place) or as ``amp_f_dc``
    [P, 1, 1] (``pc._features_dc_amp``, the same numbers); ``visible`` bool [P] or the rasterizer's int32 ``radii``
    (visible where > 0); ``extras``: up to eight 0-dim or one-element float32 device tensors copied into the row (``loss``,
    ``Ll1``, ``Ll1_p``, the flow terms ...).  An absent input leaves 0 in its slots and its bit of the ``present`` word
    cleared; no visible row gives 0, not NaN.  Everything is read when the kernels run; nothing is read on the host."""
    rows = torch.empty((1, _lib.TOF_LOG_WORDS), device=phasor.device if isinstance(phasor, torch.Tensor) else None, dtype=torch.float32)
    _launch(rows, 1, None, None, phasor, depth, gt_phasor, depth_range, phase_offset, tof_multiplier, gt_depth, depth_distortion, features_phasor,
            amp_f_dc, visible, extras)
    return rows[0]


def unpack(rows):
    """Rows as a host array [n, TOF_LOG_WORDS] (float32, or the uint32 view of it) -> dict of names to numpy arrays [n]:
    the eleven means of ``FLOATS``, ``visible`` / ``present`` / ``num_extras`` / ``seq`` (uint32) and ``extras`` [n, 8]."""
    rows = np.ascontiguousarray(rows).reshape(-1, _lib.TOF_LOG_WORDS)
    f, u = rows.view(np.float32), rows.view(np.uint32)
    out = {name: f[:, k].copy() for k, name in enumerate(FLOATS)}
    out.update(visible=u[:, _lib.TOF_LOG_VISIBLE].copy(), present=u[:, _lib.TOF_LOG_PRESENT].copy(),
               num_extras=u[:, _lib.TOF_LOG_NUM_EXTRAS].copy(), seq=u[:, _lib.TOF_LOG_SEQ].copy(),
               extras=f[:, _lib.TOF_LOG_EXTRAS:_lib.TOF_LOG_EXTRAS + MAX_EXTRAS].copy())
    return out


class TrainLog:
    """A ring of ``slots`` log rows on the device with a device cursor, so that the log can live in a replayed graph::

        log = tof.TrainLog(slots=256)
        ...
        log.record(phasor, depth, gt_phasor, cam.depth_range, pc.get_phase_offset, ..., extras=(loss, Ll1, Ll1_p))   # captured or not
        ...
        rows, lost = log.drain()          # now and then, outside the graph: the rows whose copy has arrived

    ``record`` takes ``train_log_row``'s arguments.  Its finish kernel reads the cursor, writes row ``cursor % slots`` with
    ``seq = cursor`` and stores ``cursor + 1``: captured once, every replay lands in the next slot.  ``drain`` copies ring
    and cursor to pinned memory asynchronously (on the current stream, which must be the one ``record`` ran on) and hands
    the rows out the next time it is called, or at once with ``wait=True``.  Nothing else touches the host."""

    def __init__(self, slots=256, device=None):
        if not 1 <= int(slots) < 1 << 31:
            raise ValueError("gftorf_amd.tof: slots must be in 1 .. 2^31 - 1, got %r" % (slots,))
        lib = _lib.load()
        self.slots = int(slots)
        self.device = _args.indexed_device(_TAG, "a TrainLog", device)
        self.rows = torch.zeros((self.slots, _lib.TOF_LOG_WORDS), device=self.device, dtype=torch.float32)
        self.cursor = torch.zeros((1,), device=self.device, dtype=torch.int32)
        # the scratch of the largest launch there is, once: a graph captured by an earlier record keeps its address
        self._partials = torch.empty((int(lib.gft_tof_log_blocks(1 << 40, 0)), _lib.TOF_PARTIAL_WORDS), device=self.device,
                                     dtype=torch.int32)
        self._host_rows = torch.empty((self.slots, _lib.TOF_LOG_WORDS), dtype=torch.float32).pin_memory()
        self._host_cursor = torch.empty((1,), dtype=torch.int32).pin_memory()
        self._arrived = None                # the event behind a copy on its way
        self._next = 0                      # the first sequence number not yet handed out

    def record(self, *args, **kwargs):
        """``train_log_row(*args, **kwargs)`` into the ring's next slot.  Returns nothing: the row is the device's."""
        _launch(self.rows, self.slots, self.cursor, self._partials, *args, **kwargs)

    def _harvest(self):
        """The rows of the copy that has arrived which were not handed out yet, and the number lost before them."""
        self._arrived = None
        cursor = int(self._host_cursor.numpy().view(np.uint32)[0])
        first = max(self._next, cursor - self.slots)
        lost = first - self._next
        host = self._host_rows.numpy()
        rows = np.stack([host[s % self.slots] for s in range(first, cursor)]) if cursor > first else \
            np.empty((0, _lib.TOF_LOG_WORDS), np.float32)
        self._next = max(self._next, cursor)
        return rows, lost

    def drain(self, wait=False):
        """``(rows, lost)``: the rows not handed out before in sequence order as a dict of names to numpy arrays
        (``unpack``), and the number of rows that were overwritten before they were drained.  Without ``wait`` the call
        never blocks: it hands out what the previous call's copy brought (nothing while that copy is still on its way) and
        starts the next copy.  With ``wait=True`` it also waits for a copy of the ring as it is now."""
        parts, lost = [], 0
        for last in ((False, True) if wait else (False,)):
            if self._arrived is not None and (wait or self._arrived.query()):
                if wait:
                    self._arrived.synchronize()
                r, n = self._harvest()
                parts.append(r)
                lost += n
            if self._arrived is None and not last:
                with _lib.on_device(self.device):
                    self._host_rows.copy_(self.rows, non_blocking=True)
                    self._host_cursor.copy_(self.cursor, non_blocking=True)
                    self._arrived = torch.cuda.Event()
                    self._arrived.record()
        rows = np.concatenate(parts) if parts else np.empty((0, _lib.TOF_LOG_WORDS), np.float32)
        return unpack(rows), lost
