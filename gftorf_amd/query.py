"""An iteration's deformation queries as one call (``csrc/k_query.hip``, ``include/gftorf_query.h``).

A dynamic iteration starts with ``GaussianModel.query_dmlp`` (``scene/gaussian_model.py:170-174``): the normalised positions
of the dynamic Gaussians, ``get_xyz_normalized[get_motion_mask]``, and the frame's time ``torch.tensor(np.array([fid]))``
go through the deformation network.  The boolean selection runs ``nonzero`` and reads the row count on the host, the time
is a pageable host-to-device copy: neither can sit in a captured iteration.  An F-ToRF iteration does it 2-3 times on the
same points (``train.py:169-176, 248, 255``) and combines the results with a lerp or two differences -- K packs, K
forwards, K backwards with a gradient buffer each, (K - 1) * 24 gradient additions by autograd and ten eager launches of
glue.

Here the K times of an iteration are one batch of K * n rows: ``gft_query_inputs`` writes ``x [K, n, 3]`` and ``t [K, n]``
from the model's own tensors, ONE ``DeformNetwork`` call runs over them (one pack, one forward, one backward, one gradient
bucket -- the one ``allreduce_gradients`` reduces), and one autograd node forms the M combinations of the K ``d_xyz``
blocks.  The dynamic rows are ranked once per mask (``DeformQuery``, one blocking read, like ``RowSelection``); the times
and the coefficients may be device tensors, read when the kernels run, so the whole query and its backward can be captured
in a graph and replayed on other frames.  A point's result does not depend on its batch (``gftorf_deform.h``), so the K
blocks equal K separate calls bit for bit, and the combinations reproduce the reference's statements bit for bit (each
product rounded, terms added in increasing k, zero coefficients skipped).  There is no CPU path.
"""
import ctypes as C

import torch

from . import _lib
from .deform import DeformNetwork, _param_list, run_network

NAMES = ("d_xyz", "flow_next", "flow_prev")


def _fail_grad(t, name):
    if isinstance(t, torch.Tensor) and t.requires_grad:
        raise NotImplementedError("gftorf_amd.query: gradients flow to the network's parameters only; %s requires grad" % name)


def _device_only(t, name):
    if t.device.type != "cuda":
        raise RuntimeError("gftorf_amd.query: %s is on %s; the query kernels run on a HIP device only, there is no CPU path"
                           % (name, t.device))


def _floats(values):
    return (C.c_float * len(values))(*values)


def _matrix(m, name, vector=False):
    """A float32 device tensor or a (nested) list of numbers -> (device tensor or None, host floats or None, shape)."""
    if isinstance(m, torch.Tensor):
        _fail_grad(m, name)
        if m.dtype != torch.float32:
            raise TypeError("gftorf_amd.query: %s must be torch.float32, got %s" % (name, m.dtype))
        return m, None, tuple(m.shape)
    try:
        rows = [list(m)] if vector else [list(r) for r in m]
        host = [float(v) for r in rows for v in r]
    except TypeError:
        raise TypeError("gftorf_amd.query: %s must be a float32 device tensor or a %slist of numbers, got %r"
                        % (name, "" if vector else "nested ", m)) from None
    cols = len(rows[0]) if rows else 0
    if any(len(r) != cols for r in rows):
        raise RuntimeError("gftorf_amd.query: the rows of %s differ in length" % name)
    return None, host, ((cols,) if vector else (len(rows), cols))


class _Combine(torch.autograd.Function):
    """outs[m] = sum_k C[m, k] * d[k] over the K blocks of ``d`` [K * n, 3] (gft_query_combine and its backward)."""

    @staticmethod
    def forward(ctx, d, coeffs_dev, coeffs_host, n, K, M):
        lib = _lib.load()
        dev = d.device
        d = d.detach().contiguous()
        outs = tuple(torch.empty((n, 3), device=dev, dtype=torch.float32) for _ in range(M))
        if n:
            table = (C.c_void_p * M)(*(o.data_ptr() for o in outs))
            with _lib.on_device(dev):
                _lib.check(lib.gft_query_combine(_lib.raw_stream(dev), n, K, M, d.data_ptr(),
                                                 coeffs_dev.data_ptr() if coeffs_dev is not None else None,
                                                 _floats(coeffs_host) if coeffs_host is not None else None, table))
        ctx.call = (coeffs_dev, coeffs_host, n, K, M, dev)
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, *g_outs):
        lib = _lib.load()
        coeffs_dev, coeffs_host, n, K, M, dev = ctx.call
        g_d = torch.empty((K * n, 3), device=dev, dtype=torch.float32)
        if n:
            gs = [g.float().contiguous() if g is not None else None for g in g_outs]
            table = (C.c_void_p * M)(*(g.data_ptr() if g is not None else None for g in gs))
            with _lib.on_device(dev):
                _lib.check(lib.gft_query_combine_backward(_lib.raw_stream(dev), n, K, M, table,
                                                          coeffs_dev.data_ptr() if coeffs_dev is not None else None,
                                                          _floats(coeffs_host) if coeffs_host is not None else None, g_d.data_ptr()))
        return g_d, None, None, None, None, None


class DeformQuery:
    """The plan of the queries for one motion mask: the dynamic rows and their count ``n``, computed once (``gft_rows_rank``,
    one blocking read, like ``RowSelection``).  Build it before a capture and again after densification, like every other
    shape-dependent object here.  ``motion_mask``: a contiguous bool tensor [P] on the HIP device, kept by reference;
    ``None``: every Gaussian is dynamic (the torf configuration), ``n`` is then the row count of the positions."""

    def __init__(self, motion_mask=None):
        self.mask = self.rank = self.count = self._scratch = None
        self.P = self.n = None
        if motion_mask is None:
            return
        if not isinstance(motion_mask, torch.Tensor):
            raise TypeError("gftorf_amd.query: motion_mask must be a tensor or None, got %s" % type(motion_mask).__name__)
        _fail_grad(motion_mask, "motion_mask")
        if motion_mask.dtype != torch.bool:
            raise TypeError("gftorf_amd.query: motion_mask must be torch.bool, got %s" % motion_mask.dtype)
        if motion_mask.dim() != 1 or not motion_mask.is_contiguous():
            raise RuntimeError("gftorf_amd.query: motion_mask must be a contiguous [P] tensor, got %s" % list(motion_mask.shape))
        _device_only(motion_mask, "motion_mask")
        lib = _lib.load()
        dev = motion_mask.device
        self.P = P = int(motion_mask.shape[0])
        self.motion_mask = motion_mask
        self.mask = motion_mask.view(torch.uint8)                # the same memory: refresh() follows an in-place edit
        self.rank = torch.empty((P,), device=dev, dtype=torch.int32)
        self._scratch = torch.empty((lib.gft_rows_rank_scratch_bytes(P),), device=dev, dtype=torch.uint8)
        self.count = torch.empty((1,), device=dev, dtype=torch.int32)
        n = C.c_int64(0)
        with _lib.on_device(dev):
            _lib.check(lib.gft_rows_rank(_lib.raw_stream(dev), P, self.mask.data_ptr() if P else None, self.rank.data_ptr() if P else None,
                                         self._scratch.data_ptr() if P else None, C.byref(n)))
        self.n = int(n.value)
        self.count.fill_(self.n)

    @classmethod
    def from_rank(cls, motion_mask, rank, n):
        """The plan of a mask that has been ranked already: adopts ``motion_mask`` (contiguous bool [P] on the HIP device),
        its exclusive ``rank`` (contiguous int32 [P]: the number of set entries before each row) and its count ``n`` without
        ranking again and without a host read -- what ``gftorf_amd.densify.densify_and_prune_fused`` leaves behind
        (``DensifyResult.deform_query``).  Both tensors are kept by reference."""
        if not isinstance(motion_mask, torch.Tensor) or not isinstance(rank, torch.Tensor):
            raise TypeError("gftorf_amd.query: motion_mask and rank must be tensors")
        if motion_mask.dtype != torch.bool or rank.dtype != torch.int32:
            raise TypeError("gftorf_amd.query: motion_mask must be torch.bool and rank torch.int32, got %s and %s"
                            % (motion_mask.dtype, rank.dtype))
        if motion_mask.dim() != 1 or not motion_mask.is_contiguous() or rank.shape != motion_mask.shape or not rank.is_contiguous():
            raise RuntimeError("gftorf_amd.query: motion_mask and rank must be contiguous [P] tensors, got %s and %s"
                               % (list(motion_mask.shape), list(rank.shape)))
        _device_only(motion_mask, "motion_mask")
        if rank.device != motion_mask.device:
            raise RuntimeError("gftorf_amd.query: rank is on %s, motion_mask on %s" % (rank.device, motion_mask.device))
        P = int(motion_mask.shape[0])
        n = int(n)
        if not 0 <= n <= P:
            raise ValueError("gftorf_amd.query: n must be the number of set mask entries (0..%d), got %d" % (P, n))
        self = cls(None)
        dev = motion_mask.device
        self.P, self.n = P, n
        self.motion_mask = motion_mask
        self.mask = motion_mask.view(torch.uint8)
        self.rank = rank
        self._scratch = torch.empty((_lib.load().gft_rows_rank_scratch_bytes(P),), device=dev, dtype=torch.uint8)      # refresh()
        self.count = torch.full((1,), n, device=dev, dtype=torch.int32)
        return self

    def refresh(self):
        """Re-derives the dynamic rows on the device from the mask's current contents (``gft_rows_rank_dev``): nothing is read
        on the host, ``n`` stays, the call can be captured.  Call it after every in-place edit of the mask, before the next
        query.  With fewer dynamic rows than ``n`` afterwards the surplus rows of a query are the point 0; with more, the
        last ones are left out."""
        if self.mask is None or self.P == 0:
            return self
        dev = self.mask.device
        with _lib.on_device(dev):
            _lib.check(_lib.load().gft_rows_rank_dev(_lib.raw_stream(dev), self.P, self.mask.data_ptr(), self.rank.data_ptr(),
                                                     self._scratch.data_ptr(), self.count.data_ptr()))
        return self

    def _checked(self, xyz, times):
        """Shapes, dtypes and gradients first, then the devices (the order of ``reg._check``)."""
        if not isinstance(xyz, torch.Tensor):
            raise TypeError("gftorf_amd.query: xyz must be a tensor, got %s" % type(xyz).__name__)
        if xyz.dim() != 2 or xyz.shape[1] != 3 or (self.P is not None and int(xyz.shape[0]) != self.P):
            raise RuntimeError("gftorf_amd.query: xyz must be %s, got %s" % ("[P, 3]" if self.P is None else "[%d, 3]" % self.P,
                                                                              list(xyz.shape)))
        if xyz.dtype != torch.float32:
            raise TypeError("gftorf_amd.query: xyz must be torch.float32, got %s" % xyz.dtype)
        t_dev, t_host, t_shape = _matrix(times, "times", vector=True)
        if len(t_shape) != 1 or not 1 <= t_shape[0] <= _lib.QUERY_MAX_TIMES:
            raise RuntimeError("gftorf_amd.query: times must be [K] with 1 <= K <= %d, got %s" % (_lib.QUERY_MAX_TIMES, list(t_shape)))
        return t_dev, t_host, t_shape[0]

    def _on_device(self, xyz, others):
        dev = xyz.device
        for t, name in (((xyz, "xyz"),) + tuple(others)):
            if t is not None:
                _device_only(t, name)
                if t.device != dev:
                    raise RuntimeError("gftorf_amd.query: %s is on %s, xyz on %s" % (name, t.device, dev))
        if self.mask is not None and self.mask.device != dev:
            raise RuntimeError("gftorf_amd.query: motion_mask is on %s, xyz on %s" % (self.mask.device, dev))
        return dev

    def inputs(self, xyz, scene_extent, times):
        """``x [K * n, 3], t [K * n]``, time-major: ``x[k * n + j] = (xyz / scene_extent)[motion_mask][j]`` with eager torch's
        bits on the device, ``t[k * n + j] = times[k]`` (``gft_query_inputs``).  Detached; every row is written."""
        t_dev, t_host, K = self._checked(xyz, times)
        return self._inputs(xyz, scene_extent, t_dev, t_host, K, self._on_device(xyz, ((t_dev, "times"),)))

    def _inputs(self, xyz, scene_extent, t_dev, t_host, K, dev):
        lib = _lib.load()
        P = int(xyz.shape[0])
        n = P if self.mask is None else self.n
        src = xyz.detach().contiguous()
        t_c = t_dev.detach().contiguous() if t_dev is not None else None
        x = torch.empty((K * n, 3), device=dev, dtype=torch.float32)
        t = torch.empty((K * n,), device=dev, dtype=torch.float32)
        if n:
            ptr = lambda v: v.data_ptr() if v is not None else None
            with _lib.on_device(dev):
                # 1 / extent in fp32, as ATen's true-divide by a scalar forms it on the device
                _lib.check(lib.gft_query_inputs(_lib.raw_stream(dev), P, src.data_ptr(), ptr(self.mask), ptr(self.rank), ptr(self.count),
                                                n, K, _recip32(scene_extent), ptr(t_c),
                                                _floats(t_host) if t_host is not None else None, x.data_ptr(), t.data_ptr()))
        return x, t

    def plan(self, net, xyz, scene_extent, times, combine=None, sh_of=None):
        """``(outs, d_sh)``: the network queried at the K ``times`` on the dynamic rows of ``xyz / scene_extent``, in one batch.

        ``net``: a ``gftorf_amd.DeformNetwork``; ``xyz`` [P, 3]: the model's raw ``_xyz`` (detached, as the reference does);
        ``times``: K <= 4 Python numbers, taken by value through float32 as ``gaussian_model.py:171`` does, or a float32
        device tensor [K] read when the kernels run.  ``combine``: None gives the K ``d_xyz`` blocks themselves; otherwise an
        [M, K] nested list or float32 device tensor (read when the kernels run), M <= 4: ``outs[m] = sum_k combine[m][k] *
        d_xyz_k``.  ``outs`` is a tuple of M [n, 3] tensors.  ``sh_of=k`` also returns the ``d_sh`` [n, 16, 3] of time k,
        with its gradient (the ``d_sh`` rows of the other times are computed and dropped); with None ``d_sh`` is None, the
        network's backward receives no ``d_sh`` gradient at all and the ``r`` / ``g`` / ``b`` heads get none, as under the
        reference's autograd when ``d_sh`` is discarded (``train.py:171``).  Gradients reach the network's parameters only.
        With no dynamic row (``n == 0``) the network is not run: the outputs are empty tensors without a gradient function."""
        if not isinstance(net, DeformNetwork):
            raise TypeError("gftorf_amd.query: net must be a gftorf_amd.DeformNetwork, got %s" % type(net).__name__)
        t_dev, t_host, K = self._checked(xyz, times)
        c_dev = c_host = None
        M = K
        if combine is not None:
            c_dev, c_host, c_shape = _matrix(combine, "combine")
            if len(c_shape) != 2 or c_shape[1] != K or not 1 <= c_shape[0] <= _lib.QUERY_MAX_OUTPUTS:
                raise RuntimeError("gftorf_amd.query: combine must be [M, %d] with 1 <= M <= %d, got %s"
                                   % (K, _lib.QUERY_MAX_OUTPUTS, list(c_shape)))
            M = c_shape[0]
        if sh_of is not None and not (isinstance(sh_of, int) and 0 <= sh_of < K):
            raise ValueError("gftorf_amd.query: sh_of must be None or an index into the %d times, got %r" % (K, sh_of))
        dev = self._on_device(xyz, ((t_dev, "times"), (c_dev, "combine")))
        n = int(xyz.shape[0]) if self.mask is None else self.n
        if n == 0:
            # no dynamic row (every one pruned): nothing is queried.  The empty outputs hang on no parameter, so the network
            # gets no gradient at all -- not 2 MB of zeros -- and its optimizer, which skips a parameter without one, neither
            # counts a step nor moves the weights on their momentum alone.
            empty = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
            return tuple(empty(0, 3) for _ in range(M)), (None if sh_of is None else empty(0, 16, 3))
        x, t = self._inputs(xyz, scene_extent, t_dev, t_host, K, dev)
        params = _param_list(net)
        if sh_of is None:
            params = params[:-6] + [p.detach() for p in params[-6:]]          # r, g, b: no output of theirs is used
        d_xyz, d_sh = run_network(net, x, t, params)
        if combine is None and K == 1:
            outs = (d_xyz,)
        else:
            if combine is None:
                c_host = [1.0 if m == k else 0.0 for m in range(K) for k in range(K)]
            outs = _Combine.apply(d_xyz, c_dev.detach().contiguous() if c_dev is not None else None, c_host, n, K, M)
        if sh_of is None:
            return outs, None
        return outs, (d_sh if K == 1 else d_sh[sh_of * n:(sh_of + 1) * n])


def _recip32(extent):
    """``1.0f / extent`` rounded once to float32 (the extent itself taken through float32 first, as a kernel argument is)."""
    import numpy as np
    return float(np.float32(1.0) / np.float32(float(extent)))


def ftorf_schedule(frame_id, total_num_views, sync=False, forward_flow=False, backward_flow=False):
    """``(times, combine, names)`` of an F-ToRF iteration on frame ``frame_id`` -- the fids and coefficients of
    ``train.py:169-176, 248, 255`` (and ``training_report``, ``:525-532``), pure Python.

    ``times[0]`` is the integer frame at or below ``frame_id``; between two integer frames (and not ``sync``:
    ``iteration <= opt.optimize_sync_iters``) ``times[1]`` is the next one and ``d_xyz`` their lerp.  On an integer frame
    ``forward_flow`` / ``backward_flow`` (``viewpoint_cam.forward_flow is not None`` inside the window of ``train.py:243``)
    add the times of frame + 4 / frame - 4 and the rows ``flow_next = d_xyz_next - d_xyz`` / ``flow_prev = d_xyz_prev -
    d_xyz``; ``d_xyz_curr`` of those lines is ``d_xyz`` itself.  ``names`` are the outputs' names, from ``NAMES``."""
    f = int(frame_id)
    den = total_num_views - 1
    curr_int_fid = (f // 4) * 4
    next_int_fid = (f // 4 + 1) * 4
    times = [curr_int_fid / den]
    rows = {"d_xyz": {0: 1.0}}
    if f % 4 != 0 and not sync:
        times.append(next_int_fid / den)
        rows["d_xyz"] = {0: 0.25 * (next_int_fid - f), 1: 0.25 * (f - curr_int_fid)}
    if f % 4 == 0:
        for flag, name, fid in ((forward_flow, "flow_next", f + 4), (backward_flow, "flow_prev", f - 4)):
            if flag:
                rows[name] = {0: -1.0, len(times): 1.0}
                times.append(fid / den)
    names = tuple(n for n in NAMES if n in rows)
    combine = [[rows[n].get(k, 0.0) for k in range(len(times))] for n in names]
    return times, combine, names


def query_dmlp(pc, fid, plan=None):
    """Drop-in for ``GaussianModel.query_dmlp`` (``scene/gaussian_model.py:170-174``): the four values
    ``DeformNetwork.forward`` returns, for the dynamic Gaussians of ``pc`` at time ``fid`` (a number or a float32 device
    tensor [1]).  ``plan``: the ``DeformQuery`` of ``pc.get_motion_mask``, built once per densification; without one it is
    built here (one blocking read, as the reference's selection has)."""
    q = plan if plan is not None else DeformQuery(pc.get_motion_mask.contiguous())
    times = fid if isinstance(fid, torch.Tensor) else [fid]
    (d_xyz,), d_sh = q.plan(pc.deform_model.deform, pc._xyz, pc.scene_extent, times, sh_of=0)
    n = d_xyz.shape[0]
    zeros = lambda *shape: torch.zeros(shape, device=d_xyz.device, dtype=torch.float32)
    return d_xyz, zeros(n, 4), d_sh, zeros(n, 16, 2)
