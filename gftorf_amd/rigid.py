"""The local-rigidity priors of the dynamic Gaussians (``csrc/k_knn.hip``, ``csrc/k_rigid.hip``, ``include/gftorf_rigid.h``):
the reference's ``find_knn``, ``rigidity_loss`` and ``isometry_loss`` (``utils/loss_utils.py:35-72``), which its ``train.py``
never calls but anyone who adds such a prior to F-ToRF training starts from.

``find_knn`` there builds the P x P matrix of ``torch.cdist`` -- 40 GB at 100 k Gaussians -- whose fp32 squared distances are
off by whole factors between close points far from the origin, so rows miss true neighbours and keep the point itself.  Here
the search is the exact, pruned one of ``distCUDA2`` with the neighbours kept.  The two losses gather ``[P, k, 3]`` tensors and
scatter the neighbours' gradients back with ``index_put``, in no defined order; here they are one autograd node: two launches
forward, one backward that walks every point's own edges and then the edges that name it (the table's transpose, built once
per table) in a stored order, without an atomic, a memset or a host read.  The same bits from run to run, and the forward and
the backward can be captured in a graph; a replay follows positions moved in place.  There is no CPU path.

    nb = rigid.Neighbours.build(xyz, 20)                       # once: idx, dist2 and the transpose
    w_i_j = torch.exp(-lam * nb.dist2)                         # and initial_xyz_to_knn_dist = nb.dist2
    loss = loss + rigid.rigid_terms(prev_xyz, curr_xyz, nb, w_i_j, nb.dist2, w_rigid=4.0, w_iso=2.0)[0]
"""
import collections

import torch

from . import _args, _lib
from ._args import ptr as _ptr

TAG = "gftorf_amd.rigid"
TERMS = ("rigidity", "isometry")                                # the order of the means and of `weights`
MAX_K = _lib.RIGID_MAX_K

RigidTerms = collections.namedtuple("RigidTerms", ["means", "total"])
RigidTerms.__doc__ = """``means``: float32 [2], the unweighted means in the order of ``TERMS`` (0 for an absent term);
``total``: float32 0-dim, their weighted sum.  Detached device tensors (views of one result block)."""


def _points(xyz, name):
    if not isinstance(xyz, torch.Tensor):
        raise TypeError("%s: %s must be a tensor, got %s" % (TAG, name, type(xyz).__name__))
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError("%s: %s must be [P, 3], got %s" % (TAG, name, list(xyz.shape)))
    if xyz.dtype != torch.float32:
        raise TypeError("%s: %s must be torch.float32, got %s" % (TAG, name, xyz.dtype))
    return xyz


def _no_grad(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a tensor, got %s" % (TAG, name, type(t).__name__))
    if t.requires_grad:
        raise NotImplementedError("%s: gradients flow to curr_xyz and prev_xyz only; %s requires grad" % (TAG, name))
    return t


def _check_k(P, k):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("%s: k = %d is outside 1..%d" % (TAG, k, MAX_K))
    if P <= k:
        raise ValueError("%s: %d points have no %d other points each (the reference's topk(k + 1) raises too)" % (TAG, P, k))
    return k


def _knn(xyz, k):
    """(idx int32 [P, k], dist2 float32 [P, k]) of gft_rigid_knn"""
    xyz = _points(xyz, "xyz").detach().contiguous()
    P, k = int(xyz.shape[0]), _check_k(int(xyz.shape[0]), k)
    dev = _args.devices(TAG, "rigidity", [(xyz, "xyz")])
    lib = _lib.load()
    idx = torch.empty((P, k), device=dev, dtype=torch.int32)
    dist2 = torch.empty((P, k), device=dev, dtype=torch.float32)
    scratch = torch.empty((lib.gft_rigid_knn_scratch_bytes(P),), device=dev, dtype=torch.uint8)
    with _lib.on_device(dev):
        _lib.check(lib.gft_rigid_knn(_lib.raw_stream(dev), P, k, xyz.data_ptr(), idx.data_ptr(), dist2.data_ptr(), scratch.data_ptr()))
    return idx, dist2


class Neighbours:
    """A neighbour table on the device: ``idx`` int32 [P, K], ``dist2`` float32 [P, K] (None for a caller's table) and the
    transpose the backward walks -- ``offsets`` int32 [P + 1], ``edges`` int32 [P * K]: ``edges[offsets[i]:offsets[i + 1]]``
    are the edge numbers ``m * K + k`` with ``idx[m, k] == i``, ascending.  Every index lies in [0, P): ``build`` gives such
    a table, ``from_indices`` checks a caller's, and the kernels see no other."""

    def __init__(self, idx, dist2):
        P, K = idx.shape
        flat = idx.reshape(-1).long()
        # built once per table with torch: not on the per-iteration path
        self.idx, self.dist2 = idx, dist2
        self.edges = torch.sort(flat, stable=True)[1].to(torch.int32)
        offsets = torch.zeros((P + 1,), device=idx.device, dtype=torch.int64)
        torch.cumsum(torch.bincount(flat, minlength=P), 0, out=offsets[1:])
        self.offsets = offsets.to(torch.int32)

    P = property(lambda self: int(self.idx.shape[0]))
    K = property(lambda self: int(self.idx.shape[1]))

    @property
    def in_degree(self):
        """int32 [P]: how many rows name each point"""
        return self.offsets[1:] - self.offsets[:-1]

    @classmethod
    def build(cls, xyz, k):
        """The exact ``k`` nearest other points of every row of ``xyz`` [P, 3] (float32, HIP device): a row is ordered by
        (squared distance ascending, index ascending); the point itself is excluded by its index, so a duplicate is a
        neighbour at distance 0.  ``dist2`` is the fp32 ``dx * dx + dy * dy + dz * dz`` of ``distCUDA2``."""
        return cls(*_knn(xyz, k))

    @classmethod
    def from_indices(cls, idx):
        """A caller's table, int32 or int64 [P, K] on a HIP device (``find_knn``'s result, the reference's).  Its range is
        checked with one blocking read: an index outside [0, P) raises ``ValueError`` before any kernel sees the table."""
        if not isinstance(idx, torch.Tensor):
            raise TypeError("%s: the neighbour table must be a tensor, got %s" % (TAG, type(idx).__name__))
        if idx.dtype not in (torch.int32, torch.int64):
            raise TypeError("%s: the neighbour table must be torch.int32 or torch.int64, got %s" % (TAG, idx.dtype))
        if idx.dim() != 2 or idx.shape[0] < 1 or idx.shape[1] < 1:
            raise RuntimeError("%s: the neighbour table must be [P, K], got %s" % (TAG, list(idx.shape)))
        if idx.device.type != "cuda":
            raise RuntimeError("%s: the neighbour table is on %s; the rigidity kernels run on a HIP device only, there is no CPU path"
                               % (TAG, idx.device))
        P = int(idx.shape[0])
        if P * int(idx.shape[1]) > 0x7fffffff:
            raise ValueError("%s: P * K = %d is too large" % (TAG, P * int(idx.shape[1])))
        lo, hi = torch.stack(torch.aminmax(idx.detach())).tolist()
        if lo < 0 or hi >= P:
            raise ValueError("%s: the neighbour table holds indices %d..%d outside [0, %d)" % (TAG, lo, hi, P))
        return cls(idx.detach().to(torch.int32).contiguous(), None)


def find_knn(xyz, k):
    """Drop-in for the reference's ``find_knn(xyz, k)`` (``utils/loss_utils.py:35-44``): int64 [P, k], the indices of the
    ``k`` nearest neighbours of every point, nearest first.  The differences are what the reference intends:

    * it is exact -- the reference takes ``topk`` of ``torch.cdist``, whose fp32 distances between close points are wrong by
      whole factors away from the origin, and needs a P x P matrix;
    * the point itself is excluded by its index -- the reference drops column 0 of ``topk(k + 1)``, which is the point only
      while its distance to itself comes out smallest; a duplicate of the point is a neighbour at distance 0;
    * equal distances are ordered by index.

    ``Neighbours.build`` also keeps the squared distances and the transpose the losses' backward needs."""
    return _knn(xyz, k)[0].long()


def _edge_tensor(t, name, nb, named):
    if tuple(t.shape) != (nb.P, nb.K):
        raise RuntimeError("%s: %s must be [%d, %d], got %s" % (TAG, name, nb.P, nb.K, list(t.shape)))
    if t.dtype != torch.float32:
        raise TypeError("%s: %s must be torch.float32, got %s" % (TAG, name, t.dtype))
    named.append((t, name))
    return t


class _Rigid(torch.autograd.Function):
    """(weighted total, result block): k_rigid_fwd + k_rigid_finish forward, k_rigid_bwd backward."""

    @staticmethod
    def forward(ctx, prev, curr, w_ij, d0, weights, nb, w):
        lib, dev = _lib.load(), curr.device
        cont = lambda t: None if t is None else t.detach().contiguous()
        pv, cu, wt, dd, wd = (cont(t) for t in (prev, curr, w_ij, d0, weights))
        res = torch.empty((int(lib.gft_rigid_result_words()),), device=dev, dtype=torch.float32)
        partials = torch.empty((int(lib.gft_rigid_blocks(nb.P, nb.K)), _lib.RIGID_PARTIAL_WORDS), device=dev, dtype=torch.int32)
        with _lib.on_device(dev):
            _lib.check(lib.gft_rigid_forward(_lib.raw_stream(dev), nb.P, nb.K, nb.idx.data_ptr(), wt.data_ptr(), _ptr(pv), cu.data_ptr(),
                                             _ptr(dd), _ptr(wd), *w, partials.data_ptr(), res.data_ptr()))
        ctx.nb, ctx.w = nb, w
        ctx.save_for_backward(pv, cu, wt, dd, wd)
        ctx.mark_non_differentiable(res)
        return res[_lib.RIGID_TOTAL], res

    @staticmethod
    def backward(ctx, g, _g_res):
        lib = _lib.load()
        pv, cu, wt, dd, wd = ctx.saved_tensors
        nb, dev = ctx.nb, cu.device
        g_prev = torch.empty_like(pv) if pv is not None and ctx.needs_input_grad[0] else None
        g_curr = torch.empty_like(cu) if ctx.needs_input_grad[1] else None
        if g_prev is not None or g_curr is not None:
            gp = g.detach().float()            # a 0-dim gradient: one float at data_ptr()
            with _lib.on_device(dev):
                _lib.check(lib.gft_rigid_backward(_lib.raw_stream(dev), nb.P, nb.K, nb.idx.data_ptr(), nb.offsets.data_ptr(),
                                                  nb.edges.data_ptr(), wt.data_ptr(), _ptr(pv), cu.data_ptr(), _ptr(dd), _ptr(wd), *ctx.w,
                                                  gp.data_ptr(), _ptr(g_curr), _ptr(g_prev)))
        return g_prev, g_curr, None, None, None, None, None


def rigid_terms(prev_xyz, curr_xyz, neighbours, w_i_j, initial_xyz_to_knn_dist=None, w_rigid=1.0, w_iso=1.0, weights=None):
    """``w_rigid * rigidity + w_iso * isometry`` as one autograd node, and the result block: ``(total, RigidTerms)``.  With
    ``j = idx[i, k]``::

        rigidity = (w_i_j * sqrt((((prev_i - prev_j) - (curr_i - curr_j)) ** 2).sum(-1) + 1e-16)).mean()
        isometry = (w_i_j * (sqrt(initial_xyz_to_knn_dist + 1e-16) - sqrt(((curr_i - curr_j) ** 2).sum(-1) + 1e-16))).abs().mean()

    ``prev_xyz``, ``curr_xyz`` float32 [P, 3]; ``neighbours`` a ``Neighbours`` (or an index tensor, which is checked and
    transposed on every call: keep a ``Neighbours`` for a table used more than once); ``w_i_j`` and
    ``initial_xyz_to_knn_dist`` float32 [P, K].  The rigidity term is absent when ``prev_xyz`` is None, the isometry term
    when ``initial_xyz_to_knn_dist`` is None.  With ``weights`` -- a float32 device tensor ``[w_rigid, w_iso]`` -- in place
    of the two floats the weights are read on the device when the kernels run.  Gradients flow to ``curr_xyz`` and
    ``prev_xyz`` only; the block is detached."""
    # shapes, dtypes and gradients first, then the table, then the devices
    nb = neighbours if isinstance(neighbours, Neighbours) else None
    _no_grad(w_i_j, "w_i_j")
    if initial_xyz_to_knn_dist is not None:
        _no_grad(initial_xyz_to_knn_dist, "initial_xyz_to_knn_dist")
    named = [(_points(curr_xyz, "curr_xyz"), "curr_xyz")]
    if prev_xyz is not None:
        named.append((_points(prev_xyz, "prev_xyz"), "prev_xyz"))
        if prev_xyz.shape != curr_xyz.shape:
            raise RuntimeError("%s: prev_xyz is %s, curr_xyz %s" % (TAG, list(prev_xyz.shape), list(curr_xyz.shape)))
    if prev_xyz is None and initial_xyz_to_knn_dist is None:
        raise ValueError("%s: neither prev_xyz nor initial_xyz_to_knn_dist is given: no term" % TAG)
    if nb is None:
        nb = Neighbours.from_indices(neighbours)
    if nb.P != int(curr_xyz.shape[0]):
        raise RuntimeError("%s: the neighbour table has %d rows, curr_xyz %d" % (TAG, nb.P, int(curr_xyz.shape[0])))
    named.append((nb.idx, "the neighbour table"))
    _edge_tensor(w_i_j, "w_i_j", nb, named)
    if initial_xyz_to_knn_dist is not None:
        _edge_tensor(initial_xyz_to_knn_dist, "initial_xyz_to_knn_dist", nb, named)
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != (2,):
            raise TypeError("%s: weights must be a float32 tensor [2]" % TAG)
        _no_grad(weights, "weights")
        named.append((weights, "weights"))
        w = (0.0, 0.0)
    else:
        w = (float(w_rigid), float(w_iso))
    _args.devices(TAG, "rigidity", named)
    total, res = _Rigid.apply(prev_xyz, curr_xyz, w_i_j, initial_xyz_to_knn_dist, weights, nb, w)
    return total, RigidTerms(res[_lib.RIGID_MEANS:_lib.RIGID_MEANS + 2], res[_lib.RIGID_TOTAL])


def _weights_of(gaussians, names):
    if isinstance(gaussians, torch.Tensor):
        return (gaussians,) + (None,) * (len(names) - 1)
    return tuple(getattr(gaussians, n) for n in names)


def rigidity_loss(gaussians, prev_xyz, curr_xyz, curr_knn_indices):
    """Drop-in for the reference's ``rigidity_loss`` (``utils/loss_utils.py:46-60``).  ``gaussians``: any object with
    ``w_i_j`` [P, K], or that tensor itself; ``curr_knn_indices``: a ``Neighbours`` or an index tensor [P, K]."""
    (w,) = _weights_of(gaussians, ("w_i_j",))
    return rigid_terms(prev_xyz, curr_xyz, curr_knn_indices, w, None, 1.0, 0.0)[0]


def isometry_loss(gaussians, curr_xyz, curr_knn_indices, initial_xyz_to_knn_dist=None):
    """Drop-in for the reference's ``isometry_loss`` (``utils/loss_utils.py:62-72``).  ``gaussians``: any object with
    ``w_i_j`` and ``initial_xyz_to_knn_dist`` [P, K]; with the weight tensor in its place the distances are the fourth
    argument."""
    w, d0 = _weights_of(gaussians, ("w_i_j", "initial_xyz_to_knn_dist"))
    if d0 is None:
        d0 = initial_xyz_to_knn_dist
    if d0 is None:
        raise ValueError("%s: isometry_loss needs initial_xyz_to_knn_dist" % TAG)
    return rigid_terms(None, curr_xyz, curr_knn_indices, w, d0, 0.0, 1.0)[0]
