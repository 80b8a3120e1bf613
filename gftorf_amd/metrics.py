"""A view's evaluation metrics on the device (``csrc/k_metrics.hip``, ``include/gftorf_metrics.h``).

The reference's evaluation pass (``train.py:508-603`` ``training_report``) renders every test and train camera and evaluates,
per view, the statements of ``train.py:535-566`` eagerly: ``l1_loss`` and ``psnr`` of the colour image, ``l1_loss``,
``l2_loss`` and ``psnr`` of the selected ToF channels, ``depth_from_tof_torch`` of the rendered phasor (two ``.item()`` s),
``l1_loss`` / ``l2_loss`` of the rendered depth and ``l2_loss`` of the ToF depth against the ground-truth distance, and eight
``+= x.mean().double()``: ~45 small launches and two blocking reads per view.  Here:

``mse(img1, img2)``, ``psnr(img1, img2)``  drop-ins for ``utils/image_utils.py:14-19``: ``[C, 1]`` on the device, two launches.
``view_metrics(...)``  the eight values of one view (``VALUES`` names them) as a float32 device tensor: two launches, no host
    read, no atomic, no memset.
``EvalReport``  the sums of ``train.py:516-517`` as eight doubles on the device: ``add_view`` adds a view's values without a
    host read and can be captured in a graph, ``result`` divides by the number of views (``train.py:570-579``) after the
    one blocking read of the pass.

The one difference from the reference: a view's value is added to the report before it is rounded to float32, where the
reference adds the float32 ``.mean()``.  Nothing here has a gradient: the results are detached (the reference's block runs
under ``torch.no_grad()``).  There is no CPU path.
"""
import numpy as np
import torch

from . import _args, _lib
from ._args import ptr as _ptr

_TAG = "gftorf_amd.metrics"
VALUES = _lib.METRICS_VALUES                     # the eight names, in the order of a row and of the report's sums
MAX_PLANES = _lib.METRICS_MAX_PLANES


def _planes(t, name, shape=None, most=MAX_PLANES, least=1):
    """``_args.planes``; `shape` = the (C, H, W) the image must have, when its partner is known"""
    if shape is not None and tuple(_args.tensor(_TAG, t, name).shape) != tuple(shape):
        raise RuntimeError("gftorf_amd.metrics: %s must be %s, got %s" % (name, list(shape), list(t.shape)))
    return _args.planes(_TAG, t, name, least, most)


def _pair(a, b, name, gt_name, most):
    """a rendered image and its ground truth, both or neither: ((a, stride), (b, stride)) or None"""
    if a is None and b is None:
        return None
    if a is None or b is None:
        raise ValueError("gftorf_amd.metrics: %s and %s come together, %s is missing" % (name, gt_name, name if a is None else gt_name))
    pa = _planes(a, name, most=most)
    return pa, _planes(b, gt_name, shape=pa[0].shape)


def _launch(row, accum, partials, image=None, gt_image=None, tof=None, gt_tof=None, depth=None, gt_depth=None, phasor=None,
            depth_range=None, phase_offset=0.0, most_colour=3):
    """Check the arguments and enqueue gft_view_metrics; `partials` is the caller's scratch (rows of METRICS_PARTIAL_WORDS
    4-byte words, on the images' device) or None for a fresh one of this call's size."""
    lib = _lib.load()
    colour = _pair(image, gt_image, "image", "gt_image", most_colour)
    chans = _pair(tof, gt_tof, "tof", "gt_tof", 3)
    named, size_b = [], None

    def group_b(t, name):
        nonlocal size_b
        if size_b is None:
            size_b = (tuple(t.shape[1:]), name)
        elif tuple(t.shape[1:]) != size_b[0]:
            raise RuntimeError("gftorf_amd.metrics: %s is %d x %d, %s %d x %d: the ToF camera's images have one size"
                               % ((name,) + tuple(t.shape[1:]) + (size_b[1],) + size_b[0]))

    if colour is not None:
        named += [(colour[0][0], "image"), (colour[1][0], "gt_image")]
    if chans is not None:
        named += [(chans[0][0], "tof"), (chans[1][0], "gt_tof")]
        group_b(chans[0][0], "tof")
    d = gd = ph = None
    ph_stride = 0
    if depth is not None or phasor is not None:
        if gt_depth is None:
            raise ValueError("gftorf_amd.metrics: depth and phasor are compared against gt_depth, which is missing")
    if gt_depth is not None:
        if depth is None and phasor is None:
            raise ValueError("gftorf_amd.metrics: gt_depth is given without depth or phasor")
        gd = _planes(gt_depth, "gt_depth", most=1)[0]
        group_b(gd, "gt_depth")
        named.append((gd, "gt_depth"))
    if depth is not None:
        d = _planes(depth, "depth", most=1)[0]
        group_b(d, "depth")
        named.append((d, "depth"))
    dr_t = po_t = None
    dr = po = 0.0
    if phasor is not None:
        if depth_range is None:
            raise ValueError("gftorf_amd.metrics: the ToF depth of phasor needs depth_range")
        ph, ph_stride = _planes(phasor, "phasor", most=1 << 30, least=2)
        group_b(ph, "phasor")
        named.append((ph, "phasor"))
        dr_t, dr = _args.scalar(_TAG, depth_range, "depth_range", named)
        po_t, po = _args.scalar(_TAG, phase_offset, "phase_offset", named)
    if not named:
        raise ValueError("gftorf_amd.metrics: nothing to compare: give image, tof, depth or phasor with their ground truth")
    dev = _args.devices(_TAG, "metric", named)
    n_a = int(colour[0][0].shape[0]) if colour else 0
    n_b = int(chans[0][0].shape[0]) if chans else 0
    pixels_a = int(colour[0][0].shape[1] * colour[0][0].shape[2]) if colour else 0
    pixels_b = int(size_b[0][0] * size_b[0][1]) if size_b else 0
    blocks = int(lib.gft_metrics_blocks(max(pixels_a, pixels_b)))
    if partials is None:
        partials = torch.empty((blocks, _lib.METRICS_PARTIAL_WORDS), device=dev, dtype=torch.float32)
    for t, name in ((partials, "scratch"), (row, "row"), (accum, "sums")):
        if t is not None and t.device != dev:
            raise RuntimeError("gftorf_amd.metrics: the images are on %s, the %s on %s" % (dev, name, t.device))
    (im, im_s), (gi, gi_s) = colour if colour else ((None, 0), (None, 0))
    (tf, tf_s), (gt, gt_s) = chans if chans else ((None, 0), (None, 0))
    with _lib.on_device(dev):
        _lib.check(lib.gft_view_metrics(_lib.raw_stream(dev), pixels_a, n_a, _ptr(im), im_s, _ptr(gi), gi_s, pixels_b, n_b, _ptr(tf), tf_s,
                                        _ptr(gt), gt_s, _ptr(d), _ptr(gd), _ptr(ph), ph_stride, _ptr(dr_t), dr, _ptr(po_t), po,
                                        partials.data_ptr(), _ptr(row), _ptr(accum)))


def _first_device(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor):
            return t.device
    return None


def _planewise(img1, img2, word):
    """mse / psnr of every channel: [C, ...] flattened per channel as the reference's ``.view(img1.shape[0], -1)``"""
    a, b = _args.tensor(_TAG, img1, "img1"), _args.tensor(_TAG, img2, "img2")
    if a.dim() < 1 or a.shape != b.shape:
        raise RuntimeError("gftorf_amd.metrics: img1 and img2 must have one shape [C, ...], got %s and %s" % (list(a.shape), list(b.shape)))
    C = int(a.shape[0])
    if not 1 <= C <= MAX_PLANES:
        raise RuntimeError("gftorf_amd.metrics: %d channels, one call takes 1..%d" % (C, MAX_PLANES))
    if a.numel() == 0:
        raise RuntimeError("gftorf_amd.metrics: img1 is empty, got %s" % list(a.shape))
    a, b = a.reshape(C, 1, -1), b.reshape(C, 1, -1)
    row = torch.empty((_lib.METRICS_ROW_WORDS,), device=a.device, dtype=torch.float32)
    _launch(row, None, None, image=a, gt_image=b, most_colour=MAX_PLANES)
    return row[word:word + C].reshape(C, 1)


def mse(img1, img2):
    """Drop-in for ``utils/image_utils.py:14-15``: the mean squared difference of every channel of two [C, ...] float32 images
    on a HIP device, ``[C, 1]``; C <= 8.  Two launches."""
    return _planewise(img1, img2, _lib.METRICS_ROW_MSE)


def psnr(img1, img2):
    """Drop-in for ``utils/image_utils.py:17-19``: ``20 log10(1 / sqrt(mse))`` of every channel, ``[C, 1]``; ``+inf`` for a
    channel without a difference, as the reference.  Two launches."""
    return _planewise(img1, img2, _lib.METRICS_ROW_PSNR)


def view_metrics(image=None, gt_image=None, tof=None, gt_tof=None, depth=None, gt_depth=None, phasor=None, depth_range=None,
                 phase_offset=0.0):
    """The eight values of ``train.py:535-566`` for one view as a detached float32 device tensor, in the order of ``VALUES``:
    ``l1, psnr`` of ``image`` against ``gt_image`` [C <= 3, H, W]; ``l1_p, l2_p, psnr_p`` of the selected ToF channels ``tof``
    against ``gt_tof`` [C <= 3, Ht, Wt] (``rendered_phasor[:n]``, or one quad plane as ``[1, Ht, Wt]``; planes of a wider
    tensor are read in place); ``l1_d, l2_d`` of ``depth`` against ``gt_depth`` [1, Ht, Wt]; ``l2_d_tof`` of the ToF depth of
    ``phasor`` [>=2, Ht, Wt] (planes 0 and 1, ``depth_from_tof_torch`` with ``depth_range`` / ``phase_offset``, each a number
    taken by value or a one-element float32 device tensor read when the kernel runs) against ``gt_depth``.  The colour
    camera and the ToF sensor may have different image sizes.  An absent group leaves 0 in its values.  Nothing is read on
    the host."""
    row = torch.empty((_lib.METRICS_ROW_WORDS,), device=_first_device(image, tof, depth, phasor, gt_depth), dtype=torch.float32)
    _launch(row, None, None, image, gt_image, tof, gt_tof, depth, gt_depth, phasor, depth_range, phase_offset)
    return row[:len(VALUES)]


class EvalReport:
    """The eight sums of one evaluation pass (``train.py:516-517``) as doubles on the device::

        report = metrics.EvalReport()
        for viewpoint in cameras:
            ...
            report.add_view(image=..., gt_image=..., tof=..., gt_tof=..., depth=..., gt_depth=..., phasor=..., depth_range=...,
                            phase_offset=...)                      # no host read; captured or not
        res = report.result()                                      # the pass's one blocking read

    ``add_view`` takes ``view_metrics``'s arguments; its finish kernel adds the view's eight values in double, in a fixed
    order by one thread (bit-reproducible), counts the view and ORs the groups it saw into ``present``.  ``result`` divides by
    the number of views as ``train.py:570-579`` does; ``reset`` zeroes the sums with a kernel."""

    def __init__(self, device=None):
        lib = _lib.load()
        self.device = _args.indexed_device(_TAG, "an EvalReport", device)
        # eight doubles, then the view count and the present word (GFT_METRICS_ACC_*): 9 doubles' worth, 8-byte aligned
        self._sums = torch.empty((_lib.METRICS_ACC_WORDS // 2,), device=self.device, dtype=torch.float64)
        # the scratch of the largest launch there is, once: a graph captured by an earlier add_view keeps its address
        self._partials = torch.empty((int(lib.gft_metrics_blocks(1 << 40)), _lib.METRICS_PARTIAL_WORDS), device=self.device,
                                     dtype=torch.float32)
        self.reset()

    def reset(self):
        """Zero the sums, the view count and ``present`` (one kernel; on the current stream)."""
        with _lib.on_device(self.device):
            _lib.check(_lib.load().gft_metrics_reset(_lib.raw_stream(self.device), self._sums.data_ptr()))

    def add_view(self, image=None, gt_image=None, tof=None, gt_tof=None, depth=None, gt_depth=None, phasor=None, depth_range=None,
                 phase_offset=0.0):
        """``view_metrics`` of the same arguments, added into the sums.  Returns nothing: the values are the device's."""
        _launch(None, self._sums, self._partials, image, gt_image, tof, gt_tof, depth, gt_depth, phasor, depth_range, phase_offset)

    def result(self):
        """The pass's averages as a dict: the eight names of ``VALUES`` (Python floats, each sum divided by the number of
        views), ``views`` and ``present`` (the OR of ``_lib.METRICS_HAS_*`` over the views).  One blocking read."""
        host = self._sums.cpu().numpy()
        words = host.view(np.uint32)
        views, present = int(words[_lib.METRICS_ACC_VIEWS]), int(words[_lib.METRICS_ACC_PRESENT])
        if views < 1:
            raise RuntimeError("gftorf_amd.metrics: no view was added to this EvalReport")
        out = {name: float(host[k]) / views for k, name in enumerate(VALUES)}
        out.update(views=views, present=present)
        return out
