"""PNG files formed on the device (``csrc/k_png.hip``, ``csrc/gft_png_coder.h``, ``include/gftorf_png.h``).

The reference writes every image of a rendered view (``render.py:105-189``, ``render_ftorf_viz_traj.py:237-259``) and of a
debug iteration (``train.py:298-398``) with ``imageio.imwrite(....png)``: zlib on the host, one image after the other.
``gftorf_amd.present`` already forms those images as uint8 bytes on the device; here the device also forms the files:

``encode(images, level=1)``  every image of a dict as the complete bytes of a ``.png`` file in one device buffer, in three
    launches whatever the number of images (two at level 0); no host read, no atomic on global memory, no memset, so the call
    can be captured in a graph.  Returns a ``PngBatch``; ``PngBatch.to_host()`` is the one blocking read.
``PngSheets``  ``present.ViewSheets`` with the encoder behind the sheet: ``submit_view`` / ``submit_debug`` / ``submit_flow``
    enqueue the ``present`` call, the encode and one asynchronous copy to pinned memory; ``ready`` hands out the files.
``save(files, path_of)``  one ``write`` per file.

``level`` 0 stores the bytes (filter type 0, stored deflate blocks; the size is ``bound(H, W, channels)`` exactly); ``level`` 1,
the default, chooses a filter per scanline and codes matches -- at five fixed distances and at the first position whose four
bytes hash alike -- with deflate's fixed Huffman codes, or stores a 32 KiB segment where that is shorter.  The file bytes are this encoder's own, not imageio's (PNG files of the same
pixels differ between encoders); any PNG reader decodes them to exactly the source bytes, and they are the same from run to
run.  ``tests/png_ref.py`` restates the encoder in numpy.  There is no CPU path.
"""
import numpy as np
import torch

from . import _args, _lib, present

_TAG = "gftorf_amd.png"
SEGMENT = _lib.PNG_SEGMENT                      # bytes of a filtered stream one workgroup codes into one IDAT chunk
MAX_IMAGES = _lib.PNG_MAX_IMAGES                # images of one encode call
_ALIGN = 16                                     # every slot of the output buffer starts on such a boundary


def bound(H, W, channels):
    """The slot size of an H x W image with `channels` samples per pixel: the size of its level-0 file and an upper bound of
    its level-1 file"""
    n = int(_lib.load().gft_png_bound(int(H), int(W), int(channels)))
    if n < 0:
        raise ValueError("%s: no PNG file for H=%s W=%s channels=%s (channels must be 1, 3 or 4)" % (_TAG, H, W, channels))
    return n


def _expand(images):
    """[(name, tensor [H, W] or [H, W, C], H, W, C, row stride)] of a dict of images; a [4, H, W] quad becomes four"""
    if not isinstance(images, dict) or not images:
        raise ValueError("%s: images must be a non-empty dict of name -> uint8 tensor" % _TAG)
    flat = []
    for name, t in images.items():
        t = _args.tensor(_TAG, t, str(name), dtypes=(torch.uint8,))
        if t.dim() == 3 and t.shape[2] not in (3, 4) and t.shape[0] == 4:
            flat += [("%s%d" % (name, k), t[k]) for k in range(4)]
        else:
            flat.append((str(name), t))
    rows = []
    for name, t in flat:
        if t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] not in (1, 3, 4)) or t.shape[0] < 1 or t.shape[1] < 1:
            raise RuntimeError("%s: %s must be [H, W], [H, W, 3], [H, W, 4] or a [4, H, W] quad, got %s" % (_TAG, name, list(t.shape)))
        H, W, Cn = int(t.shape[0]), int(t.shape[1]), int(t.shape[2]) if t.dim() == 3 else 1
        inner = (t.dim() == 2 or Cn == 1 or t.stride(2) == 1) and (W == 1 or t.stride(1) == Cn)
        if not inner or (H > 1 and t.stride(0) < W * Cn):
            raise RuntimeError("%s: %s has strides %s: the bytes of a row must be contiguous and the rows must not overlap (a row "
                               "stride is fine)" % (_TAG, name, list(t.stride())))
        rows.append((name, t, H, W, Cn, int(t.stride(0)) if H > 1 else W * Cn))
    if len(set(r[0] for r in rows)) != len(rows):
        raise ValueError("%s: two images are named alike: %s" % (_TAG, sorted(r[0] for r in rows)))
    if len(rows) > MAX_IMAGES:
        raise ValueError("%s: %d images; one call takes at most %d" % (_TAG, len(rows), MAX_IMAGES))
    return rows


def layout(shapes):
    """``(bytes of the batch's buffer, [slot offset per image], offset of the int64 sizes)`` for images of the shapes
    ``[(H, W, channels)]``: the slots in order, each ``bound`` bytes on a 16-byte boundary, then one int64 per image"""
    offsets, at = [], 0
    for H, W, Cn in shapes:
        offsets.append(at)
        at += (bound(H, W, Cn) + _ALIGN - 1) // _ALIGN * _ALIGN
    return at + 8 * len(offsets), offsets, at


def _table(rows, offsets):
    table = (_lib.PngImage * len(rows))()
    for k, (name, t, H, W, Cn, stride) in enumerate(rows):
        table[k].src, table[k].row_stride, table[k].out_offset = t.data_ptr(), stride, offsets[k]
        table[k].H, table[k].W, table[k].channels = H, W, Cn
    return table


def scratch_bytes(shapes):
    """bytes of scratch an encode of images of the shapes ``[(H, W, channels)]`` takes"""
    table = (_lib.PngImage * len(shapes))()
    for k, (H, W, Cn) in enumerate(shapes):
        table[k].H, table[k].W, table[k].channels = int(H), int(W), int(Cn)
    n = int(_lib.load().gft_png_scratch_bytes(len(shapes), table))
    if n < 0:
        raise ValueError("%s: no scratch for the shapes %s" % (_TAG, list(shapes)))
    return n


class PngBatch:
    """The files of one ``encode``: ``buffer`` (uint8, device) holds file k at ``buffer[offsets[k] : offsets[k] + sizes[k]]``;
    ``names`` and ``offsets`` (host ints, fixed by the shapes) are in the order of the images, ``sizes`` is a device int64
    tensor, a view of the buffer's last ``8 * len(names)`` bytes, so that one copy of ``buffer`` brings everything."""

    def __init__(self, names, buffer, offsets, sizes):
        self.names, self.buffer, self.offsets, self.sizes = names, buffer, offsets, sizes

    @staticmethod
    def split(names, offsets, host):
        """{name: memoryview of the file's bytes} over a host copy of ``buffer`` (a uint8 numpy array)"""
        count = len(names)
        sizes = host[len(host) - 8 * count:].view(np.int64)
        view = memoryview(host)
        return {name: view[offsets[k]:offsets[k] + int(sizes[k])] for k, name in enumerate(names)}

    def to_host(self):
        """``{name: bytes}``: the one blocking read"""
        host = self.buffer.cpu().numpy()
        return {name: bytes(v) for name, v in self.split(self.names, self.offsets, host).items()}


def encode(images, level=1, out=None, scratch=None):
    """The PNG files of ``images``, a dict of name -> uint8 device tensor ``[H, W]`` (gray), ``[H, W, 3]`` (RGB) or
    ``[H, W, 4]`` (RGBA).  The bytes of a row must be contiguous; a row stride is allowed, so views into a ``present`` sheet
    are read where they lie.  A ``[4, H, W]`` tensor (the quad images; a tensor whose last dimension is 3 or 4 is a colour
    image) becomes the four gray images ``name0 .. name3``.  At most ``MAX_IMAGES`` images, all on one HIP device.

    ``level``: 0 or 1 (see the module's text).  ``out``: a uint8 device tensor of at least ``layout(shapes)[0]`` bytes, 16-byte
    aligned, to write into; else a new one.  ``scratch``: a uint8 device tensor of at least ``scratch_bytes(shapes)`` bytes to
    work in; else a new one.  Everything runs on the current stream; nothing is read on the host."""
    rows = _expand(images)
    if level not in (0, 1):
        raise ValueError("%s: level must be 0 or 1, got %r" % (_TAG, level))
    dev = _args.devices(_TAG, "PNG", [(t, name) for name, t, *_ in rows])
    shapes = [(H, W, Cn) for _, _, H, W, Cn, _ in rows]
    total, offsets, sizes_at = layout(shapes)
    if out is None:
        out = torch.empty((total,), device=dev, dtype=torch.uint8)
    else:
        out = _args.tensor(_TAG, out, "out", dtypes=(torch.uint8,))
        _args.devices(_TAG, "PNG", [(rows[0][1], rows[0][0]), (out, "out")])
        if out.dim() != 1 or not out.is_contiguous() or out.numel() < total or out.data_ptr() % _ALIGN:
            raise ValueError("%s: out must be a contiguous 16-byte aligned uint8 vector of at least %d bytes for these images, got %s"
                             % (_TAG, total, list(out.shape)))
        out = out[:total]
    lib = _lib.load()
    need = scratch_bytes(shapes)
    if scratch is None:
        scratch = torch.empty((need,), device=dev, dtype=torch.uint8)
    else:
        scratch = _args.tensor(_TAG, scratch, "scratch", dtypes=(torch.uint8,))
        _args.devices(_TAG, "PNG", [(rows[0][1], rows[0][0]), (scratch, "scratch")])
        if scratch.dim() != 1 or not scratch.is_contiguous() or scratch.numel() < need or scratch.data_ptr() % _ALIGN:
            raise ValueError("%s: scratch must be a contiguous 16-byte aligned uint8 vector of at least %d bytes for these images, got %s"
                             % (_TAG, need, list(scratch.shape)))
    sizes = out[sizes_at:].view(torch.int64)
    with _lib.on_device(dev):
        _lib.check(lib.gft_png_encode(_lib.raw_stream(dev), len(rows), _table(rows, offsets), int(level), out.data_ptr(), sizes_at,
                                      sizes.data_ptr(), scratch.data_ptr(), scratch.numel()))
    return PngBatch([r[0] for r in rows], out, offsets, sizes)


def save(files, path_of):
    """Writes ``files`` (``{name: bytes-like}``, as ``PngBatch.to_host`` or ``PngSheets.ready`` give them) with one ``write``
    per file, to ``path_of(name)``; a float array (the two depths of a view) goes through ``numpy.save`` to that path."""
    for name, data in files.items():
        path = path_of(name)
        if isinstance(data, np.ndarray):
            np.save(path, data)
        else:
            with open(path, "wb") as f:
                f.write(data)


class PngSheets:
    """Pinned staging for a render or debug loop, as ``present.ViewSheets``, with the files formed on the device::

        sheets = png.PngSheets(slots=2)
        for vid, view in enumerate(views):
            pkg = render_eval(view, ...)
            sheets.submit_view(vid, image=pkg["render"], phasor=pkg["render_phasor"], ..., ranges=ranges.tensor, zplanes=zp)
            for tag, files in sheets.ready():                 # the views whose copy has completed, oldest first
                png.save(files, lambda name: "%s/%05d_%s.png" % (folder, tag, name))
        for tag, files in sheets.ready(wait=True):
            png.save(files, ...)

    ``submit*`` never wait: with every slot in flight or handed out they raise.  ``ready`` yields ``(tag, {name: memoryview of
    the file's bytes})``; float images (a view's ``depth_tof_f`` and ``depth_norm_f``, which the reference ``np.save``s) come
    as numpy arrays.  What ``ready`` yields lies in the slot's pinned memory and belongs to the slot, which is free again when
    the loop moves past it (or with the next ``ready`` call)."""

    def __init__(self, slots=2, level=1):
        _lib.load()
        if int(slots) < 1:
            raise ValueError("%s: PngSheets needs at least one slot, got %s" % (_TAG, slots))
        if level not in (0, 1):
            raise ValueError("%s: level must be 0 or 1, got %r" % (_TAG, level))
        self.level = level
        self._slots = [dict(state="free", bufs={}, event=None) for _ in range(int(slots))]
        self._order = []          # slots in flight, oldest first
        self._lent = []           # slots whose files the caller holds

    def _release(self):
        for s in self._lent:
            s["state"] = "free"
        self._lent = []

    def _free_slot(self):
        slot = next((s for s in self._slots if s["state"] == "free"), None)
        if slot is None:
            raise RuntimeError("%s: all %d slots of this PngSheets are in flight; take the finished files with ready()"
                               % (_TAG, len(self._slots)))
        return slot

    @staticmethod
    def _buf(slot, key, n, dev, dtype=torch.uint8, pinned=False):
        """the slot's buffer `key` of at least n elements, kept between submits"""
        b = slot["bufs"].get(key)
        if b is None or b.numel() < n or (not pinned and b.device != dev):
            b = torch.empty((n,), dtype=dtype, pin_memory=True) if pinned else torch.empty((n,), device=dev, dtype=dtype)
            slot["bufs"][key] = b
        return b

    def _submit(self, slot, tag, images):
        """encode + one copy of the files and sizes (+ one per float image) + event, on the current stream"""
        coded = {k: t for k, t in images.items() if t.dtype == torch.uint8}
        plain = {k: t for k, t in images.items() if t.dtype != torch.uint8}
        rows = _expand(coded)
        dev = rows[0][1].device
        shapes = [(H, W, Cn) for _, _, H, W, Cn, _ in rows]
        total = layout(shapes)[0]
        extra = sum(t.numel() * t.element_size() for t in plain.values())
        out = self._buf(slot, "out", total, dev)
        host = self._buf(slot, "host", total + _ALIGN + extra, dev, pinned=True)
        batch = encode(coded, level=self.level, out=out, scratch=self._buf(slot, "scratch", scratch_bytes(shapes), dev))
        host[:total].copy_(batch.buffer, non_blocking=True)
        arrays, at = {}, (total + _ALIGN - 1) // _ALIGN * _ALIGN
        for name, t in plain.items():
            n = t.numel() * t.element_size()
            host[at:at + n].copy_(t.contiguous().view(-1).view(torch.uint8), non_blocking=True)
            arrays[name] = host.numpy()[at:at + n].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape))
            at += n
        if slot["event"] is None:
            slot["event"] = torch.cuda.Event()
        slot["event"].record()
        slot.update(state="flight", tag=tag, names=batch.names, offsets=batch.offsets, total=total, arrays=arrays)
        self._order.append(slot)

    def submit(self, tag, images):
        """``encode(images)`` into a free slot; float tensors among ``images`` are copied as they are"""
        slot = self._free_slot()
        if not isinstance(images, dict) or not any(isinstance(t, torch.Tensor) and t.dtype == torch.uint8 for t in images.values()):
            raise ValueError("%s: nothing to encode: images must hold at least one uint8 tensor" % _TAG)
        for name, t in images.items():
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s: %s must be a tensor, got %s" % (_TAG, name, type(t).__name__))
        self._submit(slot, tag, images)

    def submit_view(self, tag, **view):
        """``present.view_images(**view)`` into the slot's sheet, then the files of its images"""
        slot = self._free_slot()
        first = next((v for v in (view.get(k) for k in ("image", "phasor", "depth", "dd")) if isinstance(v, torch.Tensor)), None)
        if first is None or first.dim() != 3:
            raise ValueError("%s: nothing to show: give image, phasor, depth or dd as [C, H, W] tensors" % _TAG)
        H, W = int(first.shape[1]), int(first.shape[2])
        full = present.sheet_layout(H, W, present._EVERY)[0]
        sheet = self._buf(slot, "sheet", full, first.device)
        rows = max(1, present.blocks(H * W)) * _lib.PRESENT_PARTIAL_WORDS
        partials = self._buf(slot, "partials", rows, first.device, dtype=torch.float32)
        images = present.view_images(out=sheet, _partials=partials.view(-1, _lib.PRESENT_PARTIAL_WORDS), **view)
        self._submit(slot, tag, images)

    def submit_debug(self, tag, **debug):
        """``present.debug_images(**debug)`` into the slot's sheet, then the files of its images"""
        slot = self._free_slot()
        keys = ("phasor", "gt_phasor", "depth", "phase_depth", "gt_phase_depth", "dd", "image", "gt_image", "gt_quad")
        first = next((v for v in (debug.get(k) for k in keys) if isinstance(v, torch.Tensor)), None)
        if first is None or first.dim() not in (2, 3):
            raise ValueError("%s: nothing to show: give phasor, depth, dd or image as [C, H, W] tensors, the ToF depths as [H, W] ones"
                             % _TAG)
        H, W = int(first.shape[-2]), int(first.shape[-1])
        full = present.debug_sheet_layout(H, W, present._DEBUG_EVERY)[0]
        sheet = self._buf(slot, "sheet", full, first.device)
        rows = present.debug_blocks(H * W) * _lib.DEBUGVIZ_PARTIAL_WORDS
        partials = self._buf(slot, "debug_partials", rows, first.device, dtype=torch.float32)
        images = present.debug_images(out=sheet, _partials=partials.view(-1, _lib.DEBUGVIZ_PARTIAL_WORDS), **debug)
        self._submit(slot, tag, images)

    def submit_flow(self, tag, flow, gt_flow):
        """``present.flow_images(flow, gt_flow)`` into the slot's sheet, then the files ``flow``, ``gt`` and ``error``"""
        slot = self._free_slot()
        if not isinstance(flow, torch.Tensor) or flow.dim() != 3:
            raise ValueError("%s: nothing to show: give flow as a [C, H, W] tensor" % _TAG)
        dev = _args.devices(_TAG, "PNG", [(flow, "flow")])
        H, W = int(flow.shape[1]), int(flow.shape[2])
        need = _lib.FLOWVIZ_IMAGES * H * W * 3
        sheet = self._buf(slot, "sheet", need, dev)[:need].view(_lib.FLOWVIZ_IMAGES, H, W, 3)
        partials = self._buf(slot, "flow_partials", present.flow_blocks(H * W) + 1, dev, dtype=torch.float32)
        present.flow_images(flow, gt_flow, out=sheet, _partials=partials)
        self._submit(slot, tag, {"flow": sheet[0], "gt": sheet[1], "error": sheet[2]})

    def ready(self, wait=False):
        """Yields (tag, files) of the submitted tags whose copy has completed, oldest first, and stops at the first that has
        not; ``wait=True`` waits for each instead, so every submitted tag comes out."""
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
            files = PngBatch.split(slot["names"], slot["offsets"], slot["bufs"]["host"].numpy()[:slot["total"]])
            files.update(slot["arrays"])
            yield slot["tag"], files
            self._release()
