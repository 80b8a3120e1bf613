"""The Gaussian model's PLY files on the device (``csrc/k_ply.hip``, ``include/gftorf_ply.h``).

``GaussianModel.save_ply`` (``scene/gaussian_model.py:340-367``) brings 7 or 12 tensors to the host with blocking copies,
concatenates them and fills a structured array from one Python tuple per Gaussian; ``Scene.save`` does so twice.
``load_ply`` (``:378-454``) copies ~95 columns one by one into float64 arrays and uploads 11 tensors.  The file's body is
nothing but the model's float32 values, one row per Gaussian in the column order of ``construct_list_of_attributes``, so:

``submit(pc, path_sibr, path_full)``  one launch forms the rows of both files in a device buffer and returns a ``PlyJob``;
    ``PlyJob.finish()`` writes the headers and streams the rows through two pinned buffers into the files.
``save_ply(pc, path, sibr_only)`` / ``save_pair(pc, path_sibr, path_full)``  the model's method and the two lines of
    ``Scene.save``.
``read_gaussians(path, device, max_sh_degree)``  the header parsed, the body streamed through pinned memory and scattered
    by one launch per chunk into the 11 tensors of ``load_ply``; ``load_ply(pc, path)`` adopts them.
``columns(pc_or_shapes, full)``, ``header(names, P)``, ``parse_header(data)``  the file's text side, pure Python (shared with
    ``gftorf_amd.pcd``, whose input clouds also hold uchar columns).

The values are moved bit for bit.  There is no CPU path; the reader handles the files this layout covers (binary little
endian, float properties) and refuses the rest by name.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _args, _lib

_TAG = "gftorf_amd.ply"
ROWS_PER_GROUP = _lib.PLY_ROWS                  # rows a workgroup of either kernel takes
MAX_COLUMNS = _lib.PLY_MAX_COLUMNS              # columns of a row the kernels' LDS tile holds
CHUNK_BYTES = 8 << 20                           # default size of a staged chunk
_REFUSAL = "; gftorf_amd.ply reads binary_little_endian files whose first element is `vertex` with scalar float properties: " \
           "load this file with the reference's own GaussianModel.load_ply (plyfile)"

# the column blocks of a row in order: (prefix of the column names, the model's attribute or None for zeros, is a [P, n, c]
# feature tensor)
_SIBR_BLOCKS = (("xyz", "_xyz", False), ("normals", None, False), ("f_dc", "_features_dc_color", True),
                ("f_rest", "_features_rest_color", True), ("opacity", "_opacity", False), ("scale", "_scaling", False),
                ("rot", "_rotation", False))
_FULL_BLOCKS = _SIBR_BLOCKS + (("phase_f_dc", "_features_dc_phase", True), ("phase_f_rest", "_features_rest_phase", True),
                               ("amp_f_dc", "_features_dc_amp", True), ("amp_f_rest", "_features_rest_amp", True),
                               ("f_seg_color", "_features_seg_color", False))


def _block_widths(pc_or_shapes):
    """{block: columns}: from a model's tensors, as ``construct_list_of_attributes`` counts them, or from a dict with ``n``
    (SH coefficients beside the DC one), ``s`` (scaling columns) and ``S`` (seg colour columns)"""
    if isinstance(pc_or_shapes, dict):
        n, s, S = (int(pc_or_shapes[k]) for k in ("n", "s", "S"))
        return {"xyz": 3, "normals": 3, "f_dc": 3, "f_rest": 3 * n, "opacity": 1, "scale": s, "rot": 4, "phase_f_dc": 1,
                "phase_f_rest": n, "amp_f_dc": 1, "amp_f_rest": n, "f_seg_color": S}
    out = {"xyz": 3, "normals": 3, "opacity": 1}
    for name, attr, feature in _FULL_BLOCKS:
        if name in out:
            continue
        t = getattr(pc_or_shapes, attr, None)
        if t is None:
            continue
        out[name] = int(t.shape[1]) * int(t.shape[2]) if feature else int(t.shape[1])
    return out


def columns(pc_or_shapes, full=False):
    """The property names of a row in order (``construct_list_of_attributes(save_all=full)``).  ``pc_or_shapes``: the model, or
    ``{"n": 15, "s": 3, "S": 3}``."""
    w = _block_widths(pc_or_shapes)
    names = ["x", "y", "z", "nx", "ny", "nz"]
    for block, _, _ in (_FULL_BLOCKS if full else _SIBR_BLOCKS)[2:]:
        names += ["opacity"] if block == "opacity" else ["%s_%d" % (block, i) for i in range(w[block])]
    return names


PROPERTY_BYTES = {"float": 4, "uchar": 1}      # the property types the kernels move, as plyfile names them (f4, u1)


def header(names, P):
    """The PLY header of P vertices with the properties ``names``, as bytes: a name alone is a float property, a
    ``(name, "uchar")`` pair one of that type (``gftorf_amd.pcd``'s colour columns)"""
    props = [("float", n) if isinstance(n, str) else (n[1], n[0]) for n in names]
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % P] + ["property %s %s" % p for p in props] + ["end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def parse_header(data, uchar=False):
    """``(P, names, offset)`` of a file that begins with the bytes ``data``: the vertex count, the vertex element's property names
    in file order and the offset of the body.  NotImplementedError for what the reader does not handle.  With ``uchar`` the
    vertex element may also hold uchar properties and the names come as ``(name, type)`` pairs (``gftorf_amd.pcd.fetch``)."""
    end = data.find(b"end_header\n")
    lines = data[:end].decode("ascii", "replace").split("\n") if end >= 0 else []
    if not lines or lines[0].strip() != "ply":
        raise ValueError("%s: not a PLY file (no `ply` ... `end_header` text at its start)" % _TAG)
    P, names, element = None, [], 0
    for line in lines[1:]:
        words = line.split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "format":
            if words[1:2] != ["binary_little_endian"]:
                raise NotImplementedError("%s: the file's format is `%s`%s" % (_TAG, " ".join(words[1:]), _REFUSAL))
        elif words[0] == "element":
            element += 1
            if element == 1:
                if words[1] != "vertex":
                    raise NotImplementedError("%s: the file's first element is `%s`%s" % (_TAG, words[1], _REFUSAL))
                P = int(words[2])
        elif words[0] == "property" and element == 1:
            kind = {"float32": "float", "uint8": "uchar"}.get(words[1], words[1])
            if kind not in (("float", "uchar") if uchar else ("float",)) or len(words) != 3:
                raise NotImplementedError("%s: the vertex element has the property `%s`%s" % (_TAG, " ".join(words[1:]), _REFUSAL))
            names.append((words[2], kind) if uchar else words[2])
    if P is None or P < 0:
        raise ValueError("%s: the header names no vertex element" % _TAG)
    if len(set(n[0] if uchar else n for n in names)) != len(names):
        raise ValueError("%s: the vertex element names a property twice" % _TAG)
    return P, names, end + len(b"end_header\n")


# ---- pinned staging -------------------------------------------------------------------------------------------------------

_staging = {"bytes": 0, "host": None, "events": None}


def _stage(nbytes):
    """two pinned buffers of at least nbytes with an event each, kept between calls (pinning memory is slow)"""
    if _staging["bytes"] < nbytes:
        _staging["host"] = [torch.empty((nbytes,), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        _staging["events"] = [torch.cuda.Event() for _ in range(2)]
        _staging["bytes"] = nbytes
    return _staging["host"], _staging["events"]


# ---- saving ---------------------------------------------------------------------------------------------------------------

def _model_blocks(pc, full):
    """[(tensor or None, width, channels)] of the row's blocks, P and the device"""
    xyz = getattr(pc, "_xyz", None)
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2:
        raise TypeError("%s: the model's _xyz must be a [P, 3] tensor" % _TAG)
    P = int(xyz.shape[0])
    blocks, named = [], []
    for name, attr, feature in (_FULL_BLOCKS if full else _SIBR_BLOCKS):
        if attr is None:
            blocks.append((None, 3, 0))
            continue
        t = getattr(pc, attr, None)
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: the model's %s must be a tensor, got %s" % (_TAG, attr, type(t).__name__))
        t = t.detach()
        if t.dim() != (3 if feature else 2) or int(t.shape[0]) != P:
            raise RuntimeError("%s: %s must be [%d, %s], got %s" % (_TAG, attr, P, "n, c" if feature else "w", list(t.shape)))
        named.append((t, attr))
        if t.dtype != torch.float32:
            t = t.to(torch.float32)
        t = t.contiguous()
        if feature:
            blocks.append((t, int(t.shape[1]) * int(t.shape[2]), int(t.shape[2]) if t.numel() else 1))
        else:
            blocks.append((t, int(t.shape[1]), 1))
    dev = _args.devices(_TAG, "PLY", named)
    return blocks, P, dev


class PlyJob:
    """The rows of one ``submit``, held in a device buffer until ``finish`` has written them."""

    def __init__(self, sheets, P, event, device):
        self._sheets, self.P, self._event, self._device = sheets, P, event, device      # sheets: [(path, names, tensor [P * K])]
        self._done = False

    def finish(self, chunk_rows=None):
        """Writes the files: each header, then the rows in chunks of ``chunk_rows`` through two pinned buffers, the copy of
        chunk i + 1 running while chunk i is written.  Waits for the device; a second call does nothing."""
        if self._done:
            return
        with _lib.on_device(self._device):
            stream = torch.cuda.current_stream(self._device)
            stream.wait_event(self._event)
            for path, names, sheet in self._sheets:
                K = len(names)
                rows = max(1, int(chunk_rows) if chunk_rows is not None else CHUNK_BYTES // (4 * K))
                folder = os.path.dirname(path)
                if folder:
                    os.makedirs(folder, exist_ok=True)
                data = sheet.view(torch.uint8)
                bounds = [(r * K * 4, min(r + rows, self.P) * K * 4) for r in range(0, self.P, rows)]
                host, events = _stage(rows * K * 4)

                def copy(i):
                    a, b = bounds[i]
                    host[i & 1][:b - a].copy_(data[a:b], non_blocking=True)
                    events[i & 1].record(stream)

                with open(path, "wb") as f:
                    f.write(header(names, self.P))
                    if bounds:
                        copy(0)
                    for i, (a, b) in enumerate(bounds):
                        if i + 1 < len(bounds):
                            copy(i + 1)
                        events[i & 1].synchronize()
                        f.write(memoryview(host[i & 1].numpy())[:b - a])
        self._sheets = []               # the device buffer is free
        self._done = True


def submit(pc, path_sibr=None, path_full=None):
    """Forms the rows of ``point_cloud.ply`` (``path_sibr``) and / or ``point_cloud_full.ply`` (``path_full``) from the model
    ``pc`` in one launch on the current stream and returns a ``PlyJob``; nothing is read on the host and nothing is waited
    for.  The job holds a snapshot: the launch is stream-ordered, so the model may be stepped, densified or freed as soon as
    this returns.  Device memory: one buffer of 4 * (K_full + K_sibr) bytes per Gaussian for the sheets asked for (K = the
    columns of a row: 97 and 62 at SH degree 3), held until ``finish``.  Model tensors that are not contiguous float32 are
    made so first."""
    if path_sibr is None and path_full is None:
        raise ValueError("%s: submit needs path_sibr, path_full or both" % _TAG)
    full = path_full is not None
    blocks, P, dev = _model_blocks(pc, full)
    lib = _lib.load()
    names_full = columns(pc, full)
    K_full = len(names_full)
    names_sibr = columns(pc, False)
    K_sibr = len(names_sibr)
    if K_full > MAX_COLUMNS:
        raise ValueError("%s: a row of %d columns; the kernels hold at most %d" % (_TAG, K_full, MAX_COLUMNS))
    both = full and path_sibr is not None
    first = (P * K_full + 3) // 4 * 4                                   # the second sheet starts 16-byte aligned
    buf = torch.empty((max(4, first + (P * K_sibr if both else 0)),), device=dev, dtype=torch.float32)
    count = len(blocks)
    sources = (C.c_void_p * count)(*[None if t is None or t.numel() == 0 else t.data_ptr() for t, _, _ in blocks])
    widths = (C.c_int32 * count)(*[w for _, w, _ in blocks])
    channels = (C.c_int32 * count)(*[c for _, _, c in blocks])
    if sum(widths) != K_full:
        raise RuntimeError("%s: the model's tensors hold %d floats per Gaussian, the row has %d columns" % (_TAG, sum(widths), K_full))
    with _lib.on_device(dev):
        _lib.check(lib.gft_ply_pack(_lib.raw_stream(dev), P, count, sources, widths, channels, K_full, K_sibr, buf.data_ptr(),
                                    buf[first:].data_ptr() if both else None))
        event = torch.cuda.Event()
        event.record()
    sheets = [(path_full if full else path_sibr, names_full, buf[:P * K_full])]
    if both:
        sheets.insert(0, (path_sibr, names_sibr, buf[first:first + P * K_sibr]))
    return PlyJob(sheets, P, event, dev)


def save_ply(pc, path, sibr_only=True, chunk_rows=None):
    """``GaussianModel.save_ply(path, sibr_only)``"""
    job = submit(pc, path_sibr=path) if sibr_only else submit(pc, path_full=path)
    job.finish(chunk_rows=chunk_rows)


def save_pair(pc, path_sibr, path_full, chunk_rows=None):
    """The two ``save_ply`` lines of ``Scene.save``: the model is read once, by one launch, for both files"""
    submit(pc, path_sibr=path_sibr, path_full=path_full).finish(chunk_rows=chunk_rows)


# ---- loading --------------------------------------------------------------------------------------------------------------

# the tensors of load_ply in order: (key, the model's attribute, file columns -> table)
TENSORS = ("xyz", "features_dc_color", "features_rest_color", "features_dc_phase", "features_rest_phase", "features_dc_amp",
           "features_rest_amp", "opacity", "scaling", "rotation", "features_seg_color")


def _file_layout(names, max_sh_degree):
    """{key: (shape behind P, [file column of every float of a row])} by the rules of load_ply"""
    col = {n: i for i, n in enumerate(names)}

    def one(name):
        if name not in col:
            raise ValueError("%s: the file has no property `%s`, which GaussianModel.load_ply reads" % (_TAG, name))
        return col[name]

    def family(prefix):
        return [col[n] for n in sorted((n for n in names if n.startswith(prefix)), key=lambda x: int(x.split("_")[-1]))]

    rest_color, rest_phase, rest_amp = family("f_rest_"), family("phase_f_rest_"), family("amp_f_rest_")
    if max_sh_degree is not None:
        n = (int(max_sh_degree) + 1) ** 2 - 1
        for what, got, want in (("f_rest_", len(rest_color), 3 * n), ("phase_f_rest_", len(rest_phase), n),
                                ("amp_f_rest_", len(rest_amp), n)):
            if got != want:
                raise ValueError("%s: the file has %d `%s*` properties, max_sh_degree = %d needs %d" % (_TAG, got, what, max_sh_degree, want))
    elif len(rest_color) % 3:
        raise ValueError("%s: the file has %d `f_rest_*` properties, not a multiple of 3" % (_TAG, len(rest_color)))
    n = len(rest_color) // 3
    scale, rot, seg = family("scale_"), family("rot"), family("f_seg_color_")
    return {
        "xyz": ((3,), [one("x"), one("y"), one("z")]),
        "features_dc_color": ((1, 3), [one("f_dc_0"), one("f_dc_1"), one("f_dc_2")]),
        # [p, j, ch] = the sorted property ch * n + j: reshape(P, 3, n).transpose(1, 2)
        "features_rest_color": ((n, 3), [rest_color[ch * n + j] for j in range(n) for ch in range(3)]),
        "features_dc_phase": ((1, 1), [one("phase_f_dc_0")]),
        "features_rest_phase": ((len(rest_phase), 1), rest_phase),
        "features_dc_amp": ((1, 1), [one("amp_f_dc_0")]),
        "features_rest_amp": ((len(rest_amp), 1), rest_amp),
        "opacity": ((1,), [one("opacity")]),
        "scaling": ((len(scale),), scale),
        "rotation": ((len(rot),), rot),
        "features_seg_color": ((len(seg),), seg),
    }


def read_gaussians(path, device=None, max_sh_degree=None, chunk_rows=None):
    """The tensors ``GaussianModel.load_ply`` builds from the file, float32 on ``device``, as a dict: ``xyz`` [P, 3],
    ``features_dc_color`` [P, 1, 3], ``features_rest_color`` [P, n, 3], ``features_dc_phase`` / ``features_dc_amp`` [P, 1, 1],
    ``features_rest_phase`` / ``features_rest_amp`` [P, n, 1], ``opacity`` [P, 1], ``scaling`` [P, s], ``rotation`` [P, 4],
    ``features_seg_color`` [P, S].  Properties are found by name in any order; the families ``f_rest_*``, ``phase_f_rest_*``,
    ``amp_f_rest_*``, ``scale_*``, ``rot*`` and ``f_seg_color_*`` are sorted by their integer suffix and other properties are
    ignored.  With ``max_sh_degree`` the three counts ``load_ply`` asserts are checked (ValueError).  The values are the
    file's float32 bits (the reference's way through float64 is exact).  The body is streamed in chunks of ``chunk_rows``
    through two pinned buffers; one launch per chunk scatters it."""
    dev = _args.indexed_device(_TAG, "a loaded model", device)
    lib = _lib.load()
    with open(path, "rb") as f:
        head = b""
        while b"end_header\n" not in head and len(head) < (1 << 20):
            piece = f.read(1 << 16)
            if not piece:
                break
            head += piece
        P, names, offset = parse_header(head)
        K = len(names)
        layout = _file_layout(names, max_sh_degree)
        if K > MAX_COLUMNS:
            raise ValueError("%s: the file has %d properties per vertex; the loader takes at most %d" % (_TAG, K, MAX_COLUMNS))
        out = {key: torch.empty((P,) + layout[key][0], device=dev, dtype=torch.float32) for key in TENSORS}
        count = len(TENSORS)
        widths = (C.c_int32 * count)(*[len(layout[key][1]) for key in TENSORS])
        flat = [c for key in TENSORS for c in layout[key][1]]
        table = (C.c_int32 * max(1, len(flat)))(*flat)
        dests = (C.c_void_p * count)(*[_args.ptr_nonempty(out[key]) for key in TENSORS])
        rows = max(1, int(chunk_rows) if chunk_rows is not None else CHUNK_BYTES // (4 * K))
        f.seek(offset)
        with _lib.on_device(dev):
            host, events = _stage(rows * K * 4)
            chunks = [torch.empty((rows * K,), device=dev, dtype=torch.float32) for _ in range(2 if P > rows else 1)] if P else []
            used = [False, False]
            for i, r0 in enumerate(range(0, P, rows)):
                slot, nrows = i & 1, min(rows, P - r0)
                nbytes = nrows * K * 4
                if used[slot]:
                    events[slot].synchronize()                      # the copy out of this buffer two chunks ago
                got = f.readinto(memoryview(host[slot].numpy())[:nbytes])
                if got != nbytes:
                    raise ValueError("%s: %s ends inside vertex %d of %d" % (_TAG, path, r0 + (got or 0) // (4 * K), P))
                chunk = chunks[slot]
                chunk.view(torch.uint8)[:nbytes].copy_(host[slot][:nbytes], non_blocking=True)
                events[slot].record()
                used[slot] = True
                _lib.check(lib.gft_ply_unpack(_lib.raw_stream(dev), nrows, r0, K, chunk.data_ptr(), count, dests, widths, table))
            for slot in range(2):
                if used[slot]:
                    events[slot].synchronize()
    return out


def load_ply(pc, path, chunk_rows=None):
    """``GaussianModel.load_ply(path)``: the file's tensors become the model's parameters (``requires_grad``) on the current
    HIP device and ``active_sh_degree = max_sh_degree``"""
    tensors = read_gaussians(path, None, max_sh_degree=pc.max_sh_degree, chunk_rows=chunk_rows)
    for key in TENSORS:
        setattr(pc, "_" + key, torch.nn.Parameter(tensors[key].requires_grad_(True)))
    pc.active_sh_degree = pc.max_sh_degree
