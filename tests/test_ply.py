"""gftorf_amd.ply: the Gaussian model's PLY files (include/gftorf_ply.h, csrc/k_ply.hip).

The oracle is the reference's own statements (scene/gaussian_model.py:315-367, 378-454), restated here with torch and numpy:
``transpose(1, 2).flatten(start_dim=1)``, the concatenation in column order, the header text of a PLY file with one element of
float properties, and a structured-dtype reader built from the parsed header.  Nothing computes, so every comparison is bit
for bit; the model tensors hold random 32-bit patterns (NaNs, infinities, denormals, -0.0)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_ply.h")
ROWS = 64                                       # the kernels' rows per workgroup (checked against the module below)
ROW_COUNTS = (0, 1, ROWS - 1, ROWS, ROWS + 1, 3 * ROWS + 5)
CHUNK_ROWS = 80                                 # 197 rows: chunks of 80, 80 and 37
# (n, s, S): SH degree 3, isotropic, no seg colour, SH degree 0 (zero-size rest tensors)
LAYOUTS = {"degree3": (15, 3, 3), "isotropic": (15, 1, 3), "no_seg": (15, 3, 0), "degree0": (0, 3, 3)}
ATTRS = ("_xyz", "_features_dc_color", "_features_rest_color", "_opacity", "_scaling", "_rotation", "_features_dc_phase",
         "_features_rest_phase", "_features_dc_amp", "_features_rest_amp", "_features_seg_color")


# ---- the reference's statements ------------------------------------------------------------------------------------------

def names_ref(n, s, S, full):
    """construct_list_of_attributes for tensors [P,1,3], [P,n,3], [P,s], [P,4], [P,1,1], [P,n,1], [P,1,1], [P,n,1], [P,S]"""
    l = ["x", "y", "z", "nx", "ny", "nz"]
    l += ["f_dc_%d" % i for i in range(1 * 3)]
    l += ["f_rest_%d" % i for i in range(n * 3)]
    l.append("opacity")
    l += ["scale_%d" % i for i in range(s)]
    l += ["rot_%d" % i for i in range(4)]
    if full:
        l += ["phase_f_dc_%d" % i for i in range(1)]
        l += ["phase_f_rest_%d" % i for i in range(n)]
        l += ["amp_f_dc_%d" % i for i in range(1)]
        l += ["amp_f_rest_%d" % i for i in range(n)]
        l += ["f_seg_color_%d" % i for i in range(S)]
    return l


def header_ref(names, P):
    text = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % P
    for n in names:
        text += "property float %s\n" % n
    return (text + "end_header\n").encode("ascii")


def attributes_ref(m, full):
    """save_ply:343-363: the [P, K] float32 array the reference hands to plyfile"""
    flat = lambda t: t.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    xyz = m._xyz.detach().cpu().numpy()
    parts = [xyz, np.zeros_like(xyz), flat(m._features_dc_color), flat(m._features_rest_color), m._opacity.detach().cpu().numpy(),
             m._scaling.detach().cpu().numpy(), m._rotation.detach().cpu().numpy()]
    if full:
        parts += [flat(m._features_dc_phase), flat(m._features_rest_phase), flat(m._features_dc_amp), flat(m._features_rest_amp),
                  m._features_seg_color.detach().contiguous().cpu().numpy()]
    return np.concatenate(parts, axis=1)


def file_ref(m, layout, full):
    a = attributes_ref(m, full)
    assert a.dtype == np.float32
    return header_ref(names_ref(*layout, full), a.shape[0]) + a.astype("<f4").tobytes()


def read_struct(path):
    """the file's vertex element as a structured array, by the parsed header"""
    from gftorf_amd import ply
    data = open(path, "rb").read()
    P, names, offset = ply.parse_header(data)
    return np.frombuffer(data, dtype=[(n, "<f4") for n in names], count=P, offset=offset)


# ---- models --------------------------------------------------------------------------------------------------------------

class Model:
    max_sh_degree = 3
    active_sh_degree = 0


def shapes(P, n, s, S):
    return {"_xyz": (P, 3), "_features_dc_color": (P, 1, 3), "_features_rest_color": (P, n, 3), "_opacity": (P, 1), "_scaling": (P, s),
            "_rotation": (P, 4), "_features_dc_phase": (P, 1, 1), "_features_rest_phase": (P, n, 1), "_features_dc_amp": (P, 1, 1),
            "_features_rest_amp": (P, n, 1), "_features_seg_color": (P, S)}


def random_bits(rng, shape):
    a = rng.integers(0, 1 << 32, size=shape, dtype=np.uint32)
    flat = a.reshape(-1)
    special = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0xffc12345, 0x00000001, 0x807fffff, 0], np.uint32)
    flat[:min(len(flat), len(special))] = special[:len(flat)]
    return a.view(np.float32)


def make_model(P, layout, dev, seed=0, one_row_in=False):
    """every tensor random bit patterns; `one_row_in`: each is the view [1:] of a [P + 1, ...] buffer, 4-byte aligned only"""
    rng = np.random.default_rng(1000 * P + seed)
    m = Model()
    m.max_sh_degree = int(round((layout[0] + 1) ** 0.5)) - 1
    for attr, shape in shapes(P, *layout).items():
        if one_row_in:
            t = torch.from_numpy(random_bits(rng, (shape[0] + 1,) + shape[1:])).to(dev)[1:]
            assert t.is_contiguous()
        else:
            t = torch.from_numpy(random_bits(rng, shape)).to(dev)
        setattr(m, attr, t)
    return m


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


# ---- CPU-runnable checks -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_column_names(layout):
    from gftorf_amd import ply
    n, s, S = LAYOUTS[layout]
    sibr, full = ply.columns({"n": n, "s": s, "S": S}, full=False), ply.columns({"n": n, "s": s, "S": S}, full=True)
    assert sibr == names_ref(n, s, S, False) and full == names_ref(n, s, S, True)
    assert full[:len(sibr)] == sibr and len(full) == len(sibr) + 2 + 2 * n + S
    assert ply.columns({"n": n, "s": s, "S": S}) == sibr
    # from a model's tensors (on the host: only their shapes are read)
    m = Model()
    for attr, shape in shapes(5, n, s, S).items():
        setattr(m, attr, torch.zeros(shape))
    assert ply.columns(m, full=False) == sibr and ply.columns(m, full=True) == full
    if layout == "degree3":
        assert len(sibr) == 62 and len(full) == 97


def test_header_text_and_round_trip():
    from gftorf_amd import ply
    names = ["x", "y", "z", "opacity", "rot_0"]
    text = ply.header(names, 7)
    assert text == (b"ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
                    b"property float opacity\nproperty float rot_0\nend_header\n")
    assert ply.parse_header(text + b"\x00" * 140) == (7, names, len(text))
    for layout in LAYOUTS.values():
        for full in (False, True):
            want = names_ref(*layout, full)
            text = ply.header(ply.columns(dict(zip("nsS", layout)), full), 12345)
            assert text == header_ref(want, 12345)
            assert ply.parse_header(text) == (12345, want, len(text))


def test_header_parser_accepts_and_refuses():
    from gftorf_amd import ply
    text = (b"ply\nformat binary_little_endian 1.0\ncomment made by hand\nobj_info nothing\nelement vertex 3\nproperty float32 rot_1\n"
            b"comment between\nproperty float z\nproperty float extra\nproperty float x\nelement face 2\n"
            b"property list uchar int vertex_indices\nend_header\n")
    assert ply.parse_header(text + b"body") == (3, ["rot_1", "z", "extra", "x"], len(text))
    head = "ply\nformat %s 1.0\nelement %s 3\nproperty %s\nend_header\n"
    refused = {"ascii": head % ("ascii", "vertex", "float x"), "binary_big_endian": head % ("binary_big_endian", "vertex", "float x"),
               "double": head % ("binary_little_endian", "vertex", "double x"),
               "list": head % ("binary_little_endian", "vertex", "list uchar float x"),
               "face": head % ("binary_little_endian", "face", "float x")}
    for found, text in refused.items():
        with pytest.raises(NotImplementedError, match=found) as e:
            ply.parse_header(text.encode("ascii"))
        assert "GaussianModel.load_ply" in str(e.value)
    with pytest.raises(ValueError, match="not a PLY"):
        ply.parse_header(b"solid cube\n")
    assert ply.parse_header((head % ("binary_little_endian", "vertex", "float x")).encode("ascii"))[:2] == (3, ["x"])


def test_header_is_plain_c_and_every_symbol_is_exported(tmp_path, lib):
    from gftorf_amd import _lib, build, ply
    import gftorf_amd
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src)))
    assert names and all(n.startswith("gft_ply_") for n in names)
    assert set(names) == set(_lib.PLY_EXPORTS), names
    for n in names:
        assert hasattr(lib, n), n
    assert "k_ply.hip" in build.SOURCES and gftorf_amd.ply is ply and "struct" not in src
    prog = tmp_path / "ply_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_ply.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "ply_abi.o")])
    out = subprocess.check_output(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-include", "gftorf_ply.h",
                                   "-x", "c", "-"], input="PLY_WORDS_ARE GFT_PLY_ROWS GFT_PLY_MAX_SOURCES GFT_PLY_MAX_COLUMNS\n", text=True)
    consts = [int(x) for x in out.split("PLY_WORDS_ARE", 1)[1].split()]
    assert consts == [_lib.PLY_ROWS, _lib.PLY_MAX_SOURCES, _lib.PLY_MAX_COLUMNS]
    assert ply.ROWS_PER_GROUP == _lib.PLY_ROWS == ROWS and ply.MAX_COLUMNS == _lib.PLY_MAX_COLUMNS
    assert ROWS * _lib.PLY_MAX_COLUMNS * 4 + 2 * _lib.PLY_MAX_COLUMNS <= 64 * 1024          # the LDS tile and the column table
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16


def test_argument_errors_are_reported(lib):
    from gftorf_amd import _lib
    ints = lambda *v: (C.c_int32 * len(v))(*v)
    ptrs = lambda *v: (C.c_void_p * len(v))(*v)
    out = C.c_void_p(4096)
    src3, w3, c3 = ptrs(256, None, 512), ints(3, 3, 6), ints(1, 0, 3)

    def pack(P=10, count=3, sources=src3, widths=w3, channels=c3, K_full=12, K_sibr=6, out_full=out, out_sibr=out):
        return lib.gft_ply_pack(None, P, count, sources, widths, channels, K_full, K_sibr, out_full, out_sibr)

    def fails(rc, *words):
        assert rc != 0
        assert all(w in _lib.last_error() for w in words), _lib.last_error()

    assert pack(P=0) == 0                                               # nothing to launch: needs no device
    assert pack(P=0, sources=ptrs(None, None, None)) == 0               # ... and looks at no source
    fails(pack(out_full=None, out_sibr=None), "gft_ply_pack", "both outputs are NULL")
    fails(pack(K_full=13), "add up", "K_full=13")
    fails(pack(K_full=11), "add up", "K_full=11")
    fails(pack(P=-1), "P=-1")
    fails(pack(K_sibr=13), "K_sibr=13")
    fails(pack(K_sibr=0), "K_sibr=0")
    assert pack(P=0, K_sibr=0, out_sibr=None) == 0                      # K_sibr is read only with out_sibr
    fails(pack(channels=ints(1, 0, 4)), "block 2")                      # 6 floats are not [n, 4]
    fails(pack(widths=ints(3, -3, 12)), "block 1")
    fails(pack(sources=ptrs(256, None, None)), "source 2 is NULL")
    fails(pack(out_full=C.c_void_p(4100)), "16-byte")
    fails(pack(count=0), "column blocks")
    fails(pack(count=_lib.PLY_MAX_SOURCES + 1), "column blocks")
    fails(pack(K_full=_lib.PLY_MAX_COLUMNS + 1), "K_full")
    fails(pack(sources=None), "NULL")

    dst2, w2 = ptrs(256, 512), ints(3, 2)

    def unpack(rows=10, row0=0, K_file=7, chunk=out, count=2, dests=dst2, widths=w2, table=ints(0, 1, 2, 6, 5)):
        return lib.gft_ply_unpack(None, rows, row0, K_file, chunk, count, dests, widths, table)

    assert unpack(rows=0) == 0
    assert unpack(rows=0, dests=ptrs(None, None), chunk=None) == 0
    fails(unpack(table=ints(0, 1, 2, 7, 5)), "gft_ply_unpack", "table entry 3", "column 7", "K_file=7")
    fails(unpack(table=ints(0, -1, 2, 6, 5)), "table entry 1")
    fails(unpack(rows=-1), "rows=-1")
    fails(unpack(row0=-5), "row0=-5")
    fails(unpack(K_file=_lib.PLY_MAX_COLUMNS + 1), "K_file")
    fails(unpack(K_file=0), "K_file")
    fails(unpack(chunk=None), "chunk is NULL")
    fails(unpack(chunk=C.c_void_p(4104)), "16-byte")
    fails(unpack(dests=ptrs(256, None)), "destination 1 is NULL")
    fails(unpack(widths=ints(3, -2)), "tensor 1")
    fails(unpack(count=0), "destination tensors")
    assert lib.gft_abi_version() == 16


def test_cpu_tensors_and_bad_models_raise(tmp_path):
    from gftorf_amd import ply
    m = make_model(5, LAYOUTS["degree3"], "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ply.save_ply(m, str(tmp_path / "a.ply"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ply.submit(m, path_full=str(tmp_path / "b.ply"))
    with pytest.raises(ValueError, match="path_sibr, path_full or both"):
        ply.submit(m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ply.read_gaussians(str(tmp_path / "a.ply"), "cpu")
    assert not os.listdir(tmp_path)


# ---- GPU -----------------------------------------------------------------------------------------------------------------

def check_file(path, want, what):
    got = open(path, "rb").read()
    assert len(got) == len(want), (what, len(got), len(want))
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        bad = np.flatnonzero(a != b)
        raise AssertionError((what, "bytes differ", len(bad), bad[:8].tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_save_ply_and_save_pair_write_the_reference_bytes(layout, gpu, tmp_path):
    from gftorf_amd import ply
    lay = LAYOUTS[layout]
    for P in ROW_COUNTS:
        m = make_model(P, lay, gpu)
        want = {full: file_ref(m, lay, full) for full in (False, True)}
        sibr, full = str(tmp_path / ("sibr_%d.ply" % P)), str(tmp_path / ("full_%d.ply" % P))
        ply.save_ply(m, sibr, chunk_rows=CHUNK_ROWS)                                # sibr_only is the default, as in the reference
        ply.save_ply(m, full, sibr_only=False, chunk_rows=CHUNK_ROWS)
        check_file(sibr, want[False], (layout, P, "sibr"))
        check_file(full, want[True], (layout, P, "full"))
        pair = str(tmp_path / "deeper" / ("iteration_%d" % P))                      # the folders are made, as mkdir_p does
        ply.save_pair(m, os.path.join(pair, "point_cloud.ply"), os.path.join(pair, "point_cloud_full.ply"), chunk_rows=CHUNK_ROWS)
        check_file(os.path.join(pair, "point_cloud.ply"), open(sibr, "rb").read(), (layout, P, "pair sibr"))
        check_file(os.path.join(pair, "point_cloud_full.ply"), open(full, "rb").read(), (layout, P, "pair full"))
        # the default chunk (one chunk here) writes the same bytes
        ply.save_pair(m, sibr, full)
        check_file(sibr, want[False], (layout, P, "sibr, default chunk"))
        check_file(full, want[True], (layout, P, "full, default chunk"))
        # and the structured reader finds the reference's columns
        rec = read_struct(full)
        assert rec.dtype.names == tuple(names_ref(*lay, True)) and len(rec) == P
        if P:
            assert np.array_equal(bits(rec["f_rest_%d" % 16] if lay[0] else rec["f_dc_1"]),
                                  bits(m._features_rest_color[:, 1, 1] if lay[0] else m._features_dc_color[:, 0, 1]))
    assert 3 * ROWS + 5 > 2 * CHUNK_ROWS and (3 * ROWS + 5) % CHUNK_ROWS                 # three chunks, the last one ragged


@pytest.mark.gpu
def test_sources_with_4_byte_alignment_and_other_layouts(gpu, tmp_path):
    """every tensor a view one row into a larger buffer; then non-contiguous and float64 tensors, which are converted first"""
    from gftorf_amd import ply
    lay = LAYOUTS["degree3"]
    P = 3 * ROWS + 5
    m = make_model(P, lay, gpu, seed=3, one_row_in=True)
    assert any(getattr(m, a).data_ptr() % 16 for a in ATTRS)
    sibr, full = str(tmp_path / "sibr.ply"), str(tmp_path / "full.ply")
    ply.save_pair(m, sibr, full, chunk_rows=CHUNK_ROWS)
    check_file(sibr, file_ref(m, lay, False), "views sibr")
    check_file(full, file_ref(m, lay, True), "views full")
    m2 = make_model(P, lay, gpu, seed=4)
    want = file_ref(m2, lay, True)
    m2._features_rest_color = m2._features_rest_color.transpose(1, 2).contiguous().transpose(1, 2)     # same values, other strides
    m2._rotation = m2._rotation.t().contiguous().t()
    assert not m2._features_rest_color.is_contiguous() and not m2._rotation.is_contiguous()
    ply.save_ply(m2, full, sibr_only=False)
    check_file(full, want, "non-contiguous")
    m3 = make_model(ROWS + 1, lay, gpu, seed=5)
    m3._xyz = torch.rand((ROWS + 1, 3), device=gpu, dtype=torch.float64)
    ply.save_ply(m3, sibr)
    m3._xyz = m3._xyz.to(torch.float32)
    check_file(sibr, file_ref(m3, lay, False), "float64")


def write_shuffled(path, m, lay, seed):
    """the full file with its properties in another order and one more float column, written with numpy"""
    names = names_ref(*lay, True)
    a = attributes_ref(m, True)
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(names) + 1)
    cols = [names[i] if i < len(names) else "confidence" for i in order]
    body = np.concatenate([a, random_bits(rng, (a.shape[0], 1))], axis=1)[:, order]
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\ncomment shuffled\nelement vertex %d\n" % a.shape[0])
        f.write("".join("property float %s\n" % c for c in cols).encode("ascii") + b"end_header\n")
        f.write(np.ascontiguousarray(body, dtype="<f4").tobytes())
    return cols


def check_tensors(got, m, lay, P, what):
    from gftorf_amd import ply
    assert tuple(got) == ply.TENSORS
    for key, t in got.items():
        want = getattr(m, "_" + key)
        assert t.dtype == torch.float32 and t.is_contiguous() and t.device == want.device, (what, key)
        assert tuple(t.shape) == shapes(P, *lay)["_" + key], (what, key, tuple(t.shape))
        assert np.array_equal(bits(t), bits(want)), (what, key)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_read_gaussians_finds_the_properties_by_name(layout, gpu, tmp_path):
    from gftorf_amd import ply
    lay = LAYOUTS[layout]
    P = 3 * ROWS + 5
    m = make_model(P, lay, gpu, seed=7)
    path = str(tmp_path / "shuffled.ply")
    cols = write_shuffled(path, m, lay, seed=len(layout))
    assert cols != names_ref(*lay, True) + ["confidence"]
    check_tensors(ply.read_gaussians(path, gpu, max_sh_degree=m.max_sh_degree, chunk_rows=CHUNK_ROWS), m, lay, P, "chunks")
    check_tensors(ply.read_gaussians(path, gpu), m, lay, P, "one chunk, no degree")
    # the counts load_ply asserts
    with pytest.raises(ValueError, match="f_rest_"):
        ply.read_gaussians(path, gpu, max_sh_degree=m.max_sh_degree + 1)
    # a file that ends early
    data = open(path, "rb").read()
    open(path, "wb").write(data[:-40])
    with pytest.raises(ValueError, match="ends inside vertex"):
        ply.read_gaussians(path, gpu, chunk_rows=CHUNK_ROWS)


@pytest.mark.gpu
def test_save_then_load_round_trip(gpu, tmp_path):
    from gftorf_amd import ply
    lay = LAYOUTS["degree3"]
    path = str(tmp_path / "point_cloud_full.ply")
    for P in ROW_COUNTS:
        m = make_model(P, lay, gpu, seed=11)
        ply.save_ply(m, path, sibr_only=False, chunk_rows=CHUNK_ROWS)
        back = Model()
        back.max_sh_degree = 3
        ply.load_ply(back, path, chunk_rows=CHUNK_ROWS)
        assert back.active_sh_degree == back.max_sh_degree == 3
        for attr in ATTRS:
            t = getattr(back, attr)
            assert isinstance(t, torch.nn.Parameter) and t.requires_grad and t.is_leaf and t.device.type == "cuda", attr
        check_tensors({k: getattr(back, "_" + k) for k in ply.TENSORS}, m, lay, P, P)
    # a sibr file has no phase or amplitude: load_ply cannot read it, here as in the reference
    ply.save_ply(m, path)
    with pytest.raises(ValueError, match="phase_f_rest_|phase_f_dc_0"):
        ply.load_ply(back, path)
    # an isotropic degree-0 model through the same route
    lay0 = (0, 1, 3)
    m0 = make_model(ROWS + 1, lay0, gpu, seed=12)
    ply.save_ply(m0, path, sibr_only=False)
    back.max_sh_degree = 0
    ply.load_ply(back, path)
    check_tensors({k: getattr(back, "_" + k) for k in ply.TENSORS}, m0, lay0, ROWS + 1, "isotropic degree 0")
    back.max_sh_degree = 3
    with pytest.raises(ValueError, match="max_sh_degree = 3 needs 45"):
        ply.load_ply(back, path)


@pytest.mark.gpu
def test_a_job_is_a_snapshot_and_submit_does_not_synchronise(gpu, tmp_path):
    from gftorf_amd import ply
    lay = LAYOUTS["degree3"]
    P = 3 * ROWS + 5
    m = make_model(P, lay, gpu, seed=21)
    want = {full: file_ref(m, lay, full) for full in (False, True)}
    sibr, full = str(tmp_path / "point_cloud.ply"), str(tmp_path / "point_cloud_full.ply")
    ply.save_pair(m, sibr, full, chunk_rows=CHUNK_ROWS)       # warm-up: the library's load and the pinned buffers are not the question
    os.remove(sibr)
    os.remove(full)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        job = ply.submit(m, path_sibr=sibr, path_full=full)
        single = ply.submit(m, path_full=str(tmp_path / "single.ply"))
        for attr in ATTRS:                                    # the model moves on before anything is written
            getattr(m, attr).fill_(1.5)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert not os.path.exists(sibr) and not os.path.exists(full)
    del m
    job.finish(chunk_rows=CHUNK_ROWS)
    single.finish()
    check_file(sibr, want[False], "snapshot sibr")
    check_file(full, want[True], "snapshot full")
    check_file(str(tmp_path / "single.ply"), want[True], "snapshot single")
    # finish() twice writes once
    os.remove(sibr)
    open(full, "wb").write(b"mine")
    job.finish(chunk_rows=CHUNK_ROWS)
    assert not os.path.exists(sibr) and open(full, "rb").read() == b"mine"
