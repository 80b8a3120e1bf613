"""Host-side checks that need no GPU: the C-ABI library loads and exports every symbol the
header declares, the header is valid C and its struct layouts equal the ctypes mirrors,
and the operator API fails loudly instead of falling back when it cannot run on a HIP device."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_rast.h")


@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


HEADERS = [HEADER, os.path.join(ROOT, "include", "gftorf_assemble.h"), os.path.join(ROOT, "include", "gftorf_knn.h"),
           os.path.join(ROOT, "include", "gftorf_optim.h"), os.path.join(ROOT, "include", "gftorf_deform.h"),
           os.path.join(ROOT, "include", "gftorf_densify.h"), os.path.join(ROOT, "include", "gftorf_loss.h")]


def declared_functions():
    names = set()
    for h in HEADERS:
        src = open(h).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names |= set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src))
    return sorted(names)


def test_library_exports_every_declared_symbol(lib):
    from gftorf_amd import _lib
    names = declared_functions()
    assert set(names) == set(_lib.EXPORTS), (names, _lib.EXPORTS)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.gft_abi_version() == _lib.ABI_VERSION


def test_header_is_plain_c_and_matches_ctypes(tmp_path, lib):
    from gftorf_amd import _lib
    prog = tmp_path / "abi.c"
    fields = {"gft_config": [f[0] for f in _lib.Config._fields_],
              "gft_forward_io": _lib.FORWARD_FIELDS, "gft_backward_io": _lib.BACKWARD_FIELDS,
              "gft_layout": _lib.LAYOUT_FIELDS,
              "gft_profile": _lib.PROFILE_FIELDS + ["forward_calls", "backward_calls"],
              "gft_assemble_io": _lib.ASSEMBLE_FIELDS, "gft_assemble_bwd_io": _lib.ASSEMBLE_BWD_FIELDS,
              "gft_deform_params": _lib.DEFORM_FIELDS, "gft_deform_grads": _lib.DEFORM_FIELDS,
              "gft_forward_hints": [f[0] for f in _lib.ForwardHints._fields_],
              "gft_forward_report": [f[0] for f in _lib.ForwardReport._fields_],
              "gft_adam_tensor": [f[0] for f in _lib.AdamTensor._fields_]}
    body = ['#include <stdio.h>', '#include <stddef.h>', '#include "gftorf_rast.h"', '#include "gftorf_assemble.h"',
            '#include "gftorf_deform.h"', '#include "gftorf_optim.h"', 'int main(void){']
    for s, fl in fields.items():
        body.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f in fl:
            body.append('printf("%s.%s %%zu\\n", offsetof(%s,%s));' % (s, f, s, f))
    body.append('printf("ACC %d\\n", GFT_ACC_STRIDE); return 0;}')
    prog.write_text("\n".join(body))
    exe = tmp_path / "abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    mirrors = {"gft_config": _lib.Config, "gft_forward_io": _lib.ForwardIO, "gft_backward_io": _lib.BackwardIO,
               "gft_layout": _lib.Layout, "gft_profile": _lib.Profile,
               "gft_assemble_io": _lib.AssembleIO, "gft_assemble_bwd_io": _lib.AssembleBwdIO,
               "gft_deform_params": _lib.DeformParams, "gft_deform_grads": _lib.DeformParams,
               "gft_forward_hints": _lib.ForwardHints, "gft_forward_report": _lib.ForwardReport, "gft_adam_tensor": _lib.AdamTensor}
    for s, cls in mirrors.items():
        assert int(out[s]) == C.sizeof(cls), s
        for f in fields[s]:
            assert int(out["%s.%s" % (s, f)]) == getattr(cls, f).offset, (s, f)
    assert int(out["ACC"]) == _lib.ACC_STRIDE


def test_size_queries_and_layout_need_no_gpu(lib):
    from gftorf_amd import _lib
    assert lib.gft_geom_bytes(0) > 0
    g1, g2 = lib.gft_geom_bytes(1000), lib.gft_geom_bytes(2000)
    assert 81 * 1000 <= g1 < g2      # 32+32+4+4+8+1 bytes per Gaussian
    assert lib.gft_image_bytes(640, 480) >= 640 * 480 * 16 + 1200 * 12
    L = _lib.get_layout(1000, 640, 480, 5000)
    offs = [getattr(L, n) for n in _lib.LAYOUT_FIELDS]
    # every region is 256-B aligned, except those that directly follow the 64-B ctrl block
    # (the ctrl words, the tile counters, the tile cuts and the supertile tables are contiguous: one clear)
    assert all(o % 256 == 0 for n, o in zip(_lib.LAYOUT_FIELDS, offs) if n not in ("img_tile_cnt", "img_tile_cut", "img_super_tab"))
    assert L.img_tile_cnt == L.img_ctrl + 64 + 128 and L.img_tile_cut == L.img_tile_cnt + 4 * 1200      # ctrl words + ticket counters
    assert L.img_super_tab == L.img_tile_cut + 4 * 1200
    assert L.geom_rec_b >= 32 * 1000 and L.bin_point_list >= 8 * 5000 and L.bin_total >= 12 * 5000 + 1200 * 2048 * 4
    assert lib.gft_binning_bytes(0, 640, 480) >= 0
    # capacity <-> bytes (what the pybind-level backward reads back from the buffer it is handed)
    for cap in (0, 64, 5056, 3_638_528):
        assert lib.gft_binning_capacity(lib.gft_binning_bytes(cap, 640, 480), 640, 480) == cap


def test_argument_errors_are_reported(lib):
    from gftorf_amd import _lib
    c = _lib.Config()
    c.P, c.W, c.H, c.D, c.M = 4, 64, 64, 5, 16
    io = _lib.ForwardIO()
    R = C.c_int64(0)
    assert lib.gft_forward_preprocess(None, C.byref(c), C.byref(io), C.byref(R), None) != 0
    assert "sh_degree" in _lib.last_error()
    c.D, c.M = 3, 4
    assert lib.gft_forward_preprocess(None, C.byref(c), C.byref(io), C.byref(R), None) != 0
    assert "coefficients" in _lib.last_error()
    c.M = 16
    assert lib.gft_forward_preprocess(None, C.byref(c), C.byref(io), C.byref(R), None) != 0
    assert "NULL" in _lib.last_error()


def test_operator_api_surface_and_loud_failure():
    import diff_gaussian_rasterization_w_tof as d
    from gftorf_amd import GaussianRasterizationSettings, GaussianRasterizer
    assert d.GaussianRasterizer is GaussianRasterizer
    # 18 fields, same names/defaults as the reference NamedTuple (__init__.py:22-40)
    assert GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug", "near_n", "far_n", "depth_range",
        "use_view_dependent_phase", "optimize_phase_offset", "optimize_dc_offset")
    assert GaussianRasterizationSettings._field_defaults == dict(
        near_n=0.01, far_n=100.0, depth_range=100.0, use_view_dependent_phase=False,
        optimize_phase_offset=False, optimize_dc_offset=False)
    eye = torch.eye(4)
    s = GaussianRasterizationSettings(image_height=32, image_width=32, tanfovx=0.5, tanfovy=0.5,
                                      bg=torch.zeros(7, 32, 32), scale_modifier=1.0, viewmatrix=eye,
                                      projmatrix=eye, sh_degree=0, campos=torch.zeros(3), prefiltered=False, debug=False)
    r = GaussianRasterizer(raster_settings=s)
    m = torch.rand(8, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=m[:, :1], scales=m, rotations=torch.rand(8, 4))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
        r(means3D=m, means2D=m, opacities=m[:, :1], shs=torch.rand(8, 1, 3), scales=m)
    # CPU tensors: no silent fallback
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(means3D=m, means2D=m, opacities=m[:, :1], shs=torch.rand(8, 1, 3), scales=m, rotations=torch.rand(8, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        r.markVisible(m)


def test_missing_library_is_an_error(tmp_path, monkeypatch):
    from gftorf_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "gftorf_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "gft_oracle" not in txt, f


def test_bench_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "HIP device" in (r.stderr + r.stdout)


def test_deform_size_queries_and_argument_errors(lib):
    from gftorf_amd import _lib
    # 2 x 96*256 (layer 0, encoding rows of layer 5) + 7*65536 + 16384 forward, 16384 + 7*65536 backward, 2112 biases
    # + three bf16 planes of both weight streams + two fp16 planes of both (999424 weights, 2 x 2 bytes each; the backward
    # stream's since round 6) + the range flag's four words + per segment the inverse of the power of two its fp16 planes
    # hold the weights times (18, padded to 20) + the largest |weight| of every 256 weights, from which the pack chooses it
    assert lib.gft_deform_packed_bytes() == (1001536 + 999424 * 3 // 2 + 999424 + 4 + 20 + 999424 // 256) * 4
    assert lib.gft_deform_inputs(10, 10) == 84 and lib.gft_deform_inputs(10, 6) == 76      # reference config / class default
    assert lib.gft_deform_inputs(10, 16) == 96 == _lib.DEFORM_MAX_INPUTS and lib.gft_deform_inputs(10, 17) == -1
    assert lib.gft_deform_inputs(-1, 6) == -1
    assert lib.gft_deform_saved_bytes(0) == 0 and lib.gft_deform_scratch_bytes(0) == 0
    # per point (padded to 192): 96 encoding + 8*256 activations + 8*8 words of ReLU sign bits
    assert lib.gft_deform_saved_bytes(1) == 192 * (96 + 2048 + 64) * 4
    assert lib.gft_deform_saved_bytes(193) == 384 * (96 + 2048 + 64) * 4
    assert lib.gft_deform_scratch_bytes(1000) > 1024 * (2048 + 64) * 4
    assert lib.gft_deform_pack(None, 10, 10, None, None) != 0
    assert "NULL" in _lib.last_error()
    assert lib.gft_deform_pack(None, 10, 17, C.byref(_lib.DeformParams()), C.c_void_p(64)) != 0
    assert "encoded inputs" in _lib.last_error()
    assert lib.gft_deform_forward(None, 10, 10, -1, None, None, 1, None, None, None, None) != 0
    assert lib.gft_deform_forward(None, 10, 10, 0, None, None, 1, None, None, None, None) == 0      # nothing to do
    assert lib.gft_deform_forward(None, 10, 10, 5, None, None, 1, None, None, None, None) != 0
    assert lib.gft_deform_forward(None, 11, 16, 0, None, None, 1, None, None, None, None) != 0      # 102 inputs
    assert lib.gft_deform_backward(None, 10, 10, 5, None, None, None, None, None, None) != 0


def test_deform_rows_launches_hold_the_splits_of_every_row_count(lib):
    """gft_deform_backward_rows sizes its weight-gradient grids and partial sums on the host, for the capacity, while the
    plan kernel picks the splits of the row count it finds on the device.  gft_deform_dw_splits is not monotone, so the
    capacity's own count is no bound: gft_deform_rows_splits_capacity has to hold the splits of EVERY row count up to
    the capacity, and the work buffer has to hold that many partial sums."""
    import numpy as np
    PAD = 192
    classes = np.arange(1, 400_000 // PAD + 2, dtype=np.int64)               # padded sizes 192 .. 400 128
    dw = np.array([lib.gft_deform_dw_splits(int(c) * PAD) for c in classes], dtype=np.int64)
    cap = np.array([lib.gft_deform_rows_splits_capacity(int(c) * PAD) for c in classes], dtype=np.int64)
    assert lib.gft_deform_dw_splits(0) == 0 and lib.gft_deform_rows_splits_capacity(0) == 0
    # a count belongs to its padding class: the first and the last size of a class give the class's answer
    assert [lib.gft_deform_dw_splits(int(c) * PAD - PAD + 1) for c in classes[:300]] == dw[:300].tolist()
    assert [lib.gft_deform_rows_splits_capacity(int(c) * PAD - PAD + 1) for c in classes[:300]] == cap[:300].tolist()
    assert dw.min() >= 1 and dw.max() == 73
    # every k <= n in steps of the padding: the largest count up to a capacity is within what that capacity launches
    most = np.maximum.accumulate(dw)
    assert (most <= cap).all(), classes[most > cap][:5] * PAD
    assert (np.diff(cap) >= 0).all()
    # the work buffer grows with n and holds a partial sum per split of the capacity beside everything else
    # (a split's partial sums: dW of layer 0 [256,96], layers 1..7 [256,256], encoding rows of layer 5 [256,96], heads
    # [64,256], biases [8,256] + [64])
    part_bytes = (2 * 256 * 96 + 7 * 256 * 256 + 64 * 256 + 8 * 256 + 64) * 4
    r256 = lambda b: (b + 255) // 256 * 256
    sizes = sorted({int(c) * PAD + d for c in classes[::7].tolist() + [42, 43, 64, 65, 104, 105] for d in (-1, 0, 1)} | {1, 8195, 12345})
    work = [lib.gft_deform_rows_work_bytes(n) for n in sizes]
    assert all(a <= b for a, b in zip(work, work[1:]))
    for n, w in zip(sizes, work):
        n_pad = (n + PAD - 1) // PAD * PAD
        # the dense scratch without its partial sums = dz, dzh, row maxima, range flag
        dense_rest = lib.gft_deform_scratch_bytes(n) - lib.gft_deform_dw_splits(n) * part_bytes
        assert dense_rest == (n_pad * (8 * 256 + 64) + n_pad * 8 + 4) * 4
        rest = (2 * 256 + r256(lib.gft_rows_rank_scratch_bytes(n)) + r256(n) + 2 * r256(4 * n) + 3 * r256(12 * n) + 2 * r256(192 * n)
                + r256(lib.gft_deform_saved_bytes(n)) + dense_rest)
        assert w - rest >= lib.gft_deform_rows_splits_capacity(n) * part_bytes, n
    # the guard on this test: dw_splits is NOT monotone, so "the capacity's own count" fails the bound above -- at the
    # smallest size the Python module sends down this path, at the test sizes and at the config-3 point count
    for n, k_pads in ((8195, (6912, 7680)), (12345, (10752, 11520, 12288)), (20000, (16896, 17664, 18432)), (40000, (18432,)),
                      (100000, (23232,))):
        own = lib.gft_deform_dw_splits(n)
        for k in k_pads:
            assert k <= n and lib.gft_deform_dw_splits(k) > own, (n, k)
            assert lib.gft_deform_dw_splits(k) <= lib.gft_deform_rows_splits_capacity(n)
    assert [lib.gft_deform_dw_splits(n) for n in (8195, 12345, 20000, 40000, 100000)] == [26, 39, 63, 70, 72]
    assert int((dw[:40128 // PAD] > 70).sum()) == 27 and int((dw[:100032 // PAD] > 72).sum()) == 68
