"""gftorf_amd.reproducible: same inputs, same state, same bits.  The switch, the deformation network's
route under it, the fixed-order backward of the flow renderer (csrc/k_features.hip), the grid-wide fixed-order sum
(csrc/k_detsum.hip, include/gftorf_detsum.h) against the one-workgroup comparator and against its numpy restatement
(tests/detsum_ref.py), and a whole F-ToRF flow iteration run twice, eagerly and from a captured graph."""
import copy
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import detsum_ref
import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    from gftorf_amd import reproducible as R
    keep = R.is_reproducible(), R._det_reduce
    yield
    R.set_reproducible(keep[0])
    R._det_reduce = keep[1]


# ---- the switch --------------------------------------------------------------------------------------------------------

def _fresh_module(monkeypatch, **env):
    """gftorf_amd/reproducible.py executed again under another environment (the package's own copy is not touched)."""
    for k in ("GFT_REPRODUCIBLE", "GFT_DET_REDUCE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    name = "reproducible_probe_%d" % len(sys.modules)
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "gftorf_amd", "reproducible.py"))
    mod = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, name, mod)
    spec.loader.exec_module(mod)
    return mod


def test_switch_is_off_by_default_and_follows_the_environment(monkeypatch):
    assert _fresh_module(monkeypatch).is_reproducible() is False
    assert _fresh_module(monkeypatch, GFT_REPRODUCIBLE="0").is_reproducible() is False
    assert _fresh_module(monkeypatch, GFT_REPRODUCIBLE="1").is_reproducible() is True
    assert _fresh_module(monkeypatch).det_reduce() == "grid"
    assert _fresh_module(monkeypatch, GFT_DET_REDUCE="serial").det_reduce() == "serial"


def test_switch_sets_nests_and_restores():
    import gftorf_amd
    from gftorf_amd import reproducible as R
    assert gftorf_amd.reproducible is R and gftorf_amd.set_reproducible is R.set_reproducible
    assert gftorf_amd.is_reproducible is R.is_reproducible
    R.set_reproducible(False)
    assert not R.is_reproducible()
    with gftorf_amd.reproducible():                      # the re-exported name is the context manager too
        assert R.is_reproducible()
        with R.reproducible(False):
            assert not R.is_reproducible()
            with R.reproducible(True):
                assert R.is_reproducible()
            assert not R.is_reproducible()
        assert R.is_reproducible()
    assert not R.is_reproducible()
    with pytest.raises(KeyError):
        with R.reproducible():
            with R.reproducible(False):
                raise KeyError("x")
    assert not R.is_reproducible()
    R.set_reproducible(True)
    with R.reproducible(False):
        assert not R.is_reproducible()
    assert R.is_reproducible()
    R.set_reproducible(0)
    assert R.is_reproducible() is False


class _FakeEvent:
    def __init__(self, answer):
        self.answer, self.asked = answer, 0

    def query(self):
        self.asked += 1
        return self.answer


def _route_cases():
    """(name, state) x3: a posted count that has arrived, one that has not, none."""
    pin = lambda: torch.tensor([2000], dtype=torch.int32)
    return [("arrived", {"fraction": None, "pending": (pin(), _FakeEvent(True), 8192), "pin": None}),
            ("under way", {"fraction": None, "pending": (pin(), _FakeEvent(False), 8192), "pin": None}),
            ("absent", {"fraction": None, "pending": None, "pin": None})]


def _count_peeks(monkeypatch):
    from gftorf_amd import deform
    calls = []
    real = deform._peek_fraction
    monkeypatch.setattr(deform, "_peek_fraction", lambda state: (calls.append(1), real(state))[1])
    return calls


def test_route_does_not_follow_the_posted_count_under_the_switch(monkeypatch):
    from gftorf_amd import deform
    from gftorf_amd import reproducible as R
    monkeypatch.setattr(deform, "device_row_count", "auto")
    monkeypatch.setattr(deform, "sparse_backward", True)
    monkeypatch.setattr(deform, "lazy_save", True)
    calls = _count_peeks(monkeypatch)
    for fraction, want in ((None, "compact"), (0.2, "recompute"), (0.5, "compact")):
        routes = []
        with R.reproducible():
            for _, state in _route_cases():
                state["fraction"] = fraction
                routes.append(deform._choose_route(True, 8192, False, state, 1024))
                ev = state["pending"][1] if state["pending"] else None
                assert ev is None or ev.asked == 0
                assert state["fraction"] == fraction
        assert routes == [want] * 3, (fraction, routes)
    assert calls == []
    with R.reproducible():
        # what does not ask the host stays as it is
        assert deform._choose_route(False, 8192, False, None, 0) == "none"
        assert deform._choose_route(True, 8191, False, None, 0) == "dense"
        assert deform._choose_route(True, 8192, True, _route_cases()[0][1], 0) == "rows"
        monkeypatch.setattr(deform, "device_row_count", True)
        assert deform._choose_route(True, 8192, False, _route_cases()[0][1], 0) == "rows"
        monkeypatch.setattr(deform, "device_row_count", False)
        assert deform._choose_route(True, 8192, True, None, 0) == "dense"
    assert calls == []


def test_route_table_is_unchanged_with_the_switch_off(monkeypatch):
    from gftorf_amd import api, deform
    from gftorf_amd import reproducible as R
    R.set_reproducible(False)
    monkeypatch.setattr(api, "_DETERMINISTIC", True)            # the rasterizer's mode alone: not this switch
    assert not R.is_reproducible()
    monkeypatch.setattr(deform, "device_row_count", "auto")
    monkeypatch.setattr(deform, "sparse_backward", True)
    monkeypatch.setattr(deform, "lazy_save", True)
    calls = _count_peeks(monkeypatch)
    got = {name: deform._choose_route(True, 8192, False, state, 1024) for name, state in _route_cases()}
    assert got == {"arrived": "rows", "under way": "count", "absent": "count"}
    assert len(calls) == 3
    big = deform._DEVICE_ROWS_MAX_BYTES + 1
    assert deform._choose_route(True, 8192, False, {"fraction": 0.2, "pending": None}, big) == "recompute"
    assert deform._choose_route(True, 8192, False, {"fraction": None, "pending": None}, lambda: big) == "compact"
    assert deform._choose_route(False, 8192, False, None, 0) == "none"
    assert deform._choose_route(True, 100, False, None, 0) == "dense"
    assert deform._choose_route(True, 8192, True, None, 0) == "rows"
    monkeypatch.setattr(deform, "device_row_count", "capture")
    assert deform._choose_route(True, 8192, True, None, 0) == "rows"
    assert deform._choose_route(True, 8192, False, {"fraction": 0.2, "pending": None}, 0) == "recompute"
    assert deform._choose_route(True, 8192, False, {"fraction": 0.3, "pending": None}, 0) == "compact"
    monkeypatch.setattr(deform, "device_row_count", False)
    assert deform._choose_route(True, 8192, True, None, 0) == "dense"
    monkeypatch.setattr(deform, "device_row_count", True)
    assert deform._choose_route(True, 8192, False, None, 0) == "rows"


def test_only_the_switch_reaches_the_flow_renderer_and_the_network():
    """GFT_BWD_DETERMINISTIC / api._DETERMINISTIC select the rasterizer's mode alone: no other module reads them."""
    for name in ("flow.py", "deform.py", "reproducible.py", "pair.py"):
        src = open(os.path.join(ROOT, "gftorf_amd", name)).read()
        code = "\n".join(l.split("#")[0] for l in src.splitlines())
        code = re.sub(r'""".*?"""', "", code, flags=re.S)
        assert "_DETERMINISTIC" not in code and "GFT_BWD_DETERMINISTIC" not in code, name
    api_src = open(os.path.join(ROOT, "gftorf_amd", "api.py")).read()
    assert '_DETERMINISTIC = _os.environ.get("GFT_BWD_DETERMINISTIC", "0") != "0"' in api_src


# ---- the order, restated ------------------------------------------------------------------------------------------------

def _hand_case():
    """Three Gaussians over four tiles (a 2 x 2 grid); lists: tile 0 = [0, 1], tile 1 = [1, 2], tile 2 = [2, 0, 1],
    tile 3 = [1]; one value per row; sums whose float32 result depends on the order."""
    lists = [[0, 1], [1, 2], [2, 0, 1], [1]]
    ranges, point_list, start = [], [], 0
    for l in lists:
        ranges.append((start, start + len(l)))
        point_list += l
        start += len(l) + 1                                # (a gap: lists need not be adjacent)
        point_list.append(99)
    rows = np.zeros((len(point_list), 4, 8), np.float32)
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    # Gaussian 1 stands in all four tiles: 2^24, 1, -2^24, 1 in tile order
    rows[1, 0, 0], rows[3, 2, 0], rows[8, 1, 0], rows[10, 3, 0] = big, one, -big, one
    # Gaussian 0: tiles 0 and 2; inside tile 2 its four quadrant rows are 2^24, 1, 1, -2^24
    rows[0, 0, 0] = np.float32(0.5)
    rows[7, :, 0] = [big, one, one, -big]
    # Gaussian 2: tiles 1 and 2, the second sum exactly zero (skipped)
    rows[4, 1, 0] = np.float32(3.0)
    rows[6, 0, 0], rows[6, 3, 0] = np.float32(1.5), np.float32(-1.5)
    quad_max = np.array([[2, 1, 0, 0], [1, 2, 1, 1], [3, 3, 3, 3], [0, 0, 0, 1]], np.uint32)
    return np.array(ranges, np.uint32), quad_max, np.array(point_list, np.uint32), rows


def test_detsum_ref_sees_an_order():
    ranges, quad_max, point_list, rows = _hand_case()
    acc = detsum_ref.detsum(ranges, quad_max, point_list, rows, 3, 1)
    f = np.float32
    # Gaussian 1, tiles 0..3: ((2^24 + 1) - 2^24) + 1 = 1 in float32 (2^24 + 1 rounds to 2^24)
    assert acc[1, 0] == f(1.0)
    # Gaussian 0: 0.5 + (((2^24 + 1) + 1) - 2^24) = 0.5 + 0
    assert acc[0, 0] == f(0.5)
    assert acc[2, 0] == f(3.0)
    other = detsum_ref.detsum(ranges, quad_max, point_list, rows, 3, 1, tile_order=[0, 2, 1, 3])
    assert other[1, 0] == f(2.0) and other[1, 0] != acc[1, 0]           # (2^24 - 2^24) + 1 + 1
    assert other[0, 0] == acc[0, 0] and other[2, 0] == acc[2, 0]
    quads = detsum_ref.detsum(ranges, quad_max, point_list, rows, 3, 1, quad_order=(0, 3, 1, 2))
    assert quads[0, 0] == f(2.5) and quads[0, 0] != acc[0, 0]           # 0.5 + ((2^24 - 2^24) + 1 + 1)
    # entries past what a tile's quadrants walked are not visited
    quad_max[3] = 0
    assert detsum_ref.detsum(ranges, quad_max, point_list, rows, 3, 1)[1, 0] == f(0.0)       # (2^24 + 1) - 2^24


@pytest.mark.parametrize("header,exports", [("gftorf_features.h", "FEATURE_EXPORTS"), ("gftorf_detsum.h", "DETSUM_EXPORTS")])
def test_headers_are_plain_c_and_every_symbol_is_exported(header, exports, tmp_path, lib):
    from gftorf_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src)) - {"gft_config"})
    assert set(names) == set(getattr(_lib, exports)), names
    assert {"gft_feature_partials_bytes", "gft_render_features_backward_det"} <= set(_lib.FEATURE_EXPORTS)
    assert not set(names) & set(_lib.EXPORTS)
    for n in names:
        assert hasattr(lib, n), n
    prog = tmp_path / "abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "%s"' % header, 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "abi.o")])
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16
    assert "k_detsum.hip" in __import__("gftorf_amd.build", fromlist=["SOURCES"]).SOURCES


def test_argument_errors_and_sizes_of_the_new_entry_points(lib):
    from gftorf_amd import _lib
    cfg = _lib.Config()
    cfg.P, cfg.W, cfg.H = 10, 72, 40
    x = C.c_void_p(16)                        # never dereferenced: the calls fail before any launch
    T = 5 * 3
    assert lib.gft_feature_partials_bytes(1000, 72, 40) * 2 == lib.gft_det_partials_bytes(1000, 72, 40)
    assert lib.gft_feature_partials_bytes(1000, 72, 40) == (T * 2048 + 1000) * 128
    assert lib.gft_feature_partials_bytes(0, 72, 40) == 0
    assert lib.gft_detsum_index_bytes(10, 1000) >= 4 * (10 + 1 + 1000)
    assert lib.gft_detsum_index_bytes(0, 0) == 0
    assert lib.gft_render_features_backward_det(None, None, x, x, x, 64, 3, x, x, x, x) != 0
    assert "config is NULL" in _lib.last_error()
    assert lib.gft_render_features_backward_det(None, C.byref(cfg), x, x, x, 64, 4, x, x, x, x) != 0
    assert "C must be 3 or 6" in _lib.last_error()
    assert lib.gft_render_features_backward_det(None, C.byref(cfg), x, x, x, 64, 3, x, x, None, x) != 0
    assert "NULL argument" in _lib.last_error()
    assert lib.gft_render_features_backward_det(None, C.byref(cfg), x, x, x, 64, 3, x, C.c_void_p(18), x, x) != 0
    assert "4-byte aligned" in _lib.last_error()
    cfg.P = 0
    assert lib.gft_render_features_backward_det(None, C.byref(cfg), x, x, None, 0, 3, None, None, None, None) == 0    # P == 0: at once
    assert lib.gft_backward_det(None, None, None, 0, None) != 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------

# small_scene arguments: Gaussians of 2 x 2 tiles and more, opacities low enough for long walks
SCENES = {
    "batch": dict(P=800, W=64, H=48, seed=5, opacity=0.05, scale_lo=0.15, scale_hi=0.4),          # lists past one staged batch (64)
    "segment": dict(P=3000, W=72, H=40, seed=7, opacity=0.01, scale_lo=0.15, scale_hi=0.5),      # ... past a backward segment (256)
    "ragged": dict(P=1500, W=72, H=40, seed=9, opacity=0.03, scale_lo=0.1, scale_hi=0.4),
}
MIN_WALK = {"batch": 64, "segment": 256, "ragged": 64}


def _geometry(scene, dev, culled=0):
    g = scene["gaussians"]
    geo = {k: torch.tensor(g[k], dtype=torch.float32, device=dev) for k in ("means3D", "opacities", "scales", "rotations")}
    if culled:
        geo["means3D"][::culled, 0] += 1000.0           # far outside the frustum: radius 0
    return geo


def _views(buffers):
    """ranges [T, 2], quad_max [T, 4], point_list of the last forward's scratch, as numpy."""
    from gftorf_amd import _lib
    P, W, H, cap = (buffers[k] for k in ("P", "W", "H", "cap"))
    L = _lib.get_layout(P, W, H, cap)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    img, binning = buffers["img"].cpu().numpy().view(np.uint8), buffers["binning"].cpu().numpy().view(np.uint8)
    u32 = lambda buf, off, n: buf[off:off + 4 * n].view(np.uint32).copy()
    slots = int(_lib.load().gft_det_partials_bytes(cap, W, H)) // 256
    return (u32(img, L.img_ranges, 2 * T).reshape(T, 2), u32(img, L.img_tile_max, 4 * T).reshape(T, 4),
            u32(binning, L.bin_point_list, slots))


def _rel(ref, got):
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _flow_grads(settings, geo, fa, fb, ga, gb):
    from gftorf_amd import flow
    a = fa.clone().requires_grad_()
    b = fb.clone().requires_grad_() if fb is not None else None
    ia, ib = flow.render_flows(settings, geo["means3D"], geo["opacities"], geo["scales"], geo["rotations"], a, b)
    loss = (ia * ga).sum() + ((ib * gb).sum() if ib is not None else 0.0)
    loss.backward()
    return a.grad, (b.grad if b is not None else None)


def _rasterizer_colour_grad(settings, geo, f, g):
    from gftorf_amd import GaussianRasterizer
    P = geo["means3D"].shape[0]
    leaf = f.clone().requires_grad_()
    o = GaussianRasterizer(raster_settings=settings)(
        means3D=geo["means3D"], means2D=torch.zeros((P, 3), device=f.device), opacities=geo["opacities"], colors_precomp=leaf,
        scales=geo["scales"], rotations=geo["rotations"])
    (o[0] * g).sum().backward()
    return leaf.grad.detach(), o[10]


def _flow_setup(name, gpu, culled=0):
    args = SCENES[name]
    scene = Hh.small_scene(**args)
    W, H, P = args["W"], args["H"], args["P"]
    geo = _geometry(scene, gpu, culled)
    settings = Hh.gpu_settings(scene, gpu, bg=torch.zeros((7, H, W), device=gpu))
    gen = torch.Generator().manual_seed(P)
    fa, fb = ((0.05 * torch.randn((P, 3), generator=gen)).to(gpu) for _ in range(2))
    ga, gb = (torch.randn((3, H, W), generator=gen).to(gpu) for _ in range(2))
    return scene, geo, settings, fa, fb, ga, gb


@pytest.mark.gpu
@pytest.mark.parametrize("binning", [0, 1])
@pytest.mark.parametrize("channels,name", [(3, "batch"), (6, "segment"), (6, "ragged"), (3, "segment")])
def test_flow_backward_in_a_fixed_order(channels, name, binning, gpu, monkeypatch):
    from gftorf_amd import _lib, api
    from gftorf_amd import reproducible as R
    lib = _lib.load()
    monkeypatch.setattr(api, "_TILE_HINTS", False)
    monkeypatch.setattr(api, "keep_last_buffers", True)
    scene, geo, settings, fa, fb, ga, gb = _flow_setup(name, gpu, culled=7 if name == "ragged" else 0)
    if channels == 3:
        fb = gb = None
    lib.gft_set_binning_mode(binning)
    lib.gft_set_render_mode(0)
    try:
        R.set_reproducible(False)
        atomics = _flow_grads(settings, geo, fa, fb, ga, gb)
        _, quad_max, _ = _views(api.last_call_buffers)
        ref_a, radii = _rasterizer_colour_grad(settings, geo, fa, ga)
        ref_b = _rasterizer_colour_grad(settings, geo, fb, gb)[0] if fb is not None else None
        with R.reproducible():
            R._det_reduce = "grid"
            grid = [_flow_grads(settings, geo, fa, fb, ga, gb) for _ in range(3)]
            R._det_reduce = "serial"
            serial = _flow_grads(settings, geo, fa, fb, ga, gb)
    finally:
        lib.gft_set_binning_mode(-1)
        lib.gft_set_render_mode(-1)
    torch.cuda.synchronize()
    assert int(quad_max.max()) > MIN_WALK[name], int(quad_max.max())             # the scene is what it is meant to be
    assert int(radii.max()) >= 16                                                   # Gaussians over 2 x 2 tiles and more
    for k, (ref, old) in enumerate(((ref_a, atomics[0]), (ref_b, atomics[1]))):
        if ref is None:
            assert grid[0][k] is None
            continue
        print("\n%s C=%d binning %d flow %d: fixed order vs atomics %.3g, vs the rasterizer %.3g"
              % (name, channels, binning, k, _rel(old, grid[0][k]), _rel(ref, grid[0][k])))
        assert float(ref.abs().max()) > 0
        assert _rel(old, grid[0][k]) <= 1e-5 and _rel(ref, grid[0][k]) <= 1e-5
        assert torch.equal(grid[0][k], grid[1][k]) and torch.equal(grid[0][k], grid[2][k])
        assert torch.equal(grid[0][k], serial[k])
        if name == "ragged":
            assert int((radii == 0).sum()) > 0
            assert float(grid[0][k][radii == 0].abs().max()) == 0.0                 # rows no pixel touched read as zero


def _frame_for_c_calls(name, gpu, monkeypatch, binning=1):
    """One drawn frame and what the C entry points need to walk it."""
    from gftorf_amd import _lib, api, flow
    lib = _lib.load()
    monkeypatch.setattr(api, "_TILE_HINTS", False)
    monkeypatch.setattr(api, "keep_last_buffers", True)
    scene, geo, settings, fa, fb, ga, gb = _flow_setup(name, gpu)
    lib.gft_set_binning_mode(binning)
    lib.gft_set_render_mode(0)
    try:
        with torch.no_grad():
            flow.render_flows(settings, geo["means3D"], geo["opacities"], geo["scales"], geo["rotations"], fa, None)
    finally:
        lib.gft_set_binning_mode(-1)
        lib.gft_set_render_mode(-1)
    buf = dict(api.last_call_buffers)
    P, W, H, cap = buf["P"], buf["W"], buf["H"], buf["cap"]
    cfg = api._make_config(settings, P, 0, 0, H, W, 0.0, 0.0, (0, 0, 0), False)
    return lib, buf, cfg, torch.cat((ga, gb)).contiguous()


def _features_det(lib, buf, cfg, g, channels, grid, out=None):
    from gftorf_amd import _lib
    dev = g.device
    P, W, H, cap = buf["P"], buf["W"], buf["H"], buf["cap"]
    partials = torch.full((lib.gft_feature_partials_bytes(cap, W, H) // 4,), float("nan"), device=dev)     # any contents
    index = torch.full((lib.gft_detsum_index_bytes(P, cap) // 4,), -1, device=dev, dtype=torch.int32) if grid else None
    out = torch.empty((P, channels), device=dev) if out is None else out
    with _lib.on_device(dev):
        _lib.check(lib.gft_render_features_backward_det(
            _lib.raw_stream(dev), C.byref(cfg), buf["geom"].data_ptr(), buf["img"].data_ptr(), buf["binning"].data_ptr(), cap,
            channels, g.data_ptr(), index.data_ptr() if grid else None, partials.data_ptr(), out.data_ptr()))
    torch.cuda.synchronize()
    return out, partials


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [3, 6])
def test_feature_rows_summed_by_the_restated_order(channels, gpu, monkeypatch):
    lib, buf, cfg, g = _frame_for_c_calls("ragged", gpu, monkeypatch)
    out, partials = _features_det(lib, buf, cfg, g[:channels].contiguous(), channels, True)
    out_s, partials_s = _features_det(lib, buf, cfg, g[:channels].contiguous(), channels, False)
    assert torch.equal(out, out_s) and torch.equal(partials, partials_s)
    ranges, quad_max, point_list = _views(buf)
    rows = partials.cpu().numpy().reshape(-1, 4, 8)
    assert np.isfinite(rows).all() and float(np.abs(rows[:, :, channels:]).max()) == 0.0
    want = detsum_ref.detsum(ranges, quad_max, point_list, rows, buf["P"], channels)
    assert float(np.abs(want).max()) > 0
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [True, False])
def test_a_frame_past_its_binning_capacity_leaves_the_gradient_untouched(grid, gpu, monkeypatch):
    from gftorf_amd import _lib
    lib, buf, cfg, g = _frame_for_c_calls("batch", gpu, monkeypatch)
    L = _lib.get_layout(buf["P"], buf["W"], buf["H"], buf["cap"])
    ctrl_total = buf["img"].view(torch.uint8)[L.img_ctrl:L.img_ctrl + 4]
    sentinel = torch.full((buf["P"], 3), 7.25, device=gpu)
    good, _ = _features_det(lib, buf, cfg, g[:3].contiguous(), 3, grid, out=sentinel.clone())
    assert float((good - 7.25).abs().max()) > 0
    # the instance count the forward left says the frame did not fit (what a forward without a host read leaves on overflow)
    ctrl_total.copy_(torch.tensor([0xff, 0xff, 0xff, 0xff], dtype=torch.uint8, device=gpu))
    out, _ = _features_det(lib, buf, cfg, g[:3].contiguous(), 3, grid, out=sentinel.clone())
    assert torch.equal(out, sentinel)


@pytest.mark.gpu
def test_flow_backward_without_gaussians(gpu):
    from gftorf_amd import flow
    from gftorf_amd import reproducible as R
    scene = Hh.small_scene(P=600, W=64, H=48, seed=3)
    settings = Hh.gpu_settings(scene, gpu, bg=torch.zeros((7, 48, 64), device=gpu))
    z = lambda *s: torch.zeros(s, device=gpu)
    a, b = z(0, 3).requires_grad_(), z(0, 3).requires_grad_()
    with R.reproducible():
        ia, ib = flow.render_flows(settings, z(0, 3), z(0, 1), z(0, 3), z(0, 4), a, b)
        (ia.sum() + ib.sum()).backward()
    torch.cuda.synchronize()
    assert a.grad.shape == (0, 3) and b.grad.shape == (0, 3)
    assert float(ia.detach().abs().max()) == 0.0 and float(ib.detach().abs().max()) == 0.0


@pytest.mark.gpu
def test_captured_flow_backward_equals_the_eager_one(gpu, monkeypatch):
    from gftorf_amd import api
    from gftorf_amd import reproducible as R
    monkeypatch.setattr(api, "_TILE_HINTS", False)
    scene, geo, settings, fa, fb, ga, gb = _flow_setup("segment", gpu)
    a, b = fa.clone().requires_grad_(), fb.clone().requires_grad_()

    def step():
        from gftorf_amd import flow
        a.grad = b.grad = None
        ia, ib = flow.render_flows(settings, geo["means3D"], geo["opacities"], geo["scales"], geo["rotations"], a, b)
        ((ia * ga).sum() + (ib * gb).sum()).backward()
        return a.grad, b.grad

    with R.reproducible():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                eager = [t.clone() for t in step()]
        torch.cuda.current_stream().wait_stream(side)
        a.grad = b.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
    # replayed with the switch off: the graph keeps the mode it was captured under
    assert not R.is_reproducible()
    for _ in range(3):
        for t in out:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


# ---- the rasterizer's mode ---------------------------------------------------------------------------------------------

def _pair_grads(scene, dev):
    from gftorf_amd import GaussianRasterizerPair
    g = scene["gaussians"]
    leaf = {k: torch.tensor(v, dtype=torch.float32, device=dev, requires_grad=True) for k, v in g.items() if v is not None}
    P = leaf["means3D"].shape[0]
    means2D = torch.zeros((P, 3), device=dev, requires_grad=True)
    sa = Hh.gpu_settings(scene, dev, use_view_dependent_phase=False, depth_range=100.0)
    sb = Hh.gpu_settings(scene, dev)
    out_a, out_b = GaussianRasterizerPair(sa, sb)(
        means3D=leaf["means3D"], means2D=means2D, opacities=leaf["opacities"], shs=leaf["shs"], shs_p=leaf["shs_p"],
        scales=leaf["scales"], rotations=leaf["rotations"], phase_offset=(0.0, scene["phase_offset"]), dc_offset=(0.0, 0.0))
    gr = scene["grads"]
    w = lambda k: torch.tensor(gr[k], device=dev)
    loss = (out_a[0] * w("color")).sum() + (out_b[1] * w("phasor")).sum() + (out_b[2] * w("depth")).sum() + (out_b[0] * w("color")).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().cpu().numpy() for k, v in leaf.items() if v.grad is not None}
    grads["means2D"] = means2D.grad.detach().cpu().numpy()
    return grads


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_rasterizer_grid_wide_sum_equals_the_serial_comparator(name, gpu, monkeypatch):
    from gftorf_amd import api
    from gftorf_amd import reproducible as R
    monkeypatch.setattr(api, "_TILE_HINTS", False)
    scene = Hh.small_scene(**SCENES[name])
    run = (lambda: _pair_grads(scene, gpu)) if name == "ragged" else (lambda: Hh.run_gpu(scene, gpu, optimize_offsets=True)[1])
    got = {}
    with R.reproducible():
        for mode in ("grid", "serial", "grid"):
            R._det_reduce = mode
            got.setdefault(mode, []).append(run())
    R._det_reduce = "serial"
    monkeypatch.setattr(api, "_DETERMINISTIC", True)            # the private switch selects the same mode
    private = run()
    keys = sorted(k for k, v in got["serial"][0].items() if v is not None)
    assert {"means3D", "means2D", "opacities", "shs", "shs_p", "scales", "rotations"} <= set(keys)
    for k in keys:
        assert float(np.abs(got["serial"][0][k]).max()) > 0, k
        assert np.array_equal(got["grid"][0][k], got["serial"][0][k]), (name, k)
        assert np.array_equal(got["grid"][0][k], got["grid"][1][k]), (name, k)
        # (the two offset gradients are summed in another order when a kept gradient set is rewritten by rows: only the
        # reproducible mode rules that out, api.prepare_backward)
        assert k in ("phase_offset", "dc_offset") or np.array_equal(private[k], got["serial"][0][k]), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["batch", "segment"])
def test_rasterizer_rows_summed_by_the_restated_order(name, gpu, monkeypatch):
    from gftorf_amd import api
    from gftorf_amd import reproducible as R
    monkeypatch.setattr(api, "_TILE_HINTS", False)
    monkeypatch.setattr(api, "keep_last_buffers", True)
    kept = []
    monkeypatch.setattr(api, "_det_keep", kept)
    scene = Hh.small_scene(**SCENES[name])
    P = SCENES[name]["P"]
    colours = (0.3 * np.random.default_rng(P).standard_normal((P, 3))).astype(np.float32)
    with R.reproducible():
        _, grads, _ = Hh.run_gpu(scene, gpu, inputs=dict(shs=None, colors_precomp=colours))
    assert len(kept) == 1
    det, cap = kept[0]
    assert cap == api.last_call_buffers["cap"]
    ranges, quad_max, point_list = _views(api.last_call_buffers)
    assert int(quad_max.max()) > MIN_WALK[name]
    rows = det.cpu().numpy().reshape(-1, 4, 16)
    want = detsum_ref.detsum(ranges, quad_max, point_list, rows, P, 15)
    # the accumulator row's first three values are dL/dcolour as it is returned
    assert float(np.abs(want[:, :3]).max()) > 0
    assert np.array_equal(grads["colors_precomp"], want[:, :3])


# ---- the network -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_network_route_and_gradients_do_not_follow_host_timing(gpu, monkeypatch):
    from gftorf_amd import deform, reference_network
    from gftorf_amd import reproducible as R
    monkeypatch.setattr(deform, "device_row_count", "auto")
    monkeypatch.setattr(deform, "sparse_backward", True)
    monkeypatch.setattr(deform, "lazy_save", True)
    n = 8192
    torch.manual_seed(5)
    net0 = reference_network()
    net0.initialize_weights(types.SimpleNamespace(isotropic_gaussians=False, xavier_init_dxyz=True))
    gen = torch.Generator().manual_seed(9)
    x, t = (torch.rand((n, 3), generator=gen) - 0.5).to(gpu), torch.rand((n, 1), generator=gen).to(gpu)
    rows = (torch.rand((n,), generator=gen) < 0.3)
    assert 0.27 < float(rows.float().mean()) < 0.33
    g_xyz = (torch.randn((n, 3), generator=gen) * rows[:, None]).to(gpu)
    g_sh = (torch.randn((n, 16, 3), generator=gen) * rows[:, None, None]).to(gpu)

    def run(sync):
        net = copy.deepcopy(net0).to(gpu)
        routes = []
        with R.reproducible():
            for k in range(2):
                for p in net.parameters():
                    p.grad = None
                d_xyz, _, d_sh, _ = net(x, t)
                ((d_xyz * g_xyz).sum() + (d_sh * g_sh).sum()).backward()
                routes.append(deform.last_backward_route)
                if sync and k == 0:
                    torch.cuda.synchronize()
        torch.cuda.synchronize()
        stats = deform.backward_stats()
        return routes, [p.grad.clone() for p in net.parameters() if p.grad is not None], stats

    routes_a, grads_a, stats_a = run(True)
    routes_b, grads_b, stats_b = run(False)
    assert routes_a == routes_b and routes_a[1] in ("compact", "recompute", "dense")
    assert stats_a["points"] == n and stats_a == stats_b
    assert len(grads_a) == len(grads_b) > 0
    for a, b in zip(grads_a, grads_b):
        assert float(a.abs().max()) > 0
        assert torch.equal(a, b)


# ---- a whole F-ToRF flow iteration -------------------------------------------------------------------------------------

class _Iteration:
    """query at three times, assemble_parameters, the pair, render_flow_pair, flow_loss, an image term, the regularisers,
    backward, FusedAdam.step(max_grad_norm=1.0) on both optimizers -- on one copy of the state."""
    P, W, H = 3000, 72, 40

    def __init__(self, dev, par, net, capturable):
        from gftorf_amd import DeformQuery, FusedAdam
        self.dev = dev
        self.par = {k: v.clone().requires_grad_() for k, v in par.items()}
        self.net = copy.deepcopy(net).to(dev)
        lrs = dict(xyz=1.6e-4, f_dc_color=2.5e-3, f_rest_color=1.25e-4, phase_f_dc=2.5e-3, phase_f_rest=1.25e-4, amp_f_dc=2.5e-3,
                   amp_f_rest=1.25e-4, opacity=0.05, scaling=5e-3, rotation=1e-3)
        self.opt = FusedAdam([{"params": [self.par[k]], "lr": lrs[k], "name": k} for k in lrs], lr=0.0, eps=1e-15,
                             capturable=capturable)
        self.opt_net = FusedAdam([{"params": list(self.net.parameters()), "lr": 8e-4, "name": "deform"}], lr=0.0, eps=1e-15,
                                 capturable=capturable)
        self.scene = scene = Hh.small_scene(P=self.P, W=self.W, H=self.H, seed=23, opacity=0.05, scale_lo=0.1, scale_hi=0.3)
        gen = torch.Generator().manual_seed(29)
        self.mask = (torch.rand((self.P,), generator=gen) < 0.95).to(dev).contiguous()
        self.query = DeformQuery(self.mask)
        assert 3 * self.query.n >= 8192                   # the batch of the three times is one the sparse routes take
        W, H = self.W, self.H
        self.bg = torch.zeros((7, H, W), device=dev)
        self.gt_tof = torch.randn((7, H, W), generator=gen).to(dev)
        self.gt_colour = torch.rand((3, H, W), generator=gen).to(dev)
        flows = [(2.0 * torch.randn((2, H, W), generator=gen)).to(dev) for _ in range(2)]
        cam = scene["cam"]
        t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
        fx = W / (2 * cam["tanfovx"])
        K = t([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]])
        self.cam = types.SimpleNamespace(
            tof_image_height=H, tof_image_width=W, FoVx_tof=2 * math.atan(cam["tanfovx"]), FoVy_tof=2 * math.atan(cam["tanfovy"]),
            world_view_transform_tof=t(cam["viewmatrix"]), full_proj_transform_tof=t(cam["projmatrix"]),
            camera_center_tof=t(cam["campos"]), znear=cam["znear"], zfar=cam["zfar"], depth_range=float(scene["depth_range"]),
            K=K, K_tof=K, world_view_transform=t(cam["viewmatrix"]), forward_flow=flows[0], backward_flow=flows[1])
        self.settings = (Hh.gpu_settings(scene, dev, bg=self.bg, use_view_dependent_phase=False, depth_range=100.0),
                         Hh.gpu_settings(scene, dev, bg=self.bg))
        self.ssp = torch.zeros((self.P, 3), device=dev, requires_grad=True)

    def step(self):
        from gftorf_amd import GaussianRasterizerPair, assemble_parameters, flow, ftorf_schedule, reg
        from gftorf_amd import loss as gft_loss
        par, mask = self.par, self.mask
        times, combine, names = ftorf_schedule(8, 30, forward_flow=True, backward_flow=True)
        assert names == ("d_xyz", "flow_next", "flow_prev") and len(times) == 3
        (d_xyz, flow_next, flow_prev), d_sh = self.query.plan(self.net, par["xyz"], 1.0, times, combine, sh_of=0)
        self.ssp.grad = None
        m3, m2, op, sc, ro, shs, shp = assemble_parameters(
            par["xyz"], self.ssp, par["opacity"], par["scaling"], par["rotation"], par["f_dc_color"], par["f_rest_color"],
            par["phase_f_dc"], par["phase_f_rest"], par["amp_f_dc"], par["amp_f_rest"], mask, d_xyz, 0.0, d_sh, 0.0)
        out_c, out_t = GaussianRasterizerPair(*self.settings)(
            means3D=m3, means2D=m2, opacities=op, shs=shs, shs_p=shp, scales=sc, rotations=ro,
            phase_offset=(0.0, self.scene["phase_offset"]), dc_offset=(0.0, 0.0))
        normalize = lambda q: torch.nn.functional.normalize(q, dim=-1)
        with torch.no_grad():
            pc = types.SimpleNamespace(
                get_xyz=par["xyz"].detach(), get_opacity=torch.sigmoid(par["opacity"]), get_scaling=torch.exp(par["scaling"]),
                _rotation=par["rotation"].detach(), get_rotation=normalize(par["rotation"]), rotation_activation=normalize,
                get_motion_mask=mask, active_sh_degree=3, use_view_dependent_phase=True)
        imf, imb = flow.render_flow_pair(self.cam, pc, d_xyz.detach(), 0.0, flow_next, flow_prev, self.bg)
        lf, lb = flow.flow_loss(out_t[2].detach(), self.cam, imf, imb)
        loss = 0.01 * (lf + lb)
        loss = loss + gft_loss.image_term(out_t[1], self.gt_tof, "l2", 0.8, 0.2)
        loss = loss + gft_loss.image_term(out_c[0], self.gt_colour, "l1", 0.8, 0.2)
        loss = loss + reg.regularizers(d_xyz=d_xyz, w_mlp=0.01, opacity=op, motion_mask=mask, w_oe=0.01)
        loss.backward()
        with torch.no_grad():
            self.opt.step(max_grad_norm=1.0)
            self.opt.zero_grad(set_to_none=True)
            self.opt_net.step(max_grad_norm=1.0)
            self.opt_net.zero_grad(set_to_none=True)
        return loss.detach()

    def tensors(self):
        """every parameter and both Adam moments of both optimizers"""
        out = []
        for opt in (self.opt, self.opt_net):
            for group in opt.param_groups:
                for p in group["params"]:
                    st = opt.state.get(p) or {}              # (the network's unused heads never take a step)
                    out += [p.detach()] + [st[k] for k in ("exp_avg", "exp_avg_sq") if k in st]
        return out


def _initial_state(dev):
    P = _Iteration.P
    scene = Hh.small_scene(P=P, W=_Iteration.W, H=_Iteration.H, seed=23, opacity=0.05, scale_lo=0.1, scale_hi=0.3)
    g = scene["gaussians"]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    inv_sig = lambda x: np.log(x / (1 - x))
    par = dict(
        xyz=t(g["means3D"]), f_dc_color=t(g["shs"][:, :1, :]), f_rest_color=t(g["shs"][:, 1:, :] * 0.1),
        phase_f_dc=t(g["shs_p"][:, :1, :1]), phase_f_rest=torch.zeros((P, 15, 1), device=dev),
        amp_f_dc=t(g["shs_p"][:, :1, 1:]), amp_f_rest=torch.zeros((P, 15, 1), device=dev),
        opacity=t(inv_sig(np.full((P, 1), 0.05))), scaling=t(np.log(g["scales"])), rotation=t(g["rotations"]))
    from gftorf_amd import reference_network
    torch.manual_seed(31)
    net = reference_network()
    net.initialize_weights(types.SimpleNamespace(isotropic_gaussians=False, xavier_init_dxyz=True))
    return par, net


def _assert_same(a, b, what):
    ta, tb = a.tensors(), b.tensors()
    assert len(ta) == len(tb) > 3 * 10 + len(list(a.net.parameters()))
    for k, (x, y) in enumerate(zip(ta, tb)):
        assert torch.equal(x, y), (what, k)


@pytest.mark.gpu
def test_a_whole_flow_iteration_twice_gives_the_same_bits(gpu, monkeypatch):
    from gftorf_amd import deform
    from gftorf_amd import reproducible as R
    monkeypatch.setattr(deform, "device_row_count", "auto")
    par, net = _initial_state(gpu)
    first = [t.clone() for t in par.values()]
    with R.reproducible():
        a, b = _Iteration(gpu, par, net, False), _Iteration(gpu, par, net, False)
        for k in range(3):
            la = a.step()
            torch.cuda.synchronize()                     # (host timing differs between the copies on purpose)
            lb = b.step()
            assert torch.equal(la, lb)
            _assert_same(a, b, "step %d" % k)
    moved = [float((p.detach() - q).abs().max()) for p, q in zip(a.par.values(), first)]
    assert all(m > 0 for m in moved), moved                # every parameter group took its steps
    assert all(bool(torch.isfinite(p).all()) for p in a.net.parameters())
    assert any(k in a.opt_net.state[p] for p in a.net.parameters() if p in a.opt_net.state for k in ("exp_avg",))


@pytest.mark.gpu
def test_a_captured_flow_iteration_replayed_on_two_copies_gives_the_same_bits(gpu, monkeypatch):
    from gftorf_amd import deform
    from gftorf_amd import reproducible as R
    monkeypatch.setattr(deform, "device_row_count", "auto")
    par, net = _initial_state(gpu)
    copies = []
    with R.reproducible():
        for _ in range(2):
            it = _Iteration(gpu, par, net, True)
            for _ in range(2):
                it.step()                                # the optimizers' state is created outside the graph
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                it.static_loss = it.step()
            it.graph = graph
            copies.append(it)
    a, b = copies
    _assert_same(a, b, "before the replays")
    for k in range(3):
        for it in copies:
            it.opt.refresh_lr()
            it.opt_net.refresh_lr()
            it.graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a.static_loss, b.static_loss)
        _assert_same(a, b, "replay %d" % k)
