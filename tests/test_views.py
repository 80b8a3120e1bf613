"""gftorf_amd.views: the training views on the device (include/gftorf_views.h, csrc/k_views.hip).

The layout and the draw order are checked on the host against restatements written here; everything a draw moves is checked
bit for bit against torch indexing of the inputs (a draw is a copy, and ``byte / 255.0`` one correctly rounded division, so
there is no tolerance anywhere in this file).  Shapes are the smallest that reach every path of the kernels: planes whose
byte size is no multiple of 16, a group of more 16-byte chunks than one workgroup moves (``_lib.VIEWS_CHUNKS``), a uint8 image
of more pixels than one workgroup converts with a ragged last tile, 1, 3 and 4 channels.
"""
import os
import random
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_views.h")
SEED = 20261020
V = 5
ORDER = (3, 1, 4, 1, 0, 2, 3)           # length 7 over 5 views, with repeats


# ---- CPU-runnable checks ------------------------------------------------------------------------------------------------

def test_header_declares_the_exports():
    from gftorf_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"\b(gft_views_\w+)\s*\(", src)
    assert sorted(names) == sorted(_lib.VIEWS_EXPORTS), names
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    defines = {k: int(v) for k, v in re.findall(r"#define (GFT_VIEWS_\w+) (\d+)", src)}
    assert defines["GFT_VIEWS_MAX_GROUPS"] == _lib.VIEWS_MAX_GROUPS and defines["GFT_VIEWS_ALIGN"] == _lib.VIEWS_ALIGN == 16
    assert defines["GFT_VIEWS_HEADER_BYTES"] == _lib.VIEWS_HEADER_BYTES and defines["GFT_VIEWS_CHUNKS"] == _lib.VIEWS_CHUNKS
    assert defines["GFT_VIEWS_INDEX_WORD"] == _lib.VIEWS_INDEX_WORD and defines["GFT_VIEWS_CURSOR_WORD"] == _lib.VIEWS_CURSOR_WORD
    assert [defines["GFT_VIEWS_" + k.upper()] for k in _lib.VIEWS_KINDS] == [0, 1]


def layout_restated(F, J, groups):
    """The layout in this file's own terms: the record (F floats, J ints) first in a slab and behind the 16-byte header in
    the current buffer, then the groups in order; everything padded to 16 bytes; a u8 group is bytes in the slab and floats
    in the current buffer"""
    up = lambda n: -(-n // 16) * 16
    record = up(4 * (F + J))
    slab, cur = record, 16 + record
    slab_off, cur_off = [], []
    for kind, c, h, w in groups:
        slab_off.append(slab)
        cur_off.append(cur)
        slab += up(c * h * w * (1 if kind == "u8" else 4))
        cur += up(c * h * w * 4)
    return slab, cur, tuple(slab_off), tuple(cur_off), 0, 16


def test_layout_against_the_restatement():
    from gftorf_amd import views
    groups = [("f32", 3, 7, 5), ("u8", 3, 7, 5), ("f32", 4, 9, 6)]          # 420 B, 105 B, 864 B
    L = views.layout(109, 9, groups)
    assert tuple(L) == layout_restated(109, 9, groups)
    assert tuple(L) == (1888, 2224, (480, 912, 1024), (496, 928, 1360), 0, 16)
    for F, J, gs in ((0, 0, groups[:1]), (5, 0, []), (0, 3, groups[1:]), (1, 1, groups * 2 + groups[:2]),
                     (96, 10, [("u8", 4, 1, 1), ("u8", 1, 33, 35), ("f32", 1, 1, 1)])):
        L = views.layout(F, J, gs)
        assert tuple(L) == layout_restated(F, J, gs), (F, J, gs)
        for off in L.slab_offsets + L.current_offsets + (L.slab_record, L.current_record, L.slab_bytes, L.current_bytes):
            assert off % 16 == 0


def test_layout_refuses_what_cannot_be_laid_out():
    import ctypes as C
    from gftorf_amd import _lib, views
    ok = ("f32", 3, 7, 5)
    assert views.layout(0, 0, []) is None                                   # no group and no record
    for bad in (("f32", 0, 7, 5), ("f32", 3, -1, 5), ("f32", 3, 7, 0), ("u8", 0, 7, 5)):
        assert views.layout(4, 0, [ok, bad]) is None, bad                   # a non-positive dimension
    assert views.layout(4, 0, [ok] * 9) is None                             # more than 8 groups
    assert views.layout(4, 0, [ok] * 8) is not None
    assert views.layout(4, 0, [("u8", 5, 7, 5)]) is None                    # a u8 group of more than 4 channels
    assert views.layout(4, 0, [("u8", 4, 7, 5)]) is not None
    # the C function itself, as a caller without the Python layer meets it
    lib = _lib.load()
    ints = lambda *v: (C.c_int32 * len(v))(*v)
    call = lambda F, J, n, k, c, h, w: lib.gft_views_layout(F, J, n, k, c, h, w, None, None, None)
    assert call(0, 0, 0, None, None, None, None) == 0
    assert call(-1, 0, 0, None, None, None, None) == 0 and call(0, -1, 0, None, None, None, None) == 0
    assert call(1, 0, 9, ints(*[0] * 9), ints(*[1] * 9), ints(*[1] * 9), ints(*[1] * 9)) == 0
    assert call(1, 0, 1, ints(1), ints(5), ints(2), ints(2)) == 0
    assert call(1, 0, 1, ints(2), ints(1), ints(2), ints(2)) == 0            # an unknown kind
    assert call(1, 0, 1, ints(0), ints(1), ints(0), ints(2)) == 0
    assert call(1, 0, 1, ints(1), ints(4), ints(2), ints(2)) == 16 + 16


def reference_draws(frame_ids, start_id, rng, n):
    """train.py:155-163 as it stands there, over stand-in cameras"""
    train_cameras = [types.SimpleNamespace(frame_id=f, uid=v) for v, f in enumerate(frame_ids)]
    viewpoint_stack = None
    drawn = []
    for _iteration in range(n):
        if not viewpoint_stack:
            viewpoint_stack = train_cameras.copy()
        viewpoint_cam = viewpoint_stack.pop(rng.randint(0, len(viewpoint_stack) - 1))
        while viewpoint_cam.frame_id < start_id:
            if not viewpoint_stack:
                viewpoint_stack = train_cameras.copy()
            viewpoint_cam = viewpoint_stack.pop(rng.randint(0, len(viewpoint_stack) - 1))
        drawn.append(viewpoint_cam.uid)
    return drawn


@pytest.mark.parametrize("shuffled", (False, True))
@pytest.mark.parametrize("start_id", (0, 3))
@pytest.mark.parametrize("views_n", (1, 5, 12))
@pytest.mark.parametrize("seed", (0, 1, 2))
def test_draw_order_is_the_reference_loop(seed, views_n, start_id, shuffled):
    from gftorf_amd.views import DrawOrder
    frame_ids = list(range(views_n))
    if shuffled:
        random.Random(100 + seed).shuffle(frame_ids)
    if max(frame_ids) < start_id:
        with pytest.raises(ValueError, match="start_id"):
            DrawOrder(frame_ids, start_id, random.Random(seed))
        return
    n = 3 * views_n + 2
    rng = random.Random(seed)
    want = reference_draws(frame_ids, start_id, rng, n)
    assert all(frame_ids[v] >= start_id for v in want)
    for pieces in ((n,), (1, views_n, n - views_n - 1), (1,) * n):
        mine = random.Random(seed)
        order = DrawOrder(frame_ids, start_id, mine)
        got = [v for k in pieces for v in order.next(k)]
        assert got == want, pieces
        assert mine.getstate() == rng.getstate(), pieces


def test_draw_order_refuses_a_loop_that_never_ends():
    from gftorf_amd.views import DrawOrder
    with pytest.raises(ValueError, match="start_id"):
        DrawOrder([0, 1, 2], start_id=3)
    with pytest.raises(ValueError, match="start_id"):
        DrawOrder([], start_id=0)


def test_no_cpu_path():
    from gftorf_amd import views
    with pytest.raises(RuntimeError, match="no CPU path"):
        views.ViewStore("cpu", record=np.zeros((2, 3), np.float32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        views.select_plane(torch.zeros((4, 3, 2)), 1)
    with pytest.raises(NotImplementedError, match="requires grad"):
        views.select_plane(torch.zeros((4, 3, 2)), torch.zeros((1,), requires_grad=True))


# ---- the inputs of the GPU tests: made once, never changed ----------------------------------------------------------------

def _inputs():
    rng = np.random.default_rng(SEED)
    f = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    d = dict(color=f(V, 3, 7, 5), phasor=f(V, 3, 9, 6), quad=f(V, 4, 9, 6), fflow=list(f(V, 2, 7, 5)), bflow=list(f(V, 2, 7, 5)),
             big=f(V, 3, 33, 65))                       # big: 1609 chunks of 16 bytes, one workgroup moves 1024
    d["fflow"][4] = None
    d["bflow"][0] = None
    d["record"] = f(V, 13)
    d["ints"] = rng.integers(-1000, 1000, (V, 3)).astype(np.int32)
    return d


INPUTS = _inputs()
GROUPS = ("color", "phasor", "quad", "fflow", "bflow", "big")


def _store(gpu):
    from gftorf_amd import _lib, views
    assert 3 * 33 * 65 * 4 > 16 * _lib.VIEWS_CHUNKS
    return views.ViewStore(gpu, record=INPUTS["record"], ints=INPUTS["ints"], **{k: INPUTS[k] for k in GROUPS})


def _expected(v):
    """every accessor's contents with view v current, as host tensors"""
    want = {}
    for k in GROUPS:
        row = INPUTS[k][v]
        shape = next(r for r in INPUTS[k] if r is not None).shape
        want[k] = torch.zeros(shape) if row is None else torch.from_numpy(row)
        want["has_" + k] = torch.tensor([0 if row is None else 1], dtype=torch.int32)
    want["record"] = torch.from_numpy(INPUTS["record"][v])
    want["ints"] = torch.from_numpy(INPUTS["ints"][v])
    want["index"] = torch.tensor([v], dtype=torch.int32)
    return want


def _accessors(store):
    acc = dict(store.current)
    acc.update({"has_" + k: store.has(k) for k in GROUPS})
    acc.update(record=store.record, ints=store.ints, index=store.index)
    return acc


def _check(got, v, what):
    want = _expected(v)
    assert set(got) == set(want)
    for k in want:
        g = got[k].cpu()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k)
        # bits, not values: -0.0 and NaN payloads would count (int32 view of the float tensors)
        same = torch.equal(g.view(torch.int32), want[k].view(torch.int32)) if g.dtype == torch.float32 else torch.equal(g, want[k])
        assert same, (what, k)


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_draw_by_value(gpu):
    store = _store(gpu)
    acc = _accessors(store)
    where = {k: t.data_ptr() for k, t in acc.items()}
    assert all(p % 16 == 0 for k, p in where.items() if k in GROUPS or k == "record")
    assert store.has("fflow").dtype == torch.int32 and tuple(store.index.shape) == (1,)
    for step, v in enumerate((0, 1, 2, 3, 4, 3, 4, 0, 1, 0, 2, 2)):      # 3 -> 4 and 1 -> 0: onto a view that lacks a flow
        store.draw(v)
        _check(acc, v, "draw %d (view %d)" % (step, v))
        assert int(store.cursor_used.item()) == -1
        assert {k: t.data_ptr() for k, t in _accessors(store).items()} == where
    for bad in (-1, V, 1 << 40):
        with pytest.raises(ValueError, match="not in"):
            store.draw(bad)
    _check(acc, 2, "after the refused draws")
    with pytest.raises(RuntimeError, match="schedule"):
        store.draw()


@pytest.mark.gpu
def test_u8_group_is_the_division_by_255(gpu):
    from gftorf_amd import views
    H, W = 33, 35                                       # 1155 pixels: two workgroups, a last tile of 131 = 4 * 32 + 3
    px = np.arange(H * W)
    images = np.stack([np.stack([(px * (2 * c + 1) * (2 * v + 1) + 7 * c + v) % 256 for c in range(3)], -1).reshape(H, W, 3)
                       for v in range(2)]).astype(np.uint8)
    for v in range(2):
        for c in range(3):
            assert len(np.unique(images[v, :, :, c])) == 256
    rng = np.random.default_rng(SEED + 1)
    rgba = rng.integers(0, 256, (2, 7, 5, 4)).astype(np.uint8)
    mask = [rng.integers(0, 256, (5, 3, 1)).astype(np.uint8), None]
    store = views.ViewStore(gpu, image=views.u8(images), rgba=views.u8(rgba), mask=views.u8(mask))
    assert store.current["image"].shape == (3, H, W) and store.current["image"].dtype == torch.float32
    host = lambda a: (torch.from_numpy(a) / 255.0).permute(2, 0, 1).clamp(0, 1)
    for v in (0, 1, 0):
        store.draw(v)
        assert torch.equal(store.current["image"].cpu(), host(images[v])), v
        assert torch.equal(store.current["rgba"].cpu(), host(rgba[v])), v
        assert torch.equal(store.current["mask"].cpu(), host(mask[0]) if v == 0 else torch.zeros((1, 5, 3))), v
        assert int(store.has("mask").item()) == (1 if v == 0 else 0) and int(store.has("image").item()) == 1
    with pytest.raises(ValueError, match="at most 4"):
        views.ViewStore(gpu, wide=views.u8(np.zeros((2, 3, 3, 5), np.uint8)))


@pytest.mark.gpu
def test_schedule(gpu):
    store = _store(gpu)
    acc = _accessors(store)
    assert store.schedule(ORDER) is store and store.cursor() == 0
    n = len(ORDER)
    for k in range(2 * n + 1):
        store.draw()
        _check(acc, ORDER[k % n], "scheduled draw %d" % k)
        assert int(store.cursor_used.item()) == k and store.cursor() == k + 1
    store.draw(2)                                       # a draw by value leaves the schedule alone
    assert store.cursor() == 2 * n + 1 and int(store.cursor_used.item()) == -1
    store.schedule(ORDER[::-1])
    assert store.cursor() == 0
    store.draw()
    _check(acc, ORDER[-1], "after the reset")
    for bad in ((), (0, V), (-1, 0), (0, 1 << 33)):
        with pytest.raises(ValueError):
            store.schedule(bad)
    with pytest.raises(TypeError):
        store.schedule((0.5, 1.0))
    assert store.cursor() == 1                          # the refused orders changed nothing
    store.draw()
    _check(acc, ORDER[-2], "after the refused orders")


def _capture(region, warm_ups=1, after_warm_up=None):
    """The recipe of tests/test_gpu_graph.py: warm-up on a side stream, then one capture"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warm_ups):
            region()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if after_warm_up is not None:
        after_warm_up()
        torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = region()
    return graph, static


@pytest.mark.gpu
def test_captured_draw_follows_the_schedule(gpu):
    store = _store(gpu)
    store.schedule(ORDER)

    def region():
        store.draw()
        return dict({k: t.clone() for k, t in _accessors(store).items()}, cursor_used=store.cursor_used.clone())

    graph, static = _capture(region, after_warm_up=lambda: store.schedule(ORDER))
    assert store.cursor() == 0                          # the capture drew nothing
    n = len(ORDER)
    for k in range(2 * n + 1):
        graph.replay()
        torch.cuda.synchronize()
        got = dict(static)
        assert int(got.pop("cursor_used").item()) == k and store.cursor() == k + 1
        _check(got, ORDER[k % n], "replay %d" % k)


@pytest.mark.gpu
def test_captured_draw_feeds_the_rasterizer(gpu):
    """draw() and a rasterizer forward whose settings refer to the store's ToF camera, in one graph: every replay is the
    eager forward with the drawn camera's own tensors"""
    import helpers as Hh
    from gftorf_amd import api, synth, views, GaussianRasterizer
    P, W, H = 300, 32, 24
    poses = [synth.look_at_w2c(0.05, -0.02, 0.0, (0.05, 0.0, 0.1)), synth.look_at_w2c(-0.08, 0.03, 0.01, (-0.1, 0.02, 0.15)),
             synth.look_at_w2c(0.12, 0.04, -0.02, (0.02, -0.06, 0.05))]
    scenes = [Hh.small_scene(P=P, W=W, H=H, seed=47, w2c=p) for p in poses]
    g = scenes[0]["gaussians"]
    leaf = {k: torch.tensor(v, dtype=torch.float32, device=gpu) for k, v in g.items() if v is not None}
    m2 = torch.zeros((P, 3), device=gpu)
    bg = torch.tensor(scenes[0]["bg"], device=gpu)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    other = synth.make_camera(W, H)                     # the colour camera: another one, which the forward must not read
    cams = [types.SimpleNamespace(world_view_transform=t(other["viewmatrix"]), full_proj_transform=t(other["projmatrix"]),
                                  camera_center=t(other["campos"]), world_view_transform_tof=t(sc["cam"]["viewmatrix"]),
                                  full_proj_transform_tof=t(sc["cam"]["projmatrix"]), camera_center_tof=t(sc["cam"]["campos"]),
                                  frame_id=v, depth_range=10.0, phase_offset=0.0, dc_offset=0.0) for v, sc in enumerate(scenes)]
    store = views.ViewStore.from_cameras(cams, gpu)
    cam = store.camera("tof")

    def render(settings):
        with torch.no_grad():
            return GaussianRasterizer(raster_settings=settings)(
                means3D=leaf["means3D"], means2D=m2, opacities=leaf["opacities"], shs=leaf["shs"], shs_p=leaf["shs_p"],
                scales=leaf["scales"], rotations=leaf["rotations"], phase_offset=0.1, dc_offset=0.05)

    api._instance_hint.clear()
    try:
        refs = []
        for _ in range(2):                              # the first frame of the shape, then the one-call flow
            refs = [[o.clone() for o in render(Hh.gpu_settings(sc, gpu, bg=bg))] for sc in scenes]
        torch.cuda.synchronize()
        assert all(len(r) == 11 for r in refs)
        assert not torch.equal(refs[0][0], refs[1][0]) and not torch.equal(refs[1][0], refs[2][0])
        order = (2, 0, 1)
        store.schedule(order)
        static_settings = Hh.gpu_settings(scenes[0], gpu, bg=bg, viewmatrix=cam.world_view_transform,
                                          projmatrix=cam.full_proj_transform, campos=cam.camera_center)

        def region():
            store.draw()
            return render(static_settings)

        graph, static = _capture(region, after_warm_up=lambda: store.schedule(order))
        for k in range(2 * 3 + 1):
            graph.replay()
            torch.cuda.synchronize()
            v = order[k % 3]
            assert int(store.index.item()) == v
            for name, got, want in zip(Hh.OUT_NAMES, static, refs[v]):
                assert torch.equal(got, want), (k, v, name)
        st = [x for x in api.enqueue_status() if x["key"][1:4] == (P, W, H)]
        assert st and all(not x["overflow"] for x in st)
    finally:
        api._instance_hint.clear()


PLANE_SHAPES = ((4, 9, 6), (7, 5, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PLANE_SHAPES)
def test_select_plane(gpu, shape):
    from gftorf_amd import views
    C_ = shape[0]
    gen = torch.Generator().manual_seed(SEED + C_)
    whole = torch.randn((C_ + 3,) + shape[1:], generator=gen).to(gpu)
    x = whole[3:]                                       # as phasor[3:]: contiguous, its first plane wherever it falls
    perm = torch.randperm(C_, generator=gen).to(torch.int32)
    ups = [torch.randn((1,) + shape[1:], generator=gen).to(gpu) for _ in range(2)]
    word = torch.zeros((1,), device=gpu, dtype=torch.int32)

    def both(i, table, modulo, up):
        """(forward, gradient) of select_plane and of the torch statement, the index by value and from the device word"""
        j = i % modulo if modulo else i
        p = int(table[j]) if table is not None else j
        leaf = x.clone().requires_grad_(True)
        want = leaf[p].unsqueeze(0)
        want.backward(up)
        outs = []
        word.fill_(i)
        for index in (i, word):
            mine = whole.clone().requires_grad_(True)
            got = views.select_plane(mine[3:], index, table=None if table is None else table.to(gpu), modulo=modulo)
            got.backward(up)
            assert not mine.grad[:3].any()
            outs.append((got.detach(), mine.grad[3:]))
        return (want.detach(), leaf.grad), outs

    cases = [(i, table, None) for table in (None, perm) for i in range(C_)]
    if C_ >= 4:
        cases += [(i, table, 4) for table in (None, perm[perm < 4] if C_ > 4 else perm) for i in range(12)]
    for n, (i, table, modulo) in enumerate(cases):
        (want, want_g), outs = both(i, table, modulo, ups[n % 2])
        for got, got_g in outs:
            assert got.shape == (1,) + shape[1:] and torch.equal(got, want), (i, modulo, table is not None)
            # the gradient tensor is the function's own allocation, so it cannot be pre-filled: consecutive cases pick other
            # planes and use another incoming gradient, and every element, the zeros too, has to be right each time
            assert got_g.shape == x.shape and torch.equal(got_g, want_g), (i, modulo, table is not None)
    # the host-side checks
    for bad, kw in ((C_, {}), (-1, {}), (4, dict(table=perm[:4].to(gpu))), (0, dict(modulo=0))):
        with pytest.raises(ValueError):
            views.select_plane(x, bad, **kw)
    with pytest.raises(RuntimeError, match="contiguous"):
        views.select_plane(whole[:, 1:], 0)
    with pytest.raises(TypeError, match="int32"):
        views.select_plane(x, torch.zeros((1,), device=gpu, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="requires grad"):
        views.select_plane(x, torch.zeros((1,), device=gpu, requires_grad=True))


def _cameras(with_images=True):
    """8 stand-ins for ToFCamera, frame_id 0..7 of 9 views; flows on some of the integer frames"""
    rng = np.random.default_rng(SEED + 2)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    cams = []
    for v in range(8):
        cam = types.SimpleNamespace(frame_id=v, depth_range=np.float32(7.5 + v), phase_offset=np.array(0.01 * v, np.float32),
                                    dc_offset=torch.tensor(0.5 - v), forward_flow=None, backward_flow=None)
        for tail in ("", "_tof"):
            setattr(cam, "world_view_transform" + tail, f(4, 4))
            setattr(cam, "full_proj_transform" + tail, f(4, 4))
            setattr(cam, "camera_center" + tail, f(3))
        if with_images:
            cam.original_image = torch.from_numpy(rng.integers(0, 256, (3, 7, 5)).astype(np.uint8)) / 255.0
            cam.original_tof_image = f(3, 9, 6)
            cam.original_tofQuad_im = f(4, 9, 6)
            cam.original_distance_image = f(1, 9, 6)
        cams.append(cam)
    cams[0].forward_flow = f(2, 9, 6)
    cams[4].forward_flow, cams[4].backward_flow = f(2, 9, 6), f(2, 9, 6)
    cams[5].backward_flow = f(2, 9, 6)                  # not an integer frame: the schedule ignores it
    return cams


@pytest.mark.gpu
@pytest.mark.parametrize("sync,flow_window,color", ((False, True, "u8"), (True, False, "f32")))
def test_from_cameras(gpu, sync, flow_window, color):
    from gftorf_amd import query, views
    cams = _cameras()
    total = 9
    store = views.ViewStore.from_cameras(cams, gpu, total_num_views=total, sync=sync, flow_window=flow_window, color=color)
    assert set(store.current) == {"color", "phasor", "quad", "distance", "forward_flow", "backward_flow"}
    assert store.layout.slab_offsets[1] - store.layout.slab_offsets[0] == (112 if color == "u8" else 432)
    f32 = lambda values: torch.tensor(values, dtype=torch.float64).to(torch.float32)
    for v in (0, 4, 5, 7, 1, 2, 3, 6):
        cam = cams[v]
        store.draw(v)
        times, combine, names = query.ftorf_schedule(cam.frame_id, total, sync, cam.forward_flow is not None and flow_window,
                                                     cam.backward_flow is not None and flow_window)
        K, M = len(times), len(combine)
        assert int(store.K.item()) == K and int(store.M.item()) == M and len(names) == M
        assert torch.equal(store.times.cpu(), f32(times + [0.0] * (4 - K)))
        pad = torch.zeros((4, 4))
        pad[:M, :K] = f32(combine)
        assert torch.equal(store.combine.cpu(), pad)
        assert torch.equal(store.time.cpu(), f32([cam.frame_id / (total - 1)]))                 # train.py:167
        assert torch.equal(store.quad.cpu(), torch.tensor([cam.frame_id % 4], dtype=torch.int32))   # train.py:219
        assert torch.equal(store.frame_id.cpu(), torch.tensor([cam.frame_id], dtype=torch.int32))
        assert store.quad.dtype == store.K.dtype == store.index.dtype == torch.int32 and store.times.dtype == torch.float32
        for which, tail in (("color", ""), ("tof", "_tof")):
            c = store.camera(which)
            assert torch.equal(c.world_view_transform.cpu(), getattr(cam, "world_view_transform" + tail))
            assert torch.equal(c.full_proj_transform.cpu(), getattr(cam, "full_proj_transform" + tail))
            assert torch.equal(c.camera_center.cpu(), getattr(cam, "camera_center" + tail))
        assert torch.equal(store.depth_range.cpu(), f32([7.5 + v])) and torch.equal(store.dc_offset.cpu(), f32([0.5 - v]))
        assert torch.equal(store.phase_offset.cpu(), torch.from_numpy(np.array([0.01 * v], np.float32)))
        for name, attr in views.CAMERA_GROUPS:
            image = getattr(cam, attr)
            assert int(store.has(name).item()) == (image is not None), (v, name)
            assert torch.equal(store.current[name].cpu(), image if image is not None else torch.zeros_like(store.current[name].cpu()))
    if color == "u8":
        cams[3].original_image = cams[3].original_image + 1e-3
        with pytest.raises(ValueError, match="f32"):
            views.ViewStore.from_cameras(cams, gpu, total_num_views=total)


@pytest.mark.gpu
def test_captured_select_plane_follows_the_quad_word(gpu):
    """train.py:219-220 inside a graph: the planes follow store.quad from replay to replay"""
    from gftorf_amd import views
    cams = _cameras()
    store = views.ViewStore.from_cameras(cams, gpu, total_num_views=9)
    gen = torch.Generator().manual_seed(SEED + 3)
    phasor = torch.randn((7, 9, 6), generator=gen).to(gpu)
    inv_perm = torch.tensor([2, 0, 3, 1], dtype=torch.int32, device=gpu)
    order = (5, 2, 7, 0, 6)
    store.schedule(order)

    def region():
        store.draw()
        return (views.select_plane(store.current["quad"], store.quad).clone(),
                views.select_plane(phasor[3:], store.quad, table=inv_perm).clone())

    graph, (tof_gt, tof_rendered) = _capture(region, after_warm_up=lambda: store.schedule(order))
    for k in range(2 * len(order) + 1):
        graph.replay()
        torch.cuda.synchronize()
        cam = cams[order[k % len(order)]]
        assert torch.equal(tof_gt.cpu(), cam.original_tofQuad_im[cam.frame_id % 4].unsqueeze(0)), k
        assert torch.equal(tof_rendered, phasor[3:][inv_perm.long()][cam.frame_id % 4].unsqueeze(0)), k
