"""gftorf_amd.pcd: ToF frames to world points, the input cloud's PLY file and create_from_pcd (include/gftorf_pcd.h,
csrc/k_pcd.hip), against tests/pcd_ref.py, the numpy restatement of scene/dataset_readers.py:110-150, 530-586, 904-973,
1067-1118, and against eager torch for scene/gaussian_model.py:180-236.

unproject is held to a two-part contract.  (a) The distance against the float64 restatement within
3 * ref_err_depth_tof * depth_range, the bound tests/test_present.py holds depth_tof_f to (tests/golden/present.npz records
ref_err_depth_tof, numpy's own float32 error): the device's atan2f is not numpy's arctan2.  (b) xyz against the restatement fed
the device's own distances: both sides are then the same float64 expression up to a few double roundings (the inverse by the
adjugate here, by LAPACK there; the 4 x 4 product's order), so the float32 results are equal or neighbours, and the
amplitude-derived float32 values are equal.  The frames keep every phase PHASE_MARGIN from the wrap, every amplitude
AMP_MARGIN from 0.04 and every F-ToRF candidate DIST_MARGIN from znear and 10.5 (pcd_ref.make_frame), each far above the
distance's error bound of (a) (about 1e-5), so (b)'s neighbour is the only slack.
"""
import os
import re
import types

import numpy as np
import pytest
import torch

import pcd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_pcd.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pcd.npz")
GOLDEN_PLY = os.path.join(ROOT, "tests", "golden", "points3d_small.ply")
PRESENT_GOLDEN = os.path.join(ROOT, "tests", "golden", "present.npz")
MODES = ("torf_init", "ftorf_init", "proxy")
# (H, W, stride): one pixel; ceil; odd sizes at two strides; 1023 pixels = four workgroups with a ragged last one, H' != W'
FRAMES = ((1, 1, 1), (3, 5, 2), (13, 17, 1), (13, 17, 3), (31, 33, 1))
FORMS = ((False, False), (True, False), (True, True), (False, True))       # (phase and amplitude, seg colours): 27, 35, 38, 30 bytes
SEED = 20261020


def neighbours(got, want):
    """float32 arrays equal or one unit in the last place apart, element by element"""
    return (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))


# ---- CPU-runnable checks ------------------------------------------------------------------------------------------------

def test_header_declares_the_exports():
    from gftorf_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"\b(gft_pcd_\w+)\s*\(", src)
    assert sorted(names) == sorted(_lib.PCD_EXPORTS), names
    defines = dict(re.findall(r"#define (GFT_PCD_\w+) (\d+)", src))
    assert int(defines["GFT_PCD_ROWS"]) == _lib.PCD_ROWS and int(defines["GFT_PCD_MAX_ROW_BYTES"]) == _lib.PCD_MAX_ROW_BYTES
    assert int(defines["GFT_PCD_STATUS_WORDS"]) == _lib.PCD_STATUS_WORDS and int(defines["GFT_PCD_FIELDS"]) == len(_lib.PCD_FIELDS)
    assert [int(defines["GFT_PCD_" + m.upper()]) for m in _lib.PCD_MODES] == [0, 1, 2]


def test_store_header_and_row_layout_against_the_fixture():
    """the header and the row layout the host-side table code builds are the fixture file's"""
    from gftorf_amd import pcd
    data = open(GOLDEN_PLY, "rb").read()
    head = pcd.header(5)
    assert data.startswith(head) and len(data) == len(head) + 5 * 38
    for has_pa, has_seg in FORMS:
        dtype = np.dtype(R.store_dtype(has_pa, has_seg))
        layout, row_bytes = pcd.row_layout(pcd.properties(has_pa, has_seg))
        assert row_bytes == dtype.itemsize == 27 + 8 * has_pa + 3 * has_seg
        assert {n: (o, {"float": "<f4", "uchar": "|u1"}[k]) for n, (o, k) in layout.items()} == \
            {n: (dtype.fields[n][1], dtype.fields[n][0].str) for n in dtype.names}
    # the fixture's rows decoded at the table's offsets are fetchPly's values
    z = np.load(GOLDEN)
    offsets, row_bytes = pcd.field_offsets(pcd.properties())
    rows = np.frombuffer(data, np.uint8, offset=len(head)).reshape(5, row_bytes)
    want = R.fetch_bytes(data)
    f4 = lambda o: rows[:, o:o + 4].copy().view("<f4")[:, 0]
    assert np.array_equal(np.stack([f4(o) for o in offsets[:3]], 1), z["cloud_xyz"].astype(np.float32))
    assert np.array_equal(np.stack([f4(o) for o in offsets[:3]], 1), want["points"])
    assert np.array_equal(np.stack([rows[:, o] for o in offsets[6:9]], 1) / 255.0, want["colors"])
    assert np.array_equal(f4(offsets[9]), z["cloud_phases"][:, 0]) and np.array_equal(f4(offsets[10]), z["cloud_amplitudes"][:, 0])
    assert np.array_equal(np.stack([rows[:, o] for o in offsets[11:]], 1) / 255.0, want["seg_colors"])
    assert data == R.store_bytes(*[z[k] for k in ("cloud_xyz", "cloud_colors", "cloud_phases", "cloud_amplitudes", "cloud_seg")])


def test_parse_header_with_uchar_columns():
    from gftorf_amd import pcd, ply
    data = open(GOLDEN_PLY, "rb").read()
    P, props, offset = ply.parse_header(data, uchar=True)
    assert P == 5 and offset == len(pcd.header(5))
    assert [p if k == "float" else (p, k) for p, k in props] == pcd.properties()
    with pytest.raises(NotImplementedError, match="uchar red"):
        ply.parse_header(data)                                   # the model's reader still refuses them
    for has_pa, has_seg in FORMS:
        P, props, _ = ply.parse_header(pcd.header(7, has_pa, has_seg), uchar=True)
        offsets, row_bytes = pcd.field_offsets(props)
        assert P == 7 and row_bytes == 27 + 8 * has_pa + 3 * has_seg
        assert (offsets[9] >= 0) == (offsets[10] >= 0) == has_pa and all((o >= 0) == has_seg for o in offsets[11:])
    # columns in another order, an extra column, `amplitude` without `phase`: found by name, the pair only together
    props = [("red", "uchar"), ("extra", "float"), ("x", "float"), ("y", "float"), ("z", "float"), ("amplitude", "float"),
             ("green", "uchar"), ("blue", "uchar"), ("nx", "float"), ("ny", "float"), ("nz", "float")]
    offsets, row_bytes = pcd.field_offsets(props)
    assert row_bytes == 35 and offsets[:9] == [5, 9, 13, 23, 27, 31, 0, 21, 22] and offsets[9:] == [-1] * 5
    with pytest.raises(ValueError, match="no property `blue`"):
        pcd.field_offsets([p for p in props if p[0] != "blue"])


def test_restatement_invariants():
    """the reference's oddities, which are the contract: equal torf_init halves, the F-ToRF amplitude index, the raise"""
    H, W, s = 5, 7, 2
    cam, tof = R.camera(W, H), R.make_frame(5, 7, SEED)
    args = (cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], R.DEPTH_RANGE, R.PHASE_OFFSET)
    t = R.unproject(tof, s, *args, "torf_init")
    n = t["xyz"].shape[0] // 2
    assert n == 3 * 4 and all(np.array_equal(v[:n], v[n:]) for v in t.values())
    # (i // W', i % H'): with H' = 3, W' = 4 pixel i = 7 reads the amplitude of image pixel (1, 1), not of its own (2, 6)
    f = R.unproject(tof, s, *args, "ftorf_init")
    first = R.depth_from_tof(tof[::s, ::s].reshape(-1, 3), R.DEPTH_RANGE, R.PHASE_OFFSET)[:, 0]
    took_second = f["dist"] - first > R.DEPTH_RANGE / 4
    own = np.array([R.amplitude_is_low(tof[(i // 4) * s, (i % 4) * s, 2]) for i in range(n)])
    odd = np.array([R.amplitude_is_low(tof[i // 4, i % 3, 2]) for i in range(n)])
    assert np.array_equal(took_second, odd) and not np.array_equal(odd, own)
    # no candidate in (znear, 10.5]: depth_range / 2 = 12 puts the second one beyond, a distance of 0.2 the first one below
    dist = np.full((H, W), 2.0)
    dist[2, 4] = 0.2
    with pytest.raises(IndexError):
        R.unproject(R.make_frame(H, W, SEED, depth_range=24.0, dist=dist), s, *args[:4], 24.0, R.PHASE_OFFSET, "ftorf_init")
    # H' > W: the amplitude index leaves the image
    with pytest.raises(IndexError):
        R.unproject(R.make_frame(7, 3, SEED), 1, *args, "ftorf_init")
    # the comparison of :940 as the reference's numpy makes it
    a = np.float32(0.04)
    assert R.amplitude_is_low(a) and R.amplitude_is_low(np.nextafter(a, np.float32(0))) and not R.amplitude_is_low(np.nextafter(a, np.float32(1)))


def test_restatement_u1_columns():
    """what numpy does when a Python float is assigned to a uint8 field, recorded: values in (-1, 256) truncate towards zero, the
    rest raises; pcd_ref.to_u1, which the restatement's files are made with, does the same value for value"""
    xyz = np.zeros((1, 3))
    field = np.zeros(1, dtype=[("b", "u1")])
    for v, byte in ((0.0, 0), (-0.5, 0), (-0.999, 0), (0.999, 0), (1.0, 1), (254.999, 254), (255.0, 255), (255.999, 255)):
        field[0] = (v,)
        assert field["b"][0] == byte == R.to_u1([v])[0]
        assert R.fetch_bytes(R.store_bytes(xyz, np.full((1, 3), v)))["colors"][0, 0] == byte / 255.0
    for v, error in ((256.0, OverflowError), (-1.0, OverflowError), (300.7, OverflowError), (1e30, OverflowError),
                     (float("nan"), ValueError), (float("inf"), OverflowError), (float("-inf"), OverflowError)):
        with pytest.raises(error):
            field[0] = (v,)
        with pytest.raises(error):
            R.to_u1([v])
        with pytest.raises(error):
            R.store_bytes(xyz, np.full((1, 3), v))


def test_fixture_is_the_restatement():
    z = np.load(GOLDEN)
    cam = R.camera(7, 5)
    assert np.array_equal(z["view"], cam["view"]) and np.array_equal(z["tof"], R.make_frame(5, 7, SEED))
    for mode in MODES:
        got = R.unproject(z["tof"], 1 if mode == "proxy" else int(z["stride"]), cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"],
                          R.DEPTH_RANGE, R.PHASE_OFFSET, mode, rendered=z["rendered"] if mode == "proxy" else None)
        for k, v in got.items():
            assert np.array_equal(z["%s_%s" % (mode, k)], v.astype(np.float32) if k == "xyz" else v), (mode, k)


# ---- GPU ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ref_err():
    return float(np.load(PRESENT_GOLDEN)["ref_err_depth_tof"])


_FRAMES = {}


def frame(H, W, **kw):
    """pcd_ref.make_frame, made once per size and shared"""
    key = (H, W) + tuple(sorted(kw.items()))
    if key not in _FRAMES:
        _FRAMES[key] = R.make_frame(H, W, SEED + 7 * H + W, **kw)
    return _FRAMES[key]


def run_unproject(gpu, tof, stride, cam, mode, depth_range=R.DEPTH_RANGE, phase_offset=R.PHASE_OFFSET, rendered=None):
    from gftorf_amd import pcd
    out = pcd.unproject(torch.tensor(tof, device=gpu), stride, cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], depth_range,
                        phase_offset, mode=mode, rendered=None if rendered is None else torch.tensor(rendered, device=gpu))
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_unproject(got, tof, stride, cam, mode, ref_err, rendered=None, depth_range=R.DEPTH_RANGE, what=""):
    """the two-part contract of the module docstring"""
    args = (cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], depth_range, R.PHASE_OFFSET)
    ref = R.unproject(tof, stride, *args, mode, rendered=rendered)
    assert set(got) == set(ref) and all(got[k].shape == ref[k].shape for k in ref), (what, sorted(got))
    assert got["dist"].dtype == ref["dist"].dtype, (what, got["dist"].dtype, ref["dist"].dtype)
    # (a) the distances: the frame's own against float64, with the candidate the float32 restatement chose
    H, W = tof.shape[:2]
    xs, ys, Hp, Wp = R.screen(H, W, stride)
    n = Hp * Wp
    d64 = R.depth_from_tof64(tof[ys, xs, :], depth_range, R.PHASE_OFFSET)[:, 0]
    d32 = R.depth_from_tof(tof[ys, xs, :], depth_range, R.PHASE_OFFSET)[:, 0]
    if mode == "ftorf_init":
        d64 = d64 + np.where(ref["dist"] - d32 > depth_range / 4, depth_range / 2.0, 0.0)
    err, bound = float(np.abs(got["dist"][:n] - d64).max()), 3 * ref_err * np.float32(depth_range)
    print("%s dist: err %.3g bound %.3g" % (what, err, bound))
    assert err <= bound, (what, err, bound)
    if mode == "torf_init":
        assert all(np.array_equal(v[:n], v[n:]) for v in got.values()), what
    if mode == "proxy":
        assert np.array_equal(got["dist"][n:], rendered[ys, xs]), what
    # (b) everything behind the distance, from the device's own
    fed = R.unproject(tof, stride, *args, mode, rendered=rendered, dist=got["dist"])
    want = fed["xyz"].astype(np.float32)
    ok = neighbours(got["xyz"], want)
    print("%s xyz: %d of %d differ, all by one unit in the last place: %s" % (what, int((got["xyz"] != want).sum()), want.size, bool(ok.all())))
    assert ok.all(), (what, np.argwhere(~ok)[:4].tolist(), got["xyz"][~ok][:4], want[~ok][:4])
    for k in fed:
        if k not in ("xyz", "dist"):
            assert got[k].dtype == np.float32 and np.array_equal(got[k], fed[k]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W,stride", FRAMES)
def test_unproject(gpu, ref_err, H, W, stride, mode):
    if mode == "proxy":
        stride = 1                                                  # the proxy clouds are at full sensor resolution
    cam, tof = R.camera(W, H), frame(H, W)
    for wide in ((False, True) if mode == "proxy" else (False,)):
        rendered = None
        if mode == "proxy":
            rendered = np.random.default_rng(SEED + H).uniform(1.0, 3.0, (H, W)).astype(np.float64 if wide else np.float32)
        got = run_unproject(gpu, tof, stride, cam, mode, rendered=rendered)
        check_unproject(got, tof, stride, cam, mode, ref_err, rendered=rendered, what="%s %dx%d/%d%s" % (mode, H, W, stride, " f64" * wide))


@pytest.mark.gpu
def test_unproject_fixture_and_device_scalars(gpu, ref_err):
    """the committed fixture's frame; depth_range and phase_offset as one-element device tensors give the same bits"""
    from gftorf_amd import pcd
    z = np.load(GOLDEN)
    cam, tof, s = R.camera(7, 5), z["tof"], int(z["stride"])
    for mode in MODES:
        rendered = z["rendered"] if mode == "proxy" else None
        got = run_unproject(gpu, tof, 1 if mode == "proxy" else s, cam, mode, rendered=rendered)
        check_unproject(got, tof, 1 if mode == "proxy" else s, cam, mode, ref_err, rendered=rendered, what="fixture " + mode)
        assert np.abs(got["xyz"] - z[mode + "_xyz"]).max() < 1e-4                # the recorded points, up to the distance's error
    by_value = run_unproject(gpu, tof, s, cam, "torf_init")
    on_device = pcd.unproject(torch.tensor(tof, device=gpu), s, cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"],
                              torch.tensor([R.DEPTH_RANGE], device=gpu), torch.tensor(R.PHASE_OFFSET, device=gpu))
    assert all(np.array_equal(by_value[k], on_device[k].cpu().numpy()) for k in by_value)


@pytest.mark.gpu
def test_unproject_frame_list_into_one_output(gpu):
    """a frame list is a loop of launches into consecutive row ranges of one output"""
    from gftorf_amd import pcd
    cam, frames = R.camera(5, 3), [frame(3, 5), frame(3, 5, low_amp=0.2)]
    rows = pcd.frame_rows("torf_init", 3, 5, 2)
    out = pcd.alloc_points(2 * rows + 1, gpu)
    for t in out.values():
        t.fill_(-7.0)
    for i, tof in enumerate(frames):
        pcd.unproject(torch.tensor(tof, device=gpu), 2, cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], R.DEPTH_RANGE, R.PHASE_OFFSET,
                      out=out, row=i * rows)
    for i, tof in enumerate(frames):
        alone = run_unproject(gpu, tof, 2, cam, "torf_init")
        assert all(np.array_equal(out[k][i * rows:(i + 1) * rows].cpu().numpy(), alone[k]) for k in alone)
    assert all(bool((t[2 * rows:] == -7.0).all()) for t in out.values())         # nothing behind the last frame's rows
    with pytest.raises(RuntimeError, match="rows"):
        pcd.unproject(torch.tensor(frames[0], device=gpu), 2, cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], R.DEPTH_RANGE,
                      R.PHASE_OFFSET, out=out, row=rows + 2)


@pytest.mark.gpu
def test_ftorf_amplitude_threshold_is_exact(gpu):
    """amplitudes at float32(0.04) and its two neighbours: the candidate chosen is the reference's (a float64 comparison:
    float32(0.04) < 0.04), and one-candidate pixels take the one kept"""
    H = W = 4                                                       # H' = W' and stride 1: the reference's index is the pixel's own
    cam = R.camera(W, H)
    dist = np.full((H, W), 2.0)
    dist[3, 0], dist[3, 1] = 0.2, 0.3                               # below znear: only z + depth_range / 2 is kept
    tof = R.make_frame(H, W, SEED, dist=dist).copy()
    a = np.float32(0.04)
    tof[0, 0, 2], tof[0, 1, 2], tof[0, 2, 2] = np.nextafter(a, np.float32(0)), a, np.nextafter(a, np.float32(1))
    tof[3, 0, 2], tof[3, 1, 2] = 0.5, 0.01
    got = run_unproject(gpu, tof, 1, cam, "ftorf_init")
    ref = R.unproject(tof, 1, cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], R.DEPTH_RANGE, R.PHASE_OFFSET, "ftorf_init")
    second = lambda d: (d.reshape(H, W) > R.DEPTH_RANGE / 2)
    assert np.array_equal(second(got["dist"]), second(ref["dist"]))
    assert second(got["dist"])[0, :3].tolist() == [True, True, False] and second(got["dist"])[3, :2].tolist() == [True, True]
    # a larger depth_range: z + depth_range / 2 leaves (znear, 10.5] where z > 2.5, and only z is kept whatever the amplitude
    tof16 = R.make_frame(H, W, SEED, depth_range=16.0, dist=np.linspace(1.0, 4.0, 16).reshape(H, W))
    got = run_unproject(gpu, tof16, 1, cam, "ftorf_init", depth_range=16.0)
    ref = R.unproject(tof16, 1, cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], 16.0, R.PHASE_OFFSET, "ftorf_init")
    assert np.array_equal(got["dist"] > 8.0, ref["dist"] > 8.0) and (got["dist"] > 8.0).any() and not (got["dist"] > 8.0).all()


@pytest.mark.gpu
def test_ftorf_raises_where_the_reference_does(gpu, tmp_path):
    from gftorf_amd import pcd
    H, W, s = 5, 7, 2
    cam = R.camera(W, H)
    dist = np.full((H, W), 2.0)
    dist[2, 4] = 0.2
    tof = R.make_frame(H, W, SEED, depth_range=24.0, dist=dist)
    f = dict(tof_image=torch.tensor(tof, device=gpu), znear=cam["znear"], FovX_tof=cam["fov_x"], FovY_tof=cam["fov_y"], world_view=cam["view"])
    path = str(tmp_path / "points3d.ply")
    with pytest.raises(ValueError, match=r"ftorf_init: 1 pixel\(s\) with no distance candidate .* and 0 whose"):
        pcd.phase_init_ftorf([f], s, 24.0, R.PHASE_OFFSET, path)
    assert not os.path.exists(path)
    # H' > W: the reference's amplitude index leaves the image where both candidates are kept
    tall = R.make_frame(7, 3, SEED)
    n_out = sum(1 for i in range(21) if i % 7 >= 3)
    with pytest.raises(ValueError, match=r"0 pixel\(s\) with no distance candidate .* and %d whose" % n_out):
        pcd.unproject(torch.tensor(tall, device=gpu), 1, cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], R.DEPTH_RANGE, R.PHASE_OFFSET,
                      mode="ftorf_init")


def cloud_on(gpu, cloud, has_pa, has_seg, offset_view=False):
    """store's arguments on the device; `offset_view`: every tensor a view one row into a larger buffer"""
    def put(a):
        if a is None:
            return None
        if not offset_view:
            return torch.tensor(a, device=gpu)
        big = torch.zeros((a.shape[0] + 1,) + a.shape[1:], device=gpu, dtype=torch.tensor(a[:0]).dtype)
        big[1:] = torch.tensor(a, device=gpu)
        return big[1:]
    xyz, colors, phases, amplitudes, seg = cloud
    return [put(xyz), put(colors), put(phases) if has_pa else None, put(amplitudes) if has_pa else None, put(seg) if has_seg else None]


def assert_cloud(got, want, what):
    for k in ("points", "normals", "colors", "phases", "amplitudes", "seg_colors"):
        g, w = getattr(got, k), want[k]
        assert (g is None) == (w is None), (what, k)
        if w is not None:
            g, w = g.cpu().numpy(), np.ascontiguousarray(w)
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k, g.dtype, w.dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("P", (1, 2, 63, 64, 65, 257))
def test_store_and_fetch(gpu, tmp_path, P):
    """every column form: the file's bytes are the restatement's, fetch gives fetchPly's tensors bit for bit, and the cloud
    store hands on is what fetch reads back.  Rows of 27, 30, 35 and 38 bytes straddle dwords within a workgroup's run (every
    P > 1); a workgroup takes 256 rows, which begin on a dword of the file, so P = 257 is the case with a second run and every
    P with P * row bytes not a multiple of 4 has the ragged last dword"""
    from gftorf_amd import pcd
    cloud = R.make_cloud(P, SEED + P)
    for has_pa, has_seg in FORMS:
        for offset_view in (False, True):
            what = "P=%d pa=%d seg=%d view=%d" % (P, has_pa, has_seg, offset_view)
            want = R.store_bytes(cloud[0], cloud[1], cloud[2] if has_pa else None, cloud[3] if has_pa else None, cloud[4] if has_seg else None)
            path = str(tmp_path / ("c%d%d%d.ply" % (has_pa, has_seg, offset_view)))
            job = pcd.submit_store(path, *cloud_on(gpu, cloud, has_pa, has_seg, offset_view), want_cloud=True)
            job.finish(chunk_bytes=1000 if offset_view else None)
            data = open(path, "rb").read()
            assert data == want, (what, len(data), len(want), next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), None))
            fetched = R.fetch_bytes(want)
            assert_cloud(pcd.fetch(path, device=gpu, chunk_rows=100 if offset_view else None), fetched, what + " fetch")
            assert_cloud(job.cloud, fetched, what + " handed on")


@pytest.mark.gpu
def test_store_fixture_and_phases_alone(gpu, tmp_path):
    from gftorf_amd import pcd
    z = np.load(GOLDEN)
    cloud = [z[k] for k in ("cloud_xyz", "cloud_colors", "cloud_phases", "cloud_amplitudes", "cloud_seg")]
    path = str(tmp_path / "sub" / "points3d.ply")                   # the folder is made
    pcd.store(path, *cloud_on(gpu, cloud, True, True))
    assert open(path, "rb").read() == open(GOLDEN_PLY, "rb").read()
    assert_cloud(pcd.fetch(GOLDEN_PLY), R.fetch_bytes(open(GOLDEN_PLY, "rb").read()), "fixture")
    # storePly writes the phasor columns only when both are given
    xyz, colors, phases, _, _ = cloud_on(gpu, cloud, True, False)
    pcd.store(path, xyz, colors, phases, None)
    assert open(path, "rb").read() == R.store_bytes(cloud[0], cloud[1], cloud[2], None)


@pytest.mark.gpu
def test_store_colours_out_of_range(gpu, tmp_path):
    """the recorded behaviour of numpy's float -> u1 assignment: (-1, 0) truncates to 0; 256, -1 and beyond (the infinities
    too) raise OverflowError, a NaN ValueError, and no file is written"""
    from gftorf_amd import pcd
    xyz = torch.zeros((3, 3), device=gpu)
    path = str(tmp_path / "bad.ply")
    ok = np.array([[-0.5, -0.999, 0.999], [254.999, 255.0, 255.999], [0.0, 1.0, 128.5]])
    for dtype in (np.float32, np.float64):
        pcd.store(path, xyz, torch.tensor(ok.astype(dtype), device=gpu))
        assert open(path, "rb").read() == R.store_bytes(np.zeros((3, 3)), ok.astype(dtype))
    os.remove(path)
    for v, error, count in ((256.0, OverflowError, 1), (-1.0, OverflowError, 1), (1e30, OverflowError, 1), (float("inf"), OverflowError, 1),
                            (float("nan"), ValueError, 1)):
        bad = ok.copy()
        bad[1, 2] = v
        for seg in (False, True):
            good = torch.tensor(ok, device=gpu)
            with pytest.raises(error, match="^gftorf_amd.pcd: %d colour" % count):
                pcd.store(path, xyz, good if seg else torch.tensor(bad, device=gpu), seg_colors=torch.tensor(bad, device=gpu) if seg else None)
            assert not os.path.exists(path)


def fetched_cloud(gpu, P, has_pa=True, has_seg=True):
    """the cloud fetchPly reads from the restatement's file of pcd_ref.make_cloud(P), on the device"""
    from gftorf_amd import pcd
    c = R.make_cloud(P, SEED + P)
    f = R.fetch_bytes(R.store_bytes(c[0], c[1], c[2] if has_pa else None, c[3] if has_pa else None, c[4] if has_seg else None))
    return pcd.Cloud(**{k: None if v is None else torch.tensor(v, device=gpu) for k, v in f.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("max_sh_degree", (0, 3))
@pytest.mark.parametrize("P", (4, 5, 257))
def test_create_tensors(gpu, P, max_sh_degree):
    """every tensor equals eager torch's statements on the same device, bit for bit"""
    from gftorf_amd import pcd
    for has_pa, has_seg in ((True, True), (False, False)):
        cloud = fetched_cloud(gpu, P, has_pa, has_seg)
        for isotropic in (False, True):
            for init_static_first in (False, True):
                what = "P=%d D=%d pa=%d iso=%d static=%d" % (P, max_sh_degree, has_pa, isotropic, init_static_first)
                want = R.eager_create(cloud, max_sh_degree, isotropic, init_static_first, 0.1)
                got = pcd.create_tensors(cloud, max_sh_degree, isotropic=isotropic, init_static_first=init_static_first, initial_opacity=0.1)
                assert set(got) == set(want), (what, sorted(got), sorted(want))
                for k in want:
                    assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and got[k].is_contiguous(), (what, k, got[k].shape)
                    assert torch.equal(got[k], want[k]), (what, k, (got[k] != want[k]).sum().item())


@pytest.mark.gpu
def test_create_from_pcd_sets_the_model(gpu):
    """the model-object form: the reference's attributes, requires_grad flags and zero offsets"""
    from gftorf_amd import pcd
    for isotropic, has_pa in ((False, True), (True, True), (False, False)):
        cloud = fetched_cloud(gpu, 65, has_pa, has_pa)
        model = types.SimpleNamespace(max_sh_degree=2)
        args = types.SimpleNamespace(isotropic_gaussians=isotropic, init_static_first=False, initial_opacity=0.1)
        pcd.create_from_pcd(model, cloud, 3.5, 7.25, args)
        want = R.eager_create(cloud, 2, isotropic, False, 0.1)
        assert model.isotropic == isotropic and model.cameras_extent == 3.5 and model.scene_extent == 7.25
        # the reference writes nn.Parameter(t.requires_grad_(False)) for `_features_seg_color` and the isotropic `_rotation`; the
        # constructor's own requires_grad=True wins, so every parameter of the reference's model takes a gradient
        assert torch.nn.Parameter(torch.zeros(1).requires_grad_(False)).requires_grad
        names = ["_xyz", "_features_dc_color", "_features_rest_color", "_scaling", "_rotation", "_opacity"]
        if has_pa:
            names += ["_features_dc_phase", "_features_rest_phase", "_features_dc_amp", "_features_rest_amp", "_features_seg_color",
                      "_phase_offset", "_dc_offset"]
        flags = {name: True for name in names}
        for name, grad in flags.items():
            p = getattr(model, name)
            assert isinstance(p, torch.nn.Parameter) and p.requires_grad == grad and p.is_leaf, name
            assert torch.equal(p.detach(), want[name] if name in want else torch.zeros((1,), device=gpu)), name
        assert not isinstance(model.max_radii2D, torch.nn.Parameter) and torch.equal(model.max_radii2D, want["max_radii2D"])
        assert has_pa or not any(hasattr(model, n) for n in ("_features_dc_phase", "_features_dc_amp", "_features_seg_color", "_phase_offset"))


def init_frame(gpu, H, W, **kw):
    cam = R.camera(W, H)
    tof = frame(H, W, **kw)
    return cam, tof, dict(tof_image=torch.tensor(tof, device=gpu), znear=cam["znear"], FovX_tof=cam["fov_x"], FovY_tof=cam["fov_y"],
                          world_view=cam["view"])


@pytest.mark.gpu
def test_composites_write_the_file_and_hand_on_its_cloud(gpu, tmp_path):
    """phase_init_torf, phase_init_ftorf and proxy_clouds: the file is the restatement's storePly of the device's own points,
    and the cloud handed on is fetch of that file"""
    from gftorf_amd import pcd
    H, W, s = 13, 17, 3
    cam, tof, f = init_frame(gpu, H, W)
    cam2, tof2, f2 = init_frame(gpu, H, W, low_amp=0.2)
    args = (cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], R.DEPTH_RANGE, R.PHASE_OFFSET)
    # ToRF, two frames (:576-593)
    path = str(tmp_path / "torf.ply")
    cloud = pcd.phase_init_torf([f, f2], s, R.DEPTH_RANGE, R.PHASE_OFFSET, path)
    parts = [run_unproject(gpu, t, s, cam, "torf_init") for t in (tof, tof2)]
    xyz = np.concatenate([p["xyz"] for p in parts])
    colors = np.concatenate([p["color"] for p in parts])
    amplitudes = np.concatenate([p["amplitude"] for p in parts]).reshape(-1, 1)
    n = xyz.shape[0]
    seg = np.repeat(np.array([[1.0, 0.0, 0.0]]), n, axis=0)
    want = R.store_bytes(xyz, colors * 255.0, R.zero_phasor(n), amplitudes, seg * 255.0)
    assert open(path, "rb").read() == want
    assert_cloud(cloud, R.fetch_bytes(want), "torf")
    assert_cloud(pcd.fetch(path), R.fetch_bytes(want), "torf fetched")
    # F-ToRF: the first frame only, the colour columns are the seg colours (:962, :990)
    path = str(tmp_path / "ftorf.ply")
    cloud = pcd.phase_init_ftorf([f, f2], s, R.DEPTH_RANGE, R.PHASE_OFFSET, path)
    p = run_unproject(gpu, tof, s, cam, "ftorf_init")
    n = p["xyz"].shape[0]
    seg = np.repeat(np.array([[1.0, 0.0, 0.0]]), n, axis=0) * 255.0
    want = R.store_bytes(p["xyz"], seg, R.zero_phasor(n), p["amplitude"].reshape(-1, 1), seg)
    assert open(path, "rb").read() == want
    assert_cloud(cloud, R.fetch_bytes(want), "ftorf")
    # the proxy clouds of three frames through the two slots (:1109-1118)
    rng = np.random.default_rng(SEED)
    rendered = [rng.uniform(1.0, 3.0, (H, W)).astype(np.float32) for _ in range(3)]
    frames = [dict(f if i != 1 else f2, rendered=torch.tensor(r, device=gpu)) for i, r in enumerate(rendered)]
    paths = [str(tmp_path / "proxy_pcd" / ("frame_%d" % i) / "input.ply") for i in range(3)]
    clouds = list(pcd.proxy_clouds(frames, R.DEPTH_RANGE, R.PHASE_OFFSET, paths))
    assert len(clouds) == 3
    for i in range(3):
        p = run_unproject(gpu, tof2 if i == 1 else tof, 1, cam, "proxy", rendered=rendered[i])
        n = p["xyz"].shape[0]
        colors = np.tile([1, 0, 0], (n, 1)).astype(np.float32)
        colors[n // 2:, :] = np.tile([0, 0, 1], (n // 2, 1)).astype(np.float32)
        want = R.store_bytes(p["xyz"], colors * 255.0, R.zero_phasor(n), R.zero_phasor(n), np.zeros((n, 3)))
        assert open(paths[i], "rb").read() == want, i
        assert_cloud(clouds[i], R.fetch_bytes(want), "proxy %d" % i)


@pytest.mark.gpu
def test_phase_init_to_a_rendered_frame(gpu, tmp_path):
    """phase_init_torf on a 13 x 17 frame -> create_from_pcd -> one rasterizer forward through the same sensor: finite outputs,
    a non-zero visible count"""
    import helpers
    from gftorf_amd import GaussianRasterizer, pcd, synth
    H, W = 13, 17
    cam, tof, f = init_frame(gpu, H, W)
    cloud = pcd.phase_init_torf([f], 1, R.DEPTH_RANGE, R.PHASE_OFFSET, str(tmp_path / "points3d.ply"))
    model = types.SimpleNamespace(max_sh_degree=3)
    pcd.create_from_pcd(model, cloud, 1.0, 1.0, types.SimpleNamespace(isotropic_gaussians=False, init_static_first=False, initial_opacity=0.1))
    P = model._xyz.shape[0]
    assert P == 2 * H * W
    sensor = helpers.sensor_camera("anisotropic", W, H, w2c=synth.look_at_w2c(0.15, -0.1, 0.05, (0.1, -0.05, 0.2)))
    scene = dict(cfg=dict(P=P, W=W, H=H, D=3), cam=sensor, bg=synth.make_background(W, H, 3), depth_range=R.DEPTH_RANGE,
                 use_view_dependent_phase=True)
    rast = GaussianRasterizer(raster_settings=helpers.gpu_settings(scene, gpu))
    shs = torch.cat([model._features_dc_color, model._features_rest_color], dim=1)
    shs_p = torch.cat([torch.cat([model._features_dc_phase, model._features_rest_phase], dim=1),
                       torch.cat([model._features_dc_amp, model._features_rest_amp], dim=1)], dim=2)
    with torch.no_grad():
        outs = rast(means3D=model._xyz, means2D=torch.zeros((P, 3), device=gpu), opacities=torch.sigmoid(model._opacity), shs=shs, shs_p=shs_p,
                    colors_precomp=None, phasors_precomp=None, scales=torch.exp(model._scaling), rotations=model._rotation,
                    cov3D_precomp=None, phase_offset=0.0, dc_offset=0.0)
    o = dict(zip(helpers.OUT_NAMES, outs))
    assert all(bool(torch.isfinite(o[k]).all()) for k in ("color", "phasor", "depth", "acc"))
    visible = int((o["radii"] > 0).sum())
    print("visible %d of %d" % (visible, P))
    assert visible > 0 and float(o["acc"].max()) > 0


@pytest.mark.gpu
def test_no_host_read(gpu):
    """unproject in the torf_init and proxy modes and create_tensors run with every device-to-host synchronisation an error"""
    from gftorf_amd import pcd
    cam, tof, f = init_frame(gpu, 13, 17)
    t = f["tof_image"]
    rendered = torch.full((13, 17), 2.0, device=gpu)
    call = lambda **kw: pcd.unproject(t, 2, cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], **kw)
    cloud = fetched_cloud(gpu, 257)
    warm = pcd.create_tensors(cloud, 3, init_static_first=True), call(depth_range=R.DEPTH_RANGE)      # the library's first load
    dr, po = torch.tensor([R.DEPTH_RANGE], device=gpu), torch.tensor([R.PHASE_OFFSET], device=gpu)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = call(depth_range=R.DEPTH_RANGE, phase_offset=R.PHASE_OFFSET)
        b = call(depth_range=dr, phase_offset=po)
        pcd.unproject(t, 1, cam["znear"], cam["fov_x"], cam["fov_y"], cam["view"], dr, po, mode="proxy", rendered=rendered)
        again = pcd.create_tensors(cloud, 3, init_static_first=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert all(torch.equal(a[k], b[k]) for k in a) and all(torch.equal(again[k], warm[0][k]) for k in again)
