"""gftorf_amd.present.quad_images: the four quad images of the track program (render_ftorf_viz_traj.py:237-244;
scene/torf_utils.py:43-50 tof_to_image; matplotlib's `seismic` map).  The yardstick is the reference's own bytes
(tests/golden/present_quad.npz, written by tests/golden/make_golden_present_quad.py from the reference's tof_to_image).

Every statement is a fixed sequence of IEEE float32 operations -- `- 0.5`, the rounded division of the tonemap, the clip,
Normalize(-0.5, 0.5) (a float32 subtraction and a division by one) and matplotlib's index trunc(n * 256) --, so every byte
must be equal; `draw_quad` therefore puts values on the bin edges, one ulp to either side of them and outside the range, and
needs no conditioning.
"""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "present_quad.npz")
SIZES = {"one": (1, 1), "small": (5, 7), "ragged": (33, 65)}        # 33 x 65: more than one run of 256 pixels, a ragged tail
PERMUTATION = (2, 0, 3, 1)
OPTIONS = [(False, False), (True, False), (False, True), (True, True)]          # (has_gt, tonemap)


def special_values():
    """float32: -0.5 and 0.5, values beyond both, the 257 bin edges of the index with their float32 neighbours, NaN and the
    infinities; then the same shifted by + 0.5 (what `has_gt` brings back onto the edges) and -1 (the tonemap's pole)"""
    inf = np.float32(np.inf)
    first = np.array([-0.5, 0.5, 0.75, np.nan, -0.75, np.inf, -np.inf, 0.0, -0.0, -1.0, 3e38, -3e38], np.float32)
    e = np.arange(0, 257, dtype=np.float32) / np.float32(256) - np.float32(0.5)
    edges = np.concatenate([e, np.nextafter(e, inf), np.nextafter(e, -inf)]).astype(np.float32)
    direct = np.concatenate([first, edges])
    return np.concatenate([direct, direct + np.float32(0.5)]).astype(np.float32)


def draw_quad(rng, H, W):
    """phasor [7, H, W] float32: the quad planes begin with the special values (as many as fit; every size gets -0.5, 0.5, a
    value beyond and a NaN), the rest is uniform in [-1, 1.5]"""
    ph = rng.uniform(-1.0, 1.5, size=(7, H, W)).astype(np.float32)
    quad = ph[3:].reshape(-1)
    sp = special_values()
    if quad.size < sp.size:
        sp = np.concatenate([sp[:12], sp[12::7]])[:quad.size]
    quad[:sp.size] = sp
    return ph


def quad_np(phasor, table, permutation, has_gt, tonemap):
    """the kernel's statements in numpy float32: uint8 [4, H, W, 3]"""
    half = np.float32(0.5)
    out = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in permutation:
            v = phasor[3 + k].astype(np.float32)
            if has_gt:
                v = v - half
            if tonemap:
                v = v / (np.float32(1) + v)
            c = np.where(v < -half, -half, np.where(v > half, half, v)).astype(np.float32)
            s = (c + half) * np.float32(256)
            row = np.where(np.isnan(s), 256, np.where(s >= 256, 255, np.trunc(s))).astype(np.int64)
            out.append(table[row][..., :3])
    return np.stack(out)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


# ---- CPU-runnable checks ------------------------------------------------------------------------------------------------

def test_wrapper_rejects_what_is_not_a_seven_plane_phasor():
    from gftorf_amd import present
    with pytest.raises(RuntimeError, match=r"phasor must be \[7, H, W\], got \[3, 4, 5\]"):
        present.quad_images(torch.zeros(3, 4, 5))
    with pytest.raises(RuntimeError, match=r"phasor must be \[7, H, W\], got \[7, 4\]"):
        present.quad_images(torch.zeros(7, 4))
    with pytest.raises(TypeError, match="phasor must be torch.float32"):
        present.quad_images(torch.zeros(7, 4, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"permutation must be four integers in 0\.\.3"):
        present.quad_images(torch.zeros(7, 4, 5), permutation=(0, 1, 2, 4))
    with pytest.raises(ValueError, match=r"permutation must be four integers in 0\.\.3"):
        present.quad_images(torch.zeros(7, 4, 5), permutation=(0, 1, 2))
    with pytest.raises(TypeError, match=r"out must be a contiguous torch.uint8 tensor \[4, 4, 5, 3\]"):
        present.quad_images(torch.zeros(7, 4, 5), out=torch.zeros(4, 4, 5, 3))
    with pytest.raises(RuntimeError, match="phasor is on cpu; the display kernels run on a HIP device only, there is no CPU path"):
        present.quad_images(torch.zeros(7, 4, 5))


def test_the_numpy_statements_and_the_table_give_the_reference_bytes(golden):
    """`quad_np` with the library's table against what the reference's tof_to_image wrote into the fixture"""
    from gftorf_amd import _lib, present
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    table = present.seismic_table()
    assert table.shape == (257, 4) and np.array_equal(table, golden["seismic_u8"]) and not table[256].any()
    for name, (H, W) in SIZES.items():
        ph = golden[name + "_phasor"]
        assert ph.shape == (7, H, W)
        quad = ph[3:].reshape(-1)
        for v in (-0.5, 0.5, 0.75) + ((-0.75,) if quad.size > 4 else ()):         # 1 x 1 has four values
            assert (quad == np.float32(v)).any(), (name, v)
        assert np.isnan(quad).any()
        for has_gt, tonemap in OPTIONS:
            want = golden["%s_out_%d%d" % (name, has_gt, tonemap)]
            assert want.shape == (4, H, W, 3) and want.dtype == np.uint8
            assert np.array_equal(quad_np(ph, table, PERMUTATION, has_gt, tonemap), want), (name, has_gt, tonemap)
    big = golden["ragged_phasor"][3:].reshape(-1)
    assert np.isinf(big).sum() >= 2 and len(set(special_values()[12:12 + 3 * 257].tolist()) - set(big.tolist())) == 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SIZES))
def test_quad_images_are_the_reference_bytes(gpu, golden, name):
    from gftorf_amd import present
    H, W = SIZES[name]
    ph = torch.tensor(golden[name + "_phasor"], device=gpu)
    for has_gt, tonemap in OPTIONS:
        want = golden["%s_out_%d%d" % (name, has_gt, tonemap)]
        got = present.quad_images(ph, permutation=PERMUTATION, has_gt=has_gt, tonemap=tonemap)
        assert got.shape == (4, H, W, 3) and got.dtype == torch.uint8
        bad = np.argwhere(got.cpu().numpy() != want)
        assert not len(bad), (name, has_gt, tonemap, len(bad), bad[:4].tolist())
    # the default permutation shows the planes in their own order
    plain = present.quad_images(ph).cpu().numpy()
    permuted = golden["%s_out_00" % name]
    for i, k in enumerate(PERMUTATION):
        assert np.array_equal(plain[k], permuted[i])


@pytest.mark.gpu
def test_planes_are_read_in_place_and_out_is_written_in_place(gpu, golden):
    from gftorf_amd import present
    H, W = SIZES["ragged"]
    ph = golden["ragged_phasor"]
    wide = torch.full((7, H + 3, W), float("nan"), device=gpu)
    wide[:, :H] = torch.tensor(ph, device=gpu)
    view = wide[:, :H]                                       # whole rows cut from every plane: a plane stride of (H + 3) * W
    assert not view.is_contiguous()
    out = torch.full((4 * H * W * 3 + 8,), 7, device=gpu, dtype=torch.uint8)
    target = out[5:5 + 4 * H * W * 3].view(4, H, W, 3)       # an address that is no multiple of 4
    before = wide.clone()
    got = present.quad_images(view, permutation=PERMUTATION, has_gt=True, out=target)
    assert got.data_ptr() == target.data_ptr()
    assert np.array_equal(got.cpu().numpy(), golden["ragged_out_10"])
    assert bool((out[:5] == 7).all()) and bool((out[5 + 4 * H * W * 3:] == 7).all())
    assert torch.equal(wide.view(torch.int32), before.view(torch.int32))


@pytest.mark.gpu
def test_quad_images_can_be_captured(gpu, golden):
    from gftorf_amd import present
    H, W = SIZES["small"]
    ph = torch.tensor(golden["small_phasor"], device=gpu)
    out = torch.zeros((4, H, W, 3), device=gpu, dtype=torch.uint8)
    present.quad_images(ph, permutation=PERMUTATION, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        present.quad_images(ph, permutation=PERMUTATION, tonemap=True, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), golden["small_out_01"])
