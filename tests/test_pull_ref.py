"""tests/pull_ref.py -- the numpy model of tile-pull binning's supertile shape and head rule -- pinned on the CPU: the shape
table of the frames that reach each code path, the library's own size query where it answers without a device, the model's
invariants on oracle lists, and what the scenes of helpers.BIG_GRIDS must reach for tests/test_gpu_big_grids.py to mean
anything (asserted on the oracle alone)."""
import os

import numpy as np
import pytest

import helpers as Hh
import pull_ref

# W, H -> sshift, NS, K, cells (computed by hand from gft_super_shape's rule: the smallest S = 2, 4, .. with
# ceil(gx / S) ceil(gy / S) <= 1024; K = 4 from S = 4 on)
SHAPES = {
    (640, 480): (1, 300, 1, 300),
    (4112, 16): (1, 129, 1, 129),
    (1024, 1024): (1, 1024, 1, 1024),          # NS = GFT_SUPER_MAX exactly; staged with one slab
    (1040, 1024): (2, 272, 4, 1088),
    (1025, 1025): (2, 289, 4, 1156),
    (1920, 1080): (2, 510, 4, 2040),
    (32784, 16): (2, 513, 4, 2052),
    (16, 32784): (2, 513, 4, 2052),
    (65552, 16): (3, 513, 4, 2052),
    (3840, 2160): (3, 510, 4, 2040),
    (131088, 16): (4, 513, 4, 2052),
}
NO_PULL = (262160, 16)


@pytest.mark.parametrize("W,H", list(SHAPES), ids=["%dx%d" % wh for wh in SHAPES])
def test_shape_table(W, H):
    sshift, NS, K, cells = SHAPES[(W, H)]
    sh = pull_ref.super_shape(W, H, slabs=0, copies=0)
    assert (sh.sshift, sh.NS, sh.K, sh.cells) == (sshift, NS, K, cells)
    assert pull_ref.tile_pull_ok(sh)
    assert (sh.gx, sh.gy, sh.T) == ((W + 15) // 16, (H + 15) // 16, ((W + 15) // 16) * ((H + 15) // 16))
    assert sh.sgx * sh.sgy == NS and (sh.sgx << sshift) >= sh.gx > ((sh.sgx - 1) << sshift) and (sh.sgy << sshift) >= sh.gy > ((sh.sgy - 1) << sshift)
    assert (1 << (12 - sh.kshift)) == K
    assert sh.staged == (cells >= 1024)                      # (no row of the table has more than 4096 cells)
    assert sh.copies == (8 if 8 * cells <= 16384 else 4)


def test_shape_edges_and_knobs():
    assert pull_ref.super_shape(1024, 1024, slabs=0, copies=0).staged
    assert not pull_ref.super_shape(992, 1024, slabs=0, copies=0).staged         # 62 x 64 tiles: 31 x 32 = 992 supertiles, direct scatter
    sh = pull_ref.super_shape(*NO_PULL, slabs=0, copies=0)
    assert sh.sshift == 5 and not pull_ref.tile_pull_ok(sh) and pull_ref.sched_words(sh) == 0
    sh = pull_ref.super_shape(1025, 1025, slabs=16, copies=0)
    assert (sh.K, sh.kshift, sh.cells, sh.staged, sh.copies) == (16, 8, 4624, False, 2)
    assert pull_ref.super_shape(1025, 1025, slabs=16, copies=1).copies == 1
    sh = pull_ref.super_shape(1025, 1025, slabs=2, copies=4)
    assert (sh.K, sh.kshift, sh.cells, sh.staged, sh.copies) == (2, 11, 578, False, 4)
    assert pull_ref.super_shape(1025, 1025, slabs=3, copies=3)[7:] == pull_ref.super_shape(1025, 1025, slabs=0, copies=0)[7:]   # not a knob's value
    assert pull_ref.super_shape(48, 32, slabs=16, copies=0).K == 16                                    # slabs can be forced on a small grid


def test_depth_bin_parameters():
    """Under the planes 0.45 / 6.05 a bin is 2^13 float steps and a slab of 1024 bins one octave of depth."""
    nb, shift = pull_ref.bin_params(0.45, 6.05)
    assert shift == 13 and nb == int(np.float32(0.45).view(np.uint32))
    bits = lambda z: np.array(z, np.float32).view(np.uint32)
    b = pull_ref.depth_bins(bits([0.1, 0.45, 0.9, 1.8, 3.6, 6.05, 1e9]), 0.45, 6.05)
    assert b[0] == 0 and b[1] == 0 and b[-1] == 4095 and (np.diff(b) >= 0).all()
    np.testing.assert_array_equal(b[2:5], [1024, 2048, 3072])                       # an octave = 2^23 steps = 1024 bins
    assert pull_ref.bin_params(0.01, 100.0)[1] == 15
    assert pull_ref.bin_params(0.0, 0.0) == (int(np.float32(1e-6).view(np.uint32)), 12)      # near clamped, far = 2 near: one octave = 2^23 steps, 2048 bins


@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


def test_library_agrees_on_the_cells(lib):
    """gft_cell_sched_words needs no device: 2 NS K + 4 words for every frame of the table (the model follows the slab knob of
    this process's environment, as the library does), 0 where the frame has no tile pull."""
    for W, H in SHAPES:
        sh = pull_ref.super_shape(W, H)
        assert int(lib.gft_cell_sched_words(W, H)) == 2 * sh.NS * sh.K + 4 == pull_ref.sched_words(sh), (W, H)
    assert int(lib.gft_cell_sched_words(*NO_PULL)) == 0


# ---- the model on oracle lists ---------------------------------------------------------------------------------------
SMALL = {      # tests/test_gpu_parity.py's scenes with the longest lists (their one-slab frames, and with slabs forced)
    "deep_lists": dict(P=1500, W=48, H=32, scale_lo=0.03, scale_hi=0.2),
    "long_lists_global": dict(P=24000, W=32, H=16, scale_lo=0.05, scale_hi=0.3),
    "long_lists_flat": dict(P=9000, W=32, H=32, scale_lo=0.05, scale_hi=0.3, w2c=None, z_lo=3.0, z_hi=3.0),   # one bin: empty heads
}


def check_model(f, scene, sh):
    m = pull_ref.head_model_of(f, scene, sh)
    lens = (f.ranges[:, 1] - f.ranges[:, 0]).astype(np.int64)
    assert (m.front_len <= m.tile_cnt).all() and (m.tile_cnt <= lens).all() and (m.front_len <= pull_ref.HEAD_SLOT).all()
    if sh.K == 1:
        np.testing.assert_array_equal(m.tile_cnt, lens)
        assert not m.more_slabs.any()
    # a tile whose list ends inside its head has a tail only through a later slab of its supertile; one without a tail has
    # its whole list in the head
    np.testing.assert_array_equal(m.front_len == lens, ~m.has_tail | (m.more_slabs & (m.front_len == m.tile_cnt) & (m.tile_cnt == lens)))
    assert (m.front_len[~m.has_tail] == lens[~m.has_tail]).all()
    np.testing.assert_array_equal(m.cut == pull_ref.NO_TAIL, ~m.has_tail)
    assert (m.front_len[m.by_crossing] < m.tile_cnt[m.by_crossing]).all()
    # the head is a union of whole depth bins: every bin in front of the cut, none from it on
    bits = np.ascontiguousarray(f.geom["depths"], np.float32).view(np.uint32)
    bins = pull_ref.depth_bins(bits, scene["cam"]["znear"], scene["cam"]["zfar"])
    for t in np.flatnonzero(m.has_tail):
        b = bins[f.point_list[int(f.ranges[t, 0]):int(f.ranges[t, 1])].astype(np.int64)]
        assert (np.diff(b) >= 0).all()
        k = int(m.front_len[t])
        assert (b[:k] < int(m.cut[t])).all() and (b[k:] >= int(m.cut[t])).all(), t
    return m, lens


@pytest.mark.parametrize("slabs", [1, 2, 4, 16])
@pytest.mark.parametrize("name", list(SMALL))
def test_model_on_small_frames(name, slabs, oracle):
    scene = Hh.small_scene(**SMALL[name])
    f, _ = Hh.run_oracle(oracle, scene, backward=False)
    sh = pull_ref.super_shape(scene["cfg"]["W"], scene["cfg"]["H"], slabs=slabs, copies=0)
    assert sh.sshift == 1 and sh.K == slabs
    m, lens = check_model(f, scene, sh)
    assert (lens > pull_ref.HEAD_DIRECT).any() or name == "deep_lists"
    if name == "long_lists_flat":
        assert (m.front_len == 0).all() and m.has_tail.all() and (m.cut < pull_ref.NO_TAIL).all()


PULLED = [n for n in Hh.BIG_GRIDS if n != "fallback"]


def _counts(m, lens):
    reach = m.tile_cnt >= pull_ref.HEAD_TARGET
    return dict(kstop=np.bincount(m.kstop[reach], minlength=4), crossing=int(m.by_crossing.sum()), more_slabs=int(m.more_slabs.sum()),
                short=int(((lens > 0) & (lens < pull_ref.HEAD_TARGET)).sum()), stops_early=int((m.tile_cnt < lens).sum()),
                long_tiles=int((lens >= pull_ref.HEAD_TARGET).sum()), longest=int(lens.max()))


@pytest.fixture(scope="module")
def big(oracle):
    out = {}
    for name in PULLED:
        sc, f, _ = Hh.big_grid_reference(oracle, name)
        sh = pull_ref.super_shape(sc["cfg"]["W"], sc["cfg"]["H"], slabs=0, copies=0)
        m, lens = check_model(f, sc, sh)
        out[name] = (sc, f, sh, m, lens, _counts(m, lens))
        print("\n[big grid] %s %dx%d: sshift %d K %d cells %d staged %s copies %d; R %d, %s" % (
            name, sc["cfg"]["W"], sc["cfg"]["H"], sh.sshift, sh.K, sh.cells, sh.staged, sh.copies, f.num_rendered,
            ", ".join("%s %s" % (k, v.tolist() if hasattr(v, "tolist") else v) for k, v in out[name][5].items())))
    return out


def test_big_grid_shapes(big):
    want = dict(all=(2, 4, True, 8), near=(2, 4, True, 8), mid=(2, 4, True, 8), far=(2, 4, True, 8), row=(2, 4, True, 4),
                col=(2, 4, True, 4), s8=(3, 4, True, 4), s16=(4, 4, True, 4), edge=(1, 1, True, 8))
    for name, (sc, f, sh, m, lens, c) in big.items():
        assert (sh.sshift, sh.K, sh.staged, sh.copies) == want[name], name
        assert (lens > 0).all() or name == "col", name       # the giant reaches every tile: no supertile without an entry
        assert f.radii[0] > 8 * min(sc["cfg"]["W"], sc["cfg"]["H"])
    assert big["col"][2].sgx == 1 and big["row"][2].sgy == 1
    sc = Hh.big_grid("fallback")
    assert not pull_ref.tile_pull_ok(pull_ref.super_shape(sc["cfg"]["W"], sc["cfg"]["H"], slabs=0, copies=0))
    # 1025 x 1025: the last supertile column and row are a single tile with one live pixel column / row, and the cluster sits
    # on the corner shared by four supertiles
    sh, lens = big["all"][2], big["all"][4]
    assert sh.gx == 65 and sh.sgx == 17 and lens[64] > 0 and lens[-1] > 0
    dense = np.flatnonzero(lens >= pull_ref.HEAD_TARGET)
    q = ((dense // sh.gx) >> sh.sshift) * sh.sgx + ((dense % sh.gx) >> sh.sshift)
    assert np.unique(q).size >= 4


def test_big_grid_scene_preconditions(big):
    """What the scenes must reach, on the oracle's lists alone.  Over the 1025 x 1025 scenes: heads that stop at every one of the
    four slabs, heads chosen by the bin-crossing rule, tiles that leave later slabs unread, and short lists.  The strips: heads
    that stop at the first and at a later slab, over many supertiles."""
    sq = [big[n][5] for n in ("all", "near", "mid", "far")]
    kstop = sum(c["kstop"] for c in sq)
    assert (kstop >= 1).all(), kstop
    assert sum(c["crossing"] for c in sq) >= 20
    assert sum(c["more_slabs"] for c in sq) >= 50
    assert sum(c["short"] for c in sq) >= 30
    assert big["far"][5]["kstop"][3] == big["far"][5]["long_tiles"] > 0 and big["far"][5]["more_slabs"] == 0      # all in the last slab
    assert big["mid"][5]["kstop"][2] == big["mid"][5]["long_tiles"] > 0
    for name in ("row", "s8", "s16"):
        c = big[name][5]
        assert c["kstop"][0] >= 1 and c["kstop"][1:].sum() >= 1, (name, c)
        assert c["more_slabs"] >= 50 and c["short"] >= 30 and c["stops_early"] >= 50, (name, c)
        sh, m = big[name][2], big[name][3]
        assert np.unique(np.flatnonzero(m.more_slabs) >> sh.sshift).size >= 20, name          # (gy = 1: supertile = tile x >> sshift)
        assert c["longest"] > 16384, name                                                     # beyond the LDS tail sorter: bin ranges
    c = big["col"][5]
    assert c["more_slabs"] >= 1 and c["crossing"] >= 1 and c["short"] >= 30, c
    c = big["edge"][5]
    assert c["crossing"] >= 20 and c["more_slabs"] == 0 and c["stops_early"] == 0, c          # one slab: the crossing rule alone


def test_low_opacity_variants_share_the_lists(oracle):
    for name in Hh.BIG_GRID_LOW_OPACITY:
        sc, f, _ = Hh.big_grid_reference(oracle, name)
        lo = Hh.big_grid(name + "@0.05")
        assert (lo["gaussians"]["opacities"] == np.float32(0.05)).all()
        for k, v in sc["gaussians"].items():
            if k != "opacities":
                assert v is not None and np.array_equal(v, lo["gaussians"][k])
