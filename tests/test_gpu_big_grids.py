"""Tile-pull binning on big tile grids: the paths that gft_super_shape / gft_launch_super_bin choose from the size of the tile
grid alone -- supertiles of 4 x 4, 8 x 8 and 16 x 16 tiles with four depth slabs (k_tile_pull stops at the slab that covers
its head, k_tail_build skips slabs by range), the staged scatter (k_super_bin<1, true> / <2, true>), fewer counter copies,
the frame too wide for any supertile -- on the smallest frames that reach them (helpers.BIG_GRIDS; what each scene reaches
is asserted on the oracle in tests/test_pull_ref.py), by the measures small frames are held to:

  * stages: test_gpu_parity.py's bit-exact measure, whose tile-pull bookkeeping follows tests/pull_ref.py's model;
  * forward and backward through the public API against the oracle over a camera's first four frames: two-stage, one call, by
    the list schedule, whole lists by tile hints;
  * tile pull against whole-frame binning bit for bit, whole lists by schedule, schedules that change nothing;
  * the feature blend (flow.render_flows, C = 3 and C = 6);
  * the knobs GFT_SLABS, GFT_SUPER_COPIES, GFT_TAIL_RESUME, which the library reads once: a child process each."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as Hh
import pull_ref
from test_flow_render import _geometry, _ours, _reference_pair, _rel
from test_gpu_parity import (SCENES, BIN_CASES, binning_mode, check_all_ones_schedule_sorts_whole_lists, check_grads, check_outputs,
                             check_preprocess_and_binning_bit_exact,
                             check_tile_hints_do_not_change_results, check_tile_pull_matches_whole_frame_binning, render_mode,
                             worst_errors)

pytestmark = pytest.mark.gpu

LOW = [n + "@0.05" for n in Hh.BIG_GRID_LOW_OPACITY]
NAMES = list(Hh.BIG_GRIDS) + LOW
# name -> sshift, K, staged, copies: what the scene is named for (the library's defaults)
REACHES = dict(all=(2, 4, True, 8), near=(2, 4, True, 8), mid=(2, 4, True, 8), far=(2, 4, True, 8), row=(2, 4, True, 4),
               col=(2, 4, True, 4), s8=(3, 4, True, 4), s16=(4, 4, True, 4), edge=(1, 1, True, 8), fallback=(5, None, None, None))
KNOBS = ("GFT_SLABS", "GFT_SUPER_COPIES")


def check_frame_reaches_its_path(name, sc):
    """The frame has the supertile side, slabs, scatter and counter copies its name says -- by the model, by the library's
    answer on whether it pulls at all, and by the size of its list schedule."""
    from gftorf_amd import _lib
    lib = _lib.load()
    W, H = sc["cfg"]["W"], sc["cfg"]["H"]
    sh = pull_ref.super_shape(W, H)
    sshift, K, staged, copies = REACHES[name.partition("@")[0]]
    assert sh.sshift == sshift
    if not any(os.environ.get(k) for k in KNOBS) and K is not None:
        assert (sh.K, sh.staged, sh.copies) == (K, staged, copies), sh
    cfg = _lib.Config(P=sc["cfg"]["P"], W=W, H=H)
    with binning_mode(1):
        assert bool(lib.gft_binning_mode(C.byref(cfg))) == (pull_ref.tile_pull_ok(sh) and bool(lib.gft_lazy_sort()))
    assert int(lib.gft_cell_sched_words(W, H)) == pull_ref.sched_words(sh)
    return sh


@pytest.mark.parametrize("mode", [1, 0], ids=["tile_pull", "whole_frame"])
@pytest.mark.parametrize("name", NAMES)
def test_stages_bit_exact(name, mode, oracle, gpu):
    """`fallback` is not pulled in mode 1 either (the measure asserts that from the model) and passes as a whole-frame frame."""
    sc, f, _ = Hh.big_grid_reference(oracle, name)
    check_frame_reaches_its_path(name, sc)
    check_preprocess_and_binning_bit_exact(sc, mode, oracle, gpu, f=f)


def flagged_quadrants():
    """ctrl word 4 (GFT_CTRL_NFLAG) of the last forward's image buffer (api.keep_last_buffers)"""
    from gftorf_amd import _lib, api
    bufs = api.last_call_buffers
    L = _lib.get_layout(bufs["P"], bufs["W"], bufs["H"], bufs["cap"])
    return int(bufs["img"][L.img_ctrl:L.img_ctrl + 64].view(torch.int32)[4].item())


@pytest.mark.parametrize("name", NAMES)
def test_four_frames_vs_oracle(name, oracle, gpu):
    """A camera's first four frames through the public API, forward and backward against the oracle on each: the two-stage flow,
    one call with the buffer sized from the first, binning by the camera's list schedule (the scatter without a count pass),
    and -- the schedule's marked tiles given the whole-list build -- whole lists sorted up front."""
    from gftorf_amd import _lib, api
    sc, f, b = Hh.big_grid_reference(oracle, name, backward=True)
    pulls = pull_ref.tile_pull_ok(pull_ref.super_shape(sc["cfg"]["W"], sc["cfg"]["H"])) and bool(_lib.load().gft_lazy_sort())
    keep = (api._TILE_HINTS_PER_CAMERA, api.keep_last_buffers)
    api._TILE_HINTS_PER_CAMERA = False                 # (run_gpu builds new camera tensors per call: one schedule per image size)
    api.keep_last_buffers = True
    api._instance_hint.clear()
    api.state.reset_schedules()
    flagged = []
    try:
        with render_mode(0):
            for frame in range(4):
                api._force_whole_lists = True if frame == 3 else None
                misses = api.last_call_stats.get("sched_misses", 0)
                out, grads, _ = Hh.run_gpu(sc, gpu, optimize_offsets=True)
                st = api.last_call_stats
                assert st["num_rendered"] == f.num_rendered and not st["restarted"], frame
                flagged.append(flagged_quadrants())
                if frame == 0:
                    print("\n[big grid] %s: R %d, %s (GRAD_RTOL 3e-4)" % (name, f.num_rendered, worst_errors(f, out, b, grads, sc)))
                check_outputs(f, out)
                check_grads(b, grads, sc)
                if frame >= 2:
                    assert api.last_call_stats.get("sched_misses", 0) == misses, frame
            if pulls and api._CELL_SCHED and api._TILE_HINTS:
                cam = next(iter(api.state.cameras.values()))
                assert cam.sched_seen and cam.cell_sched is not None and cam.cell_sched is not False and cam.sched_off_until == 0
    finally:
        api._force_whole_lists = None
        api._TILE_HINTS_PER_CAMERA, api.keep_last_buffers = keep
        api.last_call_buffers.clear()
        api._instance_hint.clear()
        api.state.reset_schedules()
    print("[big grid] %s: flagged quadrants per frame %s" % (name, flagged))
    if pulls and api._TILE_HINTS:
        if name in LOW:
            assert flagged[0] > 0, flagged                  # few pixels saturate inside a head: tiles with a tail flag
        assert flagged[3] == 0, flagged                     # whole lists: nothing is completed on demand


BINNING = ["all", "all@0.05", "row", "s16"]


@pytest.mark.parametrize("name", BINNING)
def test_tile_pull_matches_whole_frame_binning(name, oracle, gpu):
    """test_gpu_parity.py's measure of the same name (the gradients' bound between the modes: that of its big-grid cases)."""
    from gftorf_amd import _lib
    if not _lib.load().gft_lazy_sort():
        pytest.skip("GFT_LAZY_SORT=0: whole-frame binning only")
    sc, f, b = Hh.big_grid_reference(oracle, name, backward=True)
    check_tile_pull_matches_whole_frame_binning(sc, oracle, gpu, rtol=3e-5, reference=(f, b))


@pytest.mark.parametrize("name", BINNING)
def test_tile_hints_do_not_change_results(name, oracle, gpu):
    """test_gpu_parity.py's measure of the same name: no schedule, the operator's, all ones, random ones, garbage list schedules."""
    from gftorf_amd import _lib
    if not _lib.load().gft_lazy_sort():
        pytest.skip("GFT_LAZY_SORT=0: whole-frame binning only")
    sc, f, b = Hh.big_grid_reference(oracle, name, backward=True)
    check_tile_hints_do_not_change_results(sc, oracle, gpu, rtol=3e-5, reference=(f, b))


@pytest.mark.parametrize("name", BINNING)
def test_hinted_tiles_sort_their_whole_list(name, oracle, gpu):
    """test_gpu_parity.py's measure of the same name, in the form that holds on a frame where SOME quadrants saturate inside their
    heads (the clusters' centres do, at any opacity the blend does not cull): without a schedule only tiles with a tail flag --
    a tail by tests/pull_ref.py's model: more than one placement, or a later slab of the supertile with entries --, and every
    tile that flags marks itself; under the schedule the frame left, every marked tile sorts its whole list -- it looks at all of
    its supertile's slabs --, nobody flags, and the images are the same bit for bit.  Then the schedule that marks every tile."""
    from gftorf_amd import _lib
    from test_gpu_parity import raw_forward
    if not _lib.load().gft_lazy_sort():
        pytest.skip("GFT_LAZY_SORT=0: whole-frame binning only")
    sc, f, _ = Hh.big_grid_reference(oracle, name)
    lens = (f.ranges[:, 1] - f.ranges[:, 0]).astype(np.int64)
    T = lens.size
    long_tiles = lens > 2048
    tails = pull_ref.head_model_of(f, sc).has_tail

    def check_whole(st, marked):
        """the marked tiles' lists are the oracle's, whole; those beyond one placement live in the pool"""
        np.testing.assert_array_equal(st["front_len"][marked], lens[marked])
        np.testing.assert_array_equal(st["tile_cnt"][marked], lens[marked])
        assert (st["tile_cut"][marked] == 0xffffffff).all()
        assert int(st["ctrl"][6]) == int(lens[marked & long_tiles].sum())                  # pool slots taken = the whole lists
        for t in np.flatnonzero(marked):
            a, e = int(st["ranges"][t, 0]), int(st["ranges"][t, 1])
            assert (a >= T * 2048) == bool(long_tiles[t]) or lens[t] == 0
            np.testing.assert_array_equal(st["point_list"][a:e], f.point_list[int(f.ranges[t, 0]):int(f.ranges[t, 1])], err_msg="tile %d" % t)

    with render_mode(0):
        h = torch.zeros((T,), device=gpu, dtype=torch.int32)
        st0 = raw_forward(sc, gpu, mode=1, hints=h)
        flagged = st0["unit_flag"].any(1)
        marked = st0["hints"].any(1)
        assert st0["pull"] and not flagged[~tails].any() and marked[flagged].all()
        assert int(st0["ctrl"][4]) == int((st0["unit_flag"] != 0).sum())
        if name in LOW:
            assert flagged.sum() >= 50 and (flagged & long_tiles).any() and (flagged & ~long_tiles).any()
        st = raw_forward(sc, gpu, mode=1, hints=h)                     # with the schedule the frame left
        assert not st["unit_flag"].any() and int(st["ctrl"][4]) == 0
        check_whole(st, marked)
        np.testing.assert_array_equal(st["planes"], st0["planes"])
        np.testing.assert_array_equal(st["pixels"], st0["pixels"])
        so = check_all_ones_schedule_sorts_whole_lists(sc, f, gpu, saturates=False)
        check_whole(so, np.ones(T, bool))


@pytest.mark.parametrize("name", ["all", "s16"])
def test_feature_blend(name, oracle, gpu):
    """flow.render_flows (C = 3, and the pair's C = 6 route) against two GaussianRasterizer(colors_precomp=...) calls, with the
    bounds of test_gpu_hostile.py's frame shapes and feature blend."""
    sc, f, _ = Hh.big_grid_reference(oracle, name)
    P, W, H = sc["cfg"]["P"], sc["cfg"]["W"], sc["cfg"]["H"]
    geo = _geometry(sc, gpu)
    settings = Hh.gpu_settings(sc, gpu)
    gen = torch.Generator().manual_seed(W + H)
    fa, fb = ((0.05 * torch.randn((P, 3), generator=gen)).to(gpu) for _ in range(2))
    ga, gb = (torch.randn((3, H, W), generator=gen).to(gpu) for _ in range(2))
    with render_mode(0):
        ia, ib, dfa, dfb = _ours(settings, geo, fa, fb, ga, gb)
        (ra, rb), (gra, grb), radii = _reference_pair(settings, geo, fa, fb, ga, gb)
        ia1, ib1, dfa1, dfb1 = _ours(settings, geo, fa, None, ga, None)
    torch.cuda.synchronize()
    print("\n[big grid] features %s: image_b %.3g, grad a %.3g, grad b %.3g, grad a (C = 3) %.3g"
          % (name, _rel(rb, ib), _rel(gra, dfa), _rel(grb, dfb), _rel(gra, dfa1)))
    assert torch.equal(ia, ra) and torch.equal(ia1, ra) and ib1 is None and dfb1 is None
    assert float(rb.abs().max()) > 0 and _rel(rb, ib) <= 1e-6
    assert float(gra.abs().max()) > 0 and _rel(gra, dfa) <= 1e-5 and _rel(grb, dfb) <= 1e-5 and _rel(gra, dfa1) <= 1e-5
    np.testing.assert_array_equal(radii.cpu().numpy(), f.radii)
    assert float(dfa[radii == 0].abs().max() if bool((radii == 0).any()) else 0.0) == 0.0


# ---- the knobs the library reads once per process ----------------------------------------------------------------------
CHILDREN = {
    "slabs2": dict(GFT_SLABS="2"),
    "slabs16_copies1": dict(GFT_SLABS="16", GFT_SUPER_COPIES="1"),
    "slabs4_no_tail_resume": dict(GFT_SLABS="4", GFT_TAIL_RESUME="0"),
    "slabs16": dict(GFT_SLABS="16"),          # `all` alone: 4624 cells, the direct scatter with the counters in 2 copies (8 -> 4 -> 2)
}
CHILD_SCENES = ("deep_lists", "long_lists_global", "wide_depth_range", "crowded_depth_bins", "thin_fog", "all")


def child_scene(name, oracle):
    """(scene, the oracle's forward, its backward)"""
    if name in Hh.BIG_GRIDS:
        return Hh.big_grid_reference(oracle, name, backward=True)
    sc = Hh.small_scene(seed=23, **BIN_CASES[name]) if name in BIN_CASES and name not in SCENES else Hh.small_scene(**SCENES[name])
    return (sc,) + tuple(Hh.run_oracle(oracle, sc))


def run_child_checks(want_slabs, want_copies, names=CHILD_SCENES):
    """What a child process runs under its knobs: on every scene of `names` the stage measure in both modes -- its model
    reads the same environment as the library -- and forward + backward against the oracle."""
    from oracle import oracle
    oracle.build()
    gpu = torch.device("cuda:0")
    for name in names:
        sc, f, b = child_scene(name, oracle)
        sh = pull_ref.super_shape(sc["cfg"]["W"], sc["cfg"]["H"])
        assert sh.K == want_slabs and (name != "all" or sh.copies == want_copies), (name, sh)
        for mode in (1, 0):
            check_preprocess_and_binning_bit_exact(sc, mode, oracle, gpu, f=f)
        out, grads, _ = Hh.run_gpu(sc, gpu, optimize_offsets=True)
        print("[big grid] child %s: K %d cells %d staged %s copies %d; %s" % (name, sh.K, sh.cells, sh.staged, sh.copies, worst_errors(f, out, b, grads, sc)), flush=True)
        check_outputs(f, out)
        check_grads(b, grads, sc)


@pytest.mark.parametrize("child", list(CHILDREN))
def test_knobs_in_a_child_process(child, tmp_path):
    """GFT_SLABS = 2 / 16 / 4, GFT_SUPER_COPIES = 1 and GFT_TAIL_RESUME = 0 (k_tail_build leaves the resume pass to a launch of
    k_render_fwd behind it): the slab logic also on 32 x 16 pixel frames with 24 000-entry lists; `all` under 16 slabs has 4624
    cells, the direct scatter, with one counter copy where the knob says so and with two where the library halves them."""
    env = dict(os.environ, **CHILDREN[child])
    here = os.path.dirname(os.path.abspath(__file__))
    script = tmp_path / "child.py"
    script.write_text(
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import test_gpu_big_grids\n"
        "test_gpu_big_grids.run_child_checks(%d, %d%s)\n" % (
            os.path.dirname(here), here, int(CHILDREN[child]["GFT_SLABS"]), dict(slabs16_copies1=1, slabs16=2).get(child, 8),
            ", names=('all',)" if child == "slabs16" else ""))
    subprocess.check_call([sys.executable, str(script)], env=env, timeout=300)
