"""gftorf_amd.tracks: the F-ToRF motion tracks (render_ftorf_viz_traj.py:262-347; scene/torf_utils.py:108-114).

Yardsticks:
  pos_last       the reference's sequential float32 additions run by torch on the CPU (tests/golden/tracks.npz, written by
                 tests/golden/make_golden_tracks.py with the reference's own project_points_subset): bit for bit
  xy, motion,    the statements in float64 (`statements_np`).  The kernel's projection is a fixed float32 sequence, the
  mean_z         reference's is a BLAS matmul and its means are torch's reductions, so neither can be matched to the bit.  The
                 fixture records, per quantity, the reference's own largest float32 distance from float64 over the cases
                 (`ref_err_*`); the kernel may be at most four times that away, with a floor of 2 ulp of the value -- the
                 factor allows for another, but still fixed, order of summation (DESIGN.md section 6 has the rule).  Every
                 fixture point is at least 0.2 in front of every camera, so the denominator is far from its 1e-7.
  step_ok        the comparisons of :318 and :339 evaluated on the kernel's own xy; and, like int(xy), the reference's on
                 inputs the generator has made safe: it redrew every point that has a coordinate nearer than 1e-3 px to an
                 integer (the bounds are integers) in the float64 or in the reference's float32 evaluation, and asserts that
                 none is left.  No point is left out of a comparison here.
  select         the reference's statements (:278-290) run by torch on the same device tensors
  walk           `walk_reference`, the loop of :297-347 restated with its own names and order, on a host table built so that
                 every branch is taken (asserted)
"""
import os
import re
import subprocess
import types
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_tracks.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tracks.npz")
SIZE = (48, 64)                                     # H, W of the fixture's ToF image
# name: (P, T, U).  P: one lane, a wave's edge from both sides, a workgroup's edge (256), several workgroups; T: one frame
# (no step), one step, a few, a sequence's 61; U < T: frames share a flow row (index t * U // T), U == T: one row each
CASES = {"p1": (1, 1, 1), "p63": (63, 2, 2), "p64": (64, 5, 2), "p65": (65, 61, 16), "p257": (257, 5, 5), "p1000": (1000, 2, 1),
         "wide": (1000, 5, 2), "long": (257, 61, 61)}
INPUTS = ("initial_pos", "flow", "flow_index", "K", "world_view")
# run_render.py: sliding_cube and occlusion of the synthetic block, fan of the real one
QUANTILES = [(0.9, 0.45, 0.9, 0.1, 0.9), (0.9, 0.45, 0.8, 0.2, 1.0), (0.75, 0.35, 0.01, 0.01, 0.5)]


# ---- the restatements ------------------------------------------------------------------------------------------------------

def draw_cameras(T):
    """K [T, 3, 3] and world_view [T, 4, 4] as a camera stores them: a camera that turns and drifts a little per frame, with a
    focal length that does too, so that a wrong frame's camera shows"""
    H, W = SIZE
    K = np.zeros((T, 3, 3), np.float64)
    view = np.zeros((T, 4, 4), np.float64)
    for t in range(T):
        a, b = 0.002 * t, -0.001 * t
        ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        m = np.eye(4)
        m[:3, :3] = rx @ ry
        m[:3, 3] = [0.03 + 0.001 * t, -0.02, 0.05 - 0.0005 * t]
        view[t] = m.T                                       # the transposed, row-vector convention
        K[t] = [[60.0 + 0.1 * t, 0.01, W / 2 - 0.25], [0.0, 61.0 - 0.05 * t, H / 2 + 0.25], [0.0, 0.0, 1.0]]
    return K.astype(np.float32), view.astype(np.float32)


def draw_points(rng, count, U):
    """`count` positions (world space, in front of the first camera, a good part of them outside the image) and their U
    flow rows"""
    z = rng.uniform(1.5, 4.0, count)
    cam = np.stack([z * rng.uniform(-0.7, 0.7, count), z * rng.uniform(-0.55, 0.55, count), z], axis=1)
    pos = cam - np.array([0.03, -0.02, 0.05])
    flow = rng.normal(0.0, 0.01, size=(U, count, 3))
    return pos.astype(np.float32), flow.astype(np.float32)


def positions_np(initial_pos, flow, flow_index, dtype):
    """all_3D_pos of :265-271, [T, P, 3]: sequential additions in `dtype` of the float32 inputs"""
    pos = [initial_pos.astype(dtype)]
    for v in range(1, len(flow_index)):
        pos.append(pos[-1] + flow[flow_index[v - 1]].astype(dtype))
    return np.stack(pos)


def statements_np(c, dtype=np.float64):
    """xy [T, P, 2], pos_last, motion, mean_z of a case's inputs, every step in `dtype`"""
    pos = positions_np(c["initial_pos"], c["flow"], c["flow_index"], dtype)
    T = pos.shape[0]
    xy = np.empty(pos.shape[:2] + (2,), dtype)
    for t in range(T):
        homog = np.concatenate([pos[t].T, np.ones((1, pos.shape[1]), dtype)], axis=0)
        h = c["K"][t].astype(dtype) @ (c["world_view"][t].astype(dtype).T @ homog)[:3]
        xy[t] = (h[:2] / (h[2:] + dtype(1e-7))).T
    per_frame = c["flow"][c["flow_index"]].astype(dtype)                                    # gs_xyz_flow [T, P, 3]
    return dict(xy=xy, pos_last=pos[-1], motion=(per_frame ** 2).sum(-1).mean(0), mean_z=pos[:, :, 2].mean(0))


def step_ok_np(xy, size=SIZE):
    """the conditions of :318 (frame 0) and :339 on an xy [T, P, 2], as Python compares the numbers: uint8 [T, P]"""
    H, W = size
    x, y = xy[..., 0].astype(np.float64), xy[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        start = (0 < x) & (x < W) & (0 < y) & (y < H)
        ok = np.empty(x.shape, bool)
        ok[0] = start[0]
        ok[1:] = (0 < x[1:]) & (x[1:] < W - 1) & (0 < y[1:]) & (y[1:] < H - 1) & start[:-1]
    return ok.astype(np.uint8)


def unsafe_points(xy, margin=1e-3):
    """bool [P]: a coordinate in some frame is nearer than `margin` px to an integer (every bound of step_ok is one)"""
    return (np.abs(xy - np.rint(xy)) < margin).any(axis=(0, 2))


def bound(err, v64):
    """four times the reference's own error, at least 2 ulp of the value"""
    return np.maximum(4 * err, 2 * np.spacing(np.abs(v64).astype(np.float32)).astype(np.float64))


def walk_reference(xy, motion, size, keep, radius):
    """The loop of :297-347 on host numbers: xy [T, S, 2] are all_2D_pos_, `keep(vid, i, init_x, init_y)` stands for the
    scene-name branches in front of the image filter.  Returns the per-frame (trajectories, colors) snapshots and the
    branches taken."""
    height, width = size
    T, S = xy.shape[:2]
    all_colors = reference_colors(S)
    trajectories, colors, frames = {}, {}, []
    taken = set()
    for vid in range(T):
        used_pixels = set()
        for i in range(S):
            init_x, init_y = float(xy[0, i, 0]), float(xy[0, i, 1])
            old_x, old_y = float(xy[vid - 1, i, 0]), float(xy[vid - 1, i, 1])
            new_x, new_y = float(xy[vid, i, 0]), float(xy[vid, i, 1])
            if not keep(vid, i, init_x, init_y):
                taken.add("dropped")
                continue
            if not (0 < init_x < width and 0 < init_y < height):
                taken.add("first outside")
                continue
            blocked = False
            for dx in range(-radius, radius + 1):
                for dy in range(-radius, radius + 1):
                    if (int(init_x) + dx, int(init_y) + dy) in used_pixels:
                        blocked = True
            if blocked:
                taken.add("blocked at the start" if vid == 0 else "blocked")
                continue
            if vid == 0:
                trajectories[i] = [[init_x, init_y]]
                colors[i] = tuple(map(int, all_colors[i]))
            else:
                if not (0 < new_x < width - 1 and 0 < new_y < height - 1 and 0 < old_x < width and 0 < old_y < height):
                    taken.add("step outside" if i in trajectories else "no step, no track")
                    if new_x != new_x or old_x != old_x:
                        taken.add("nan")
                    continue
                if i in trajectories.keys():
                    if len(trajectories[i]) < vid:
                        taken.add("came back")
                    trajectories[i].append([new_x, new_y])
                else:
                    taken.add("late start")
                    trajectories[i] = [[new_x, new_y]]
                    colors[i] = tuple(map(int, all_colors[i]))
            used_pixels.add((int(init_x), int(init_y)))
        frames.append(({k: [list(p) for p in v] for k, v in trajectories.items()}, dict(colors)))
    return frames, taken


def reference_colors(S):
    """generate_color_array(S) and the shuffle of :294-295, with numpy's global generator as the reference uses it"""
    state = np.random.get_state()
    try:
        np.random.seed(42)
        r = np.random.randint(0, 128, S)
        g = np.random.randint(128, 256, S)
        b = np.random.randint(128, 256, S)
        colors = np.stack([r, g, b], axis=1).astype(np.uint8)
        np.random.shuffle(colors)
    finally:
        np.random.set_state(state)
    return colors


def walk_table(T=6, S=40, size=(12, 16)):
    """A host table for `walk`: random tracks that drift over a 12 x 16 image, then rows placed by hand --
    rows 0, 1: neighbours at the start, so 1 is blocked by 0 in every frame; row 2: starts in the image, leaves it in frames 2
    and 3 and is back in frame 4; row 3: starts in the image but its frame-0 neighbour 4 comes first only in the frames where
    `keep` lets 4 through; row 5: dropped by `keep` in frame 0, starts late; row 6: a NaN from frame 3 on; row 7: outside at
    the start."""
    H, W = size
    rng = np.random.default_rng(7)
    start = np.stack([rng.uniform(-1.0, W + 1.0, S), rng.uniform(-1.0, H + 1.0, S)], axis=1)
    xy = start[None] + np.cumsum(rng.normal(0.0, 0.8, size=(T, S, 2)), axis=0)
    xy[0] = start
    xy[:, 0] = [5.5, 5.5]
    xy[:, 1] = [6.2, 5.1]
    xy[:, 2] = [[10.5, 2.5], [11.0, 2.5], [16.5, 2.5], [15.5, 2.5], [14.2, 2.6], [13.0, 2.7]][:T]
    xy[:, 3] = [2.5, 9.5]
    xy[:, 4] = [3.4, 9.6]
    xy[:, 5] = [13.5, 9.5]
    xy[:, 6] = [8.5, 1.5]
    xy[3:, 6] = np.nan
    xy[:, 7] = [-0.5, 3.5]
    xy = xy.astype(np.float32)
    # rows 8.. keep clear of the hand-placed starts, so those meet the branch they were placed for
    for i in range(8, S):
        while any(abs(int(xy[0, i, 0]) - int(xy[0, j, 0])) <= 1 and abs(int(xy[0, i, 1]) - int(xy[0, j, 1])) <= 1 for j in range(8)):
            xy[:, i, 0] += np.float32(2.0)
    # the table is in index order: put row 4 in front of row 3 by swapping them, so the earlier one blocks the later
    xy[:, [3, 4]] = xy[:, [4, 3]]
    from gftorf_amd import tracks
    motion = rng.uniform(0.0, 1.0, S).astype(np.float32)
    return tracks.HostTable(xy, step_ok_np(xy, size), motion, np.arange(S, dtype=np.int64) * 3, size)


def keep_rule(vid):
    """drops row 3 (the earlier of the two neighbours) in odd frames and row 5 in frame 0: bool [S] per frame"""
    def rule(i):
        return not ((i == 3 and vid % 2 == 1) or (i == 5 and vid == 0))
    return rule


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    out = {k: z[k] for k in z.files if "_" not in k or k.split("_", 1)[0] not in CASES}
    for name in CASES:
        out[name] = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    return out


# ---- not GPU ---------------------------------------------------------------------------------------------------------------

def _lib_built():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


def test_header_is_plain_c_and_every_symbol_is_exported(tmp_path):
    from gftorf_amd import _lib, build, tracks
    import gftorf_amd
    lib = _lib_built()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src)))
    assert names and all(n.startswith("gft_tracks_") for n in names)
    assert set(names) == set(_lib.TRACKS_EXPORTS), names
    for n in names:
        assert hasattr(lib, n), n
    assert "k_tracks.hip" in build.SOURCES and gftorf_amd.tracks is tracks and "struct" not in src
    prog = tmp_path / "tracks_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_tracks.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "tracks_abi.o")])
    words = ["GFT_TRACKS_" + k.upper() for k in _lib.TRACKS_PARTS] + ["GFT_TRACKS_PARTS"]
    out = subprocess.check_output(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-include", "gftorf_tracks.h",
                                   "-x", "c", "-"], input="TRACKS_WORDS_ARE " + " ".join(words) + "\n", text=True)
    assert [int(x) for x in out.split("TRACKS_WORDS_ARE", 1)[1].split()] == [0, 1, 2, 3, 4]
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16
    # the layout: every part aligned as its type asks, S == 0 valid, a bad T not
    total, off = tracks.table_layout(6, 40)
    assert off == {"index": 0, "xy": 320, "motion": 320 + 1920, "step_ok": 320 + 1920 + 160} and total == off["step_ok"] + 240
    assert tracks.table_layout(3, 0)[0] == 0 and tracks.table_layout(0, 5)[0] == 0


def test_the_fixture_is_what_its_docstring_says(golden):
    assert 0 < golden["ref_err_xy"] < 1e-4 and 0 < golden["ref_err_motion"] < 1e-8 and 0 < golden["ref_err_mean_z"] < 1e-5
    for name, (P, T, U) in CASES.items():
        c = golden[name]
        assert c["initial_pos"].shape == (P, 3) and c["flow"].shape == (U, P, 3) and c["K"].shape == (T, 3, 3)
        assert c["world_view"].shape == (T, 4, 4) and c["flow_index"].dtype == np.int32
        assert c["flow_index"].tolist() == [t * U // T for t in range(T)]
        s64, s32 = statements_np(c), statements_np(c, np.float32)
        # the sequential float32 sums are the reference's, bit for bit
        assert np.array_equal(s32["pos_last"].view(np.uint32), c["ref_pos_last"].view(np.uint32)), name
        # safe: the float64 coordinates here; the reference's float32 ones were checked when the fixture was made
        assert not unsafe_points(s64["xy"]).any(), name
        assert np.array_equal(step_ok_np(s64["xy"]), c["ref_step_ok"]) and np.array_equal(s64["xy"].astype(np.int32), c["ref_xy_int"])
        homog = np.concatenate([positions_np(c["initial_pos"], c["flow"], c["flow_index"], np.float64), np.ones((T, P, 1))], axis=2)
        depth = np.einsum("tpk,tkr->tpr", homog, c["world_view"].astype(np.float64))[..., 2]
        assert depth.min() >= 0.2, (name, depth.min())
        if T > 1:
            assert 0 < c["ref_step_ok"].mean() < 1, name            # both outcomes occur
    assert golden["select_opacity"].shape == (1000, 1) and golden["select_scaling"].shape == (1000, 3)


@pytest.mark.parametrize("S", [0, 40])
def test_walk_is_the_reference_loop(S):
    from gftorf_amd import tracks
    full = walk_table()
    host = tracks.HostTable(full.xy[:, :S], full.step_ok[:, :S], full.motion[:S], full.index[:S], full.size)
    keep = lambda vid: np.array([keep_rule(vid)(i) for i in range(S)], dtype=bool)
    want, taken = walk_reference(host.xy, host.motion, host.size, lambda vid, i, x, y: keep_rule(vid)(i), 1)
    got = []
    for vid, trajectories, colors in tracks.walk(host, radius=1, keep=keep):
        assert vid == len(got)
        got.append(({k: [list(p) for p in v] for k, v in trajectories.items()}, dict(colors)))
    assert len(got) == host.T == 6
    for vid, ((t_got, c_got), (t_want, c_want)) in enumerate(zip(got, want)):
        assert list(t_got) == list(t_want) and t_got == t_want, vid           # the same keys in the same order, the same points
        assert c_got == c_want and list(c_got) == list(c_want), vid
        assert all(type(v) is float for p in t_got.values() for q in p for v in q)
        assert all(type(v) is int for c in c_got.values() for v in c)
    if S:
        assert taken >= {"dropped", "first outside", "blocked at the start", "blocked", "step outside", "came back", "late start", "nan"}, taken
        last = want[-1][0]
        assert 0 in last and 1 not in last                              # row 1 never got past its neighbour
        assert len(last[2]) == 4 and 5 in last and len(last[5]) == 5    # left and came back; started late
        assert len(last[6]) == 3 and 7 not in last                      # the NaN ends a track; outside at the start
        assert 3 in last and 4 in last and len(last[4]) == 3            # the later neighbour draws in the frames the earlier is dropped
        # no keep at all, a fixed bool array, and another radius
        plain, _ = walk_reference(host.xy, host.motion, host.size, lambda vid, i, x, y: True, 2)
        for (t_w, c_w), (_, t_g, c_g) in zip(plain, tracks.walk(host, radius=2)):
            assert t_w == t_g and c_w == c_g
        fixed = np.arange(S) % 3 != 0
        some, _ = walk_reference(host.xy, host.motion, host.size, lambda vid, i, x, y: bool(fixed[i]), 1)
        for (t_w, c_w), (_, t_g, c_g) in zip(some, tracks.walk(host, keep=fixed)):
            assert t_w == t_g and c_w == c_g
        with pytest.raises(ValueError, match=r"keep must give a bool \[40\]"):
            list(tracks.walk(host, keep=np.ones(39, bool)))
    else:
        assert all(t == {} and c == {} for t, c in got)


@pytest.mark.parametrize("S", [1, 40])
def test_colors_are_the_reference_generator_and_shuffle(golden, S):
    from gftorf_amd import tracks
    state = np.random.get_state()
    got = tracks.color_array(S)
    assert got.dtype == np.uint8 and np.array_equal(got, golden["colors_%d" % S])
    assert np.array_equal(reference_colors(S), golden["colors_%d" % S])
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]     # the caller's generator is left alone


def _cpu_args(P=6, T=3, U=2, n=None):
    n = P if n is None else n
    return dict(initial_pos=torch.zeros(P, 3), flow=torch.zeros(U, n, 3), flow_index=torch.zeros(T, dtype=torch.int32),
                K=torch.zeros(T, 3, 3), world_view=torch.zeros(T, 4, 4), size=(12, 16))


def test_argument_errors_come_before_the_library_is_needed():
    from gftorf_amd import tracks
    bad = [(dict(flow_index=torch.zeros(3, dtype=torch.int64)), TypeError, "flow_index must be torch.int32"),
           (dict(flow_index=torch.zeros(4, dtype=torch.int32)), RuntimeError, r"flow_index must be \[3\], one row of flow per frame, got \[4\]"),
           (dict(K=torch.zeros(3, 3, 4)), RuntimeError, r"K must be \[T, 3, 3\], got \[3, 3, 4\]"),
           (dict(K=torch.zeros(3, 3)), RuntimeError, r"K must be \[T, 3, 3\]"),
           (dict(world_view=torch.zeros(3, 3, 4)), RuntimeError, r"world_view must be \[3, 4, 4\], got \[3, 3, 4\]"),
           (dict(world_view=torch.zeros(2, 4, 4)), RuntimeError, r"world_view must be \[3, 4, 4\], got \[2, 4, 4\]"),
           (dict(initial_pos=torch.zeros(6, 2)), RuntimeError, r"initial_pos must be \[P, 3\]"),
           (dict(initial_pos=torch.zeros(6, 3, dtype=torch.float64)), TypeError, "initial_pos must be torch.float32"),
           (dict(flow=torch.zeros(2, 5, 3)), RuntimeError, r"without a motion mask flow must have n = P = 6 rows, got 5"),
           (dict(flow=torch.zeros(6, 3)), RuntimeError, r"flow must be \[U, n, 3\]"),
           (dict(size=(0, 16)), ValueError, r"size must be \(H, W\)"),
           (dict(size=16), TypeError, r"size must be \(H, W\)"),
           (dict(motion_mask=torch.tensor([True, False, True, True, False, False])), RuntimeError,
            "the motion mask has 3 set entries, flow has n = 6 rows"),
           (dict(motion_mask=torch.ones(5, dtype=torch.bool)), RuntimeError, r"motion_mask must be \[6\]"),
           (dict(motion_mask=torch.ones(6)), TypeError, "motion_mask must be torch.bool")]
    for change, kind, message in bad:
        with pytest.raises(kind, match=message):
            tracks.integrate(**dict(_cpu_args(), **change))
    with pytest.raises(RuntimeError, match="initial_pos is on cpu; the track kernels run on a HIP device only, there is no CPU path"):
        tracks.integrate(**_cpu_args())
    with pytest.raises(RuntimeError, match="initial_pos is on cpu"):                 # a mask with the right count gets as far
        tracks.integrate(**dict(_cpu_args(n=3), motion_mask=torch.tensor([True, False, True, True, False, False])))
    with pytest.raises(TypeError, match="table takes the Tracks of integrate"):
        tracks.table(None, torch.ones(3, dtype=torch.bool))
    with pytest.raises(TypeError, match="select takes the Tracks of integrate"):
        tracks.select(None, torch.ones(3, 1), torch.ones(3, 3))
    with pytest.raises(ValueError, match="needs at least one frame"):
        tracks.sequence_flows(None, torch.zeros(4, 3), [], 59)


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def on(dev, c):
    return {k: torch.tensor(c[k], device=dev) for k in INPUTS}


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def same_tracks(a, b):
    return all(same_bits(getattr(a, k), getattr(b, k)) for k in ("xy", "pos_last", "motion", "mean_z", "step_ok"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_integrate_against_the_fixture(gpu, golden, name):
    from gftorf_amd import tracks
    P, T, U = CASES[name]
    c = golden[name]
    tr = tracks.integrate(size=SIZE, **on(gpu, c))
    assert tr.xy.shape == (T, P, 2) and tr.step_ok.shape == (T, P) and tr.step_ok.dtype == torch.uint8 and tr.size == SIZE
    got = {k: getattr(tr, k).cpu().numpy() for k in ("xy", "pos_last", "motion", "mean_z", "step_ok")}
    assert np.array_equal(got["pos_last"].view(np.uint32), c["ref_pos_last"].view(np.uint32))
    assert np.array_equal(got["step_ok"], step_ok_np(got["xy"]))
    assert np.array_equal(got["step_ok"], c["ref_step_ok"])
    assert np.array_equal(got["xy"].astype(np.int32), c["ref_xy_int"])
    s64 = statements_np(c)
    for k in ("xy", "motion", "mean_z"):
        err = np.abs(got[k].astype(np.float64) - s64[k])
        lim = bound(float(golden["ref_err_" + k]), s64[k])
        print("%s %s: err %.3g, reference's %.3g, worst err / bound %.3g" % (name, k, err.max(), golden["ref_err_" + k], (err / lim).max()))
        assert (err <= lim).all(), (name, k, float(err.max()), float((err / lim).max()))
    again = tracks.integrate(size=SIZE, **on(gpu, c))
    assert same_tracks(tr, again)


@pytest.mark.gpu
def test_motion_mask(gpu, golden):
    from gftorf_amd import DeformQuery, tracks
    c = golden["long"]                                   # P = 257: two workgroups, the second with one row
    P, T, U = CASES["long"]
    t = on(gpu, c)
    g = torch.Generator().manual_seed(5)
    mask = (torch.rand(P, generator=g) < 0.4).to(gpu)
    mask[256] = True                                     # the lone row of the last workgroup is dynamic
    n = int(mask.sum())
    assert 0 < n < P
    flow = t["flow"][:, mask].contiguous()               # row of rank r moves by the flow of the r-th set entry
    args = dict(t, flow=flow)
    tr = tracks.integrate(size=SIZE, motion_mask=mask, **args)
    # static rows: the projection of initial_pos in every view, a motion of exactly zero, where they were at the end
    still = tracks.integrate(size=SIZE, **dict(t, flow=torch.zeros_like(t["flow"])))
    assert same_bits(tr.xy[:, ~mask], still.xy[:, ~mask]) and same_bits(tr.step_ok[:, ~mask], still.step_ok[:, ~mask])
    assert bool((tr.motion[~mask] == 0).all()) and same_bits(tr.pos_last[~mask], t["initial_pos"][~mask])
    assert same_bits(tr.mean_z[~mask], still.mean_z[~mask])
    # dynamic rows: what they are without a mask
    free = tracks.integrate(size=SIZE, **t)
    for k in ("xy", "step_ok"):
        assert same_bits(getattr(tr, k)[:, mask], getattr(free, k)[:, mask]), k
    for k in ("pos_last", "motion", "mean_z"):
        assert same_bits(getattr(tr, k)[mask], getattr(free, k)[mask]), k
    assert bool((tr.motion[mask] > 0).all())
    # an all-true mask gives the bits of no mask; a DeformQuery the bits of its mask; a DeformQuery of no mask those too
    every = torch.ones(P, dtype=torch.bool, device=gpu)
    assert same_tracks(tracks.integrate(size=SIZE, motion_mask=every, **t), free)
    assert same_tracks(tracks.integrate(size=SIZE, motion_mask=DeformQuery(every), **t), free)
    assert same_tracks(tracks.integrate(size=SIZE, motion_mask=DeformQuery(None), **t), free)
    assert same_tracks(tracks.integrate(size=SIZE, motion_mask=DeformQuery(mask), **args), tr)
    # no dynamic row at all
    none = torch.zeros(P, dtype=torch.bool, device=gpu)
    assert same_tracks(tracks.integrate(size=SIZE, motion_mask=none, **dict(t, flow=t["flow"][:, :0].contiguous())), still)
    with pytest.raises(RuntimeError, match="the motion mask has %d set entries, flow has n = %d rows" % (n, P)):
        tracks.integrate(size=SIZE, motion_mask=DeformQuery(mask), **t)


@pytest.mark.gpu
def test_special_values_fault_nothing(gpu, golden):
    from gftorf_amd import tracks
    c = {k: np.array(v) for k, v in golden["p65"].items()}
    P, T, U = CASES["p65"]
    c["initial_pos"][3] = [0.1, 0.1, -2.0]              # behind every camera
    c["initial_pos"][4] = [np.inf, 0.0, 2.0]
    c["initial_pos"][5] = [0.0, -np.inf, 2.0]
    c["flow"][2, 7] = np.nan                            # frames 8..11 use row 2: a NaN from frame 9 on
    c["flow"][0, 8, 2] = np.inf
    tr = tracks.integrate(size=SIZE, **on(gpu, c))
    torch.cuda.synchronize()
    xy, ok = tr.xy.cpu().numpy(), tr.step_ok.cpu().numpy()
    assert np.array_equal(ok, step_ok_np(xy))
    assert np.isnan(xy[12:, 7]).all() and not ok[12:, 7].any() and np.isfinite(xy[:8, 7]).all()
    assert not ok[:, 4].any() and not ok[:, 5].any()
    assert np.isnan(tr.motion.cpu().numpy()[7]) and np.isinf(tr.motion.cpu().numpy()[8])
    # the rows around them are what they are without the special values
    clean = tracks.integrate(size=SIZE, **on(gpu, golden["p65"]))
    rest = torch.tensor([i for i in range(P) if i not in (3, 4, 5, 7, 8)], device=gpu)
    assert same_bits(tr.xy[:, rest], clean.xy[:, rest]) and same_bits(tr.step_ok[:, rest], clean.step_ok[:, rest])
    # an index outside the flow's rows is clamped, not followed
    wild = on(gpu, golden["p65"])
    wild["flow_index"] = torch.full((T,), 1 << 20, dtype=torch.int32, device=gpu)
    last = on(gpu, golden["p65"])
    last["flow_index"] = torch.full((T,), U - 1, dtype=torch.int32, device=gpu)
    assert same_tracks(tracks.integrate(size=SIZE, **wild), tracks.integrate(size=SIZE, **last))


@pytest.mark.gpu
@pytest.mark.parametrize("quantiles", QUANTILES)
def test_select_is_the_reference_statements(gpu, golden, quantiles):
    from gftorf_amd import tracks
    tr = tracks.integrate(size=SIZE, **on(gpu, golden["wide"]))
    opacity, scaling = torch.tensor(golden["select_opacity"], device=gpu), torch.tensor(golden["select_scaling"], device=gpu)
    big_motion_quantile, z_distr_quantile, opacity_quantile, small_size_quantile, big_size_quantile = quantiles
    # :278-290, with the two per-Gaussian means the kernel has formed
    motion, mean_z = tr.motion, tr.mean_z
    big_motion_threshold = torch.quantile(motion, big_motion_quantile)
    big_big_motion_threshold = torch.quantile(motion, 0.95)
    gs_sample_mask = (motion > big_motion_threshold)
    z_distr_threshold = torch.quantile(mean_z[gs_sample_mask], z_distr_quantile)
    gs_sample_mask *= (mean_z < z_distr_threshold)
    opacity_threshold = torch.quantile(opacity[gs_sample_mask], opacity_quantile)
    gs_sample_mask *= (opacity > opacity_threshold).squeeze()
    small_size_threshold = torch.quantile(torch.mean(scaling[gs_sample_mask], dim=-1), small_size_quantile)
    big_size_threshold = torch.quantile(torch.mean(scaling[gs_sample_mask], dim=-1), big_size_quantile)
    gs_sample_mask *= ((small_size_threshold < torch.mean(scaling, dim=-1)) * (torch.mean(scaling, dim=-1) < big_size_threshold)).squeeze()
    mask, threshold = tracks.select(tr, opacity, scaling, *quantiles)
    assert mask.dtype == torch.bool and mask.shape == (1000,) and torch.equal(mask, gs_sample_mask)
    assert threshold.dim() == 0 and threshold.device == motion.device and same_bits(threshold, big_big_motion_threshold)
    print("select %s: %d of 1000 drawn" % (quantiles, int(mask.sum())))
    assert 0 < int(mask.sum()) < 200
    again, _ = tracks.select(tr, opacity, scaling, big_motion_quantile=big_motion_quantile, z_distr_quantile=z_distr_quantile,
                             opacity_quantile=opacity_quantile, small_size_quantile=small_size_quantile, big_size_quantile=big_size_quantile)
    assert torch.equal(again, mask)


@pytest.mark.gpu
def test_table_gathers_the_selected_rows(gpu, golden):
    from gftorf_amd import tracks
    P, T, U = CASES["wide"]
    tr = tracks.integrate(size=SIZE, **on(gpu, golden["wide"]))
    g = torch.Generator().manual_seed(3)
    some = (torch.rand(P, generator=g) < 0.1).to(gpu)
    one = torch.zeros(P, dtype=torch.bool, device=gpu)
    one[777] = True
    for mask in (some, one, torch.zeros(P, dtype=torch.bool, device=gpu), torch.ones(P, dtype=torch.bool, device=gpu)):
        S = int(mask.sum())
        tab = tracks.table(tr, mask)
        assert (tab.S, tab.T, tab.size) == (S, T, SIZE) and tab.buffer.dtype == torch.uint8 and tab.buffer.is_contiguous()
        assert tab.buffer.numel() == tracks.table_layout(T, S)[0] == 8 * S + 8 * T * S + 4 * S + T * S
        assert tab.xy.shape == (T, S, 2) and tab.step_ok.shape == (T, S) and tab.motion.shape == (S,) and tab.index.shape == (S,)
        assert tab.index.dtype == torch.int64 and torch.equal(tab.index, torch.nonzero(mask).reshape(-1))
        assert same_bits(tab.xy, tr.xy[:, mask]) and same_bits(tab.step_ok, tr.step_ok[:, mask]) and same_bits(tab.motion, tr.motion[mask])
        host = tab.to_host()
        assert (host.T, host.S, host.size) == (T, S, SIZE)
        for k in ("xy", "step_ok", "motion", "index"):
            a, b = getattr(host, k), getattr(tab, k).cpu().numpy()
            assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=(k == "xy")), k
    with pytest.raises(RuntimeError, match=r"mask must be \[1000\]"):
        tracks.table(tr, torch.ones(999, dtype=torch.bool, device=gpu))
    # the host copy walks: the device's step_ok drives the loop as the comparisons on the host copy of xy do
    host = tracks.table(tr, some).to_host()
    want, _ = walk_reference(host.xy, host.motion, SIZE, lambda vid, i, x, y: True, 1)
    for (t_w, c_w), (_, t_g, c_g) in zip(want, tracks.walk(host)):
        assert t_w == t_g and c_w == c_g
    assert len(want[-1][0]) > 10


@pytest.mark.gpu
def test_integrate_reads_nothing_on_the_host_and_table_reads_once(gpu, golden):
    from gftorf_amd import DeformQuery, tracks
    P, T, U = CASES["wide"]
    t = on(gpu, golden["wide"])
    g = torch.Generator().manual_seed(3)
    mask = (torch.rand(P, generator=g) < 0.1).to(gpu)
    every = DeformQuery(torch.ones(P, dtype=torch.bool, device=gpu))
    tr = tracks.integrate(size=SIZE, **t)                 # warm-up: the library's first load is not the question
    tracks.table(tr, mask)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tr = tracks.integrate(size=SIZE, **t)
        tracks.integrate(size=SIZE, motion_mask=every, **t)
        with pytest.raises(RuntimeError):                 # the count of the selected rows
            tracks.table(tr, mask)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            tab = tracks.table(tr, mask)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert len(seen) == 1, [str(w.message) for w in seen]
    assert tab.S == int(mask.sum())


@pytest.mark.gpu
def test_captured_integrate_follows_new_positions(gpu, golden):
    from gftorf_amd import tracks
    t = on(gpu, golden["p257"])
    first = t["initial_pos"].clone()
    tracks.integrate(size=SIZE, **t)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tr = tracks.integrate(size=SIZE, **t)
    for shift in (0.05, -0.1):
        t["initial_pos"].copy_(first + shift)
        graph.replay()
        torch.cuda.synchronize()
        kept = types.SimpleNamespace(**{k: getattr(tr, k).clone() for k in ("xy", "pos_last", "motion", "mean_z", "step_ok")})
        eager = tracks.integrate(size=SIZE, **t)
        assert same_tracks(kept, eager)
        assert not same_bits(eager.xy, tracks.integrate(size=SIZE, **dict(t, initial_pos=first)).xy)


@pytest.mark.gpu
def test_sequence_flows_evaluates_each_distinct_time_once(gpu):
    from gftorf_amd import DeformNetwork, tracks
    torch.manual_seed(11)
    net = DeformNetwork(D=8, W=256, xyz_multires=10, t_multires=10, sh_degree=3).to(gpu)
    xyz = (torch.rand(300, 3) * 2 - 1).to(gpu)
    frame_ids, denom = list(range(12)), 59
    calls = []
    hook = net.register_forward_hook(lambda *a: calls.append(1))
    try:
        seq = tracks.sequence_flows(net, xyz, frame_ids, denom)
        mine = len(calls)

        def query_dmlp(fid):            # scene/gaussian_model.py:170-174 on the same module and rows
            t = torch.tensor(np.array([fid])).float().cuda().unsqueeze(0).expand(xyz.shape[0], -1)
            return net(xyz, t)

        with torch.no_grad():
            for t_, frame_id in enumerate(frame_ids):       # :223-228
                curr_int_fid = (frame_id // 4) * 4
                next_int_fid = (frame_id // 4 + 1) * 4
                d_xyz_curr, _, _, _ = query_dmlp(curr_int_fid / denom)
                d_xyz_next, _, _, _ = query_dmlp(next_int_fid / denom)
                d_xyz = 0.25 * ((frame_id - curr_int_fid) * d_xyz_next + (next_int_fid - frame_id) * d_xyz_curr)
                assert same_bits(seq.d_xyz(t_), d_xyz), t_
                assert same_bits(seq.flow[int(seq.flow_index[t_])], (d_xyz_next - d_xyz_curr) * 0.25), t_
    finally:
        hook.remove()
    U = int(seq.flow.shape[0])
    assert U == 3 and seq.flow.shape == (3, 300, 3) and seq.flow_index.dtype == torch.int32 and seq.flow_index.device == xyz.device
    assert seq.flow_index.tolist() == [0] * 4 + [1] * 4 + [2] * 4
    assert mine == seq.evaluations <= U + 1 and len(calls) - mine == 2 * len(frame_ids)
    assert not seq.flow.requires_grad and float(seq.flow.abs().max()) > 0
