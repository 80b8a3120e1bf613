"""gftorf_amd.present.debug_images: the debug images of the training loop's pipe.debug block, the ToF branch of train.py:295-378
(with :194-200 for the scattering phases; scene/torf_utils.py:11-29 to8b, normalize_im, normalize_im_gt; utils/graphics_utils.py:
117-137 phasor2real_img_amp; matplotlib's cm.magma).  The yardsticks are the reference's own bytes (tests/golden/
present_debug.npz, written by tests/golden/make_golden_present_debug.py from the block's statements in the block's order) and
`debug_np` below, the same statements restated in numpy float32.

Every statement of the block is an IEEE operation -- the two ToF depths are inputs, as train.py:188-189 leaves them -- so every
byte is required exactly, on every case.  The ranges follow line 317's zip: `amp` is normalised by the range of gt_reals,
`scattering_phase` by that of gt_imags, `scattering_phase_tof_depth` by that of gt_amps; only `scattering_phase_gt` (line 323) has
gt_scattering_phases'.  The fixture's ranges really come from lists of three views.

Two pixels of `ragged` carry a NaN into an unnormalised to8b (the NaN of `depth` into scattering_phase_error, the NaN of
gt_quad[quad_index] into quad_gt): numpy's cast of a NaN to uint8 is what the platform makes of it, and the fixture holds what
numpy on x86-64 gave, 0, which is also what include/gftorf_present.h's to8b defines.  The generator asserts it.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_debugviz.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "present_debug.npz")
IMAGES = ("depth", "amp", "amp_error", "scattering_phase", "scattering_phase_error", "scattering_phase_tof_depth",
          "scattering_phase_tof_depth_error", "scattering_phase_gt", "depth_error", "phase_depth", "phase_depth_gt", "phase_depth_error",
          "color", "color_gt", "color_error", "dd", "quad", "quad_gt", "quad_error")
BPP = dict(zip(IMAGES, (4, 1, 1, 1, 1, 1, 1, 1, 1, 4, 4, 1, 3, 3, 3, 1, 4, 4, 4)))
SELFNORM = ("amp_error", "depth_error", "phase_depth_error", "dd", "quad_error")
P, GP, D, PD, GPD, DD, C, Q, GQ = (1 << k for k in range(9))
NEEDS = dict(zip(IMAGES, (D, P, P | GP, P | D, P | D | GP | GPD, P | PD, P | PD | GP | GPD, GP | GPD, GPD | D, PD, GPD, GPD | PD, C, C, C, DD,
                          Q, GQ, GQ)))
TENSORS = ("phasor", "gt_phasor", "depth", "phase_depth", "gt_phase_depth", "dd", "image", "gt_image", "gt_quad")
RUN_PIXELS = 1024                       # pixels of one workgroup's run: 256 lanes of 4
# name: (H, W, permutation, quad_index, kind)
CASES = {"one": (1, 1, (0, 1, 2, 3), 0, "plain"), "small": (7, 13, (1, 0, 3, 2), 1, "plain"), "ragged": (37, 53, (2, 0, 3, 1), 3, "ragged"),
         "flat": (7, 13, (1, 0, 3, 2), 2, "flat")}
DEPTH_RANGE, PHASE_OFFSET, MULT = 7.5, 0.3, 2.0


# ---- the restatement -----------------------------------------------------------------------------------------------------

def zplanes_np(depth_range):
    """train.py:297 with the camera's 0-d float32 depth_range (numpy >= 2 keeps the products float32)"""
    r = np.array(depth_range, dtype=np.float32)
    return 0.05 * r * 0.9, 0.55 * r * 1.1


def to8b_np(x):
    """torf_utils.py:11-12; a NaN gives 0"""
    with np.errstate(invalid="ignore"):
        y = 255 * np.clip(x, 0, 1)
        return np.where(np.isnan(y), np.float32(0), y).astype(np.uint8)


def normalize_np(im, lo, hi):
    """torf_utils.py:21-29 with the bounds given: float32 throughout"""
    assert im.dtype == np.float32
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        im = (im - np.float32(lo)) / (np.float32(hi) - np.float32(lo))
    im[np.isnan(im)] = 0.
    return np.clip(im, 0, 1)


def selfnorm_np(im):
    """torf_utils.py:21-24: np.min and np.max propagate a NaN"""
    with np.errstate(invalid="ignore"):
        return normalize_np(im, np.min(im), np.max(im))


def magma_np(table, d, znear, zfar):
    """to8b(cm.magma(1 - (d - znear) / (zfar - znear))) through the 257 x 4 table: matplotlib's index of a float32 is
    trunc(x * 256), below 0 the first entry, from 256 on (x == 1 too) the last, a NaN row 256"""
    assert d.dtype == np.float32
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = 1 - (d - np.float32(znear)) / (np.float32(zfar) - np.float32(znear))
        s = x * np.float32(256)
        row = np.where(np.isnan(x), 256, np.where(x < 0, 0, np.where(s >= 256, 255, np.trunc(s))))
    return table[row.astype(np.int64)]


def debug_np(v, table):
    """train.py:295-378 (ToF branch) for the inputs `v` holds: {image name: uint8 array}"""
    has = lambda *keys: all(k in v for k in keys)
    out = {}
    with np.errstate(invalid="ignore", over="ignore"):
        if has("phasor"):
            amp = v["phasor"][2] * np.float32(v["tof_multiplier"])                             # :311
        if has("gt_phasor"):
            gt_amp = v["gt_phasor"][2]                                                        # :312
        if has("gt_phasor", "gt_phase_depth"):
            gt_sp = gt_amp * (v["gt_phase_depth"] * v["gt_phase_depth"])                      # :196
        r = [np.float32(x) for x in v["ranges"]] if "ranges" in v else None
        if has("depth"):
            out["depth"] = magma_np(table, v["depth"][0], v["znear"], v["zfar"])              # :297-298
        if has("phasor"):
            out["amp"] = to8b_np(normalize_np(amp, r[0], r[1]))                               # :318, gt_reals
        if has("phasor", "gt_phasor"):
            out["amp_error"] = to8b_np(selfnorm_np(np.abs(gt_amp - amp)))                     # :313-314, 319
        if has("phasor", "depth"):
            sp = amp * (v["depth"][0] * v["depth"][0])                                        # :197
            out["scattering_phase"] = to8b_np(normalize_np(sp, r[2], r[3]))                   # :318, gt_imags
            if has("gt_phasor", "gt_phase_depth"):
                out["scattering_phase_error"] = to8b_np(np.abs(gt_sp - sp))                   # :199, 319
        if has("phasor", "phase_depth"):
            sp_tof = amp * (v["phase_depth"] * v["phase_depth"])                              # :198
            out["scattering_phase_tof_depth"] = to8b_np(normalize_np(sp_tof, r[4], r[5]))     # :318, gt_amps
            if has("gt_phasor", "gt_phase_depth"):
                out["scattering_phase_tof_depth_error"] = to8b_np(np.abs(gt_sp - sp_tof))     # :200, 319
        if has("gt_phasor", "gt_phase_depth"):
            out["scattering_phase_gt"] = to8b_np(normalize_np(gt_sp, r[6], r[7]))             # :323
        if has("gt_phase_depth", "depth"):
            out["depth_error"] = to8b_np(selfnorm_np(np.abs(v["gt_phase_depth"] - v["depth"][0])))         # :325-327
        if has("phase_depth"):
            out["phase_depth"] = magma_np(table, v["phase_depth"], v["znear"], v["zfar"])     # :332, 334
        if has("gt_phase_depth"):
            out["phase_depth_gt"] = magma_np(table, v["gt_phase_depth"], v["znear"], v["zfar"])            # :333, 335
        if has("gt_phase_depth", "phase_depth"):
            out["phase_depth_error"] = to8b_np(selfnorm_np(np.abs(v["gt_phase_depth"] - v["phase_depth"])))  # :337-338
        if has("image", "gt_image"):
            im, gt = v["image"].transpose(1, 2, 0), v["gt_image"].transpose(1, 2, 0)
            out["color"], out["color_gt"], out["color_error"] = to8b_np(im), to8b_np(gt), to8b_np(np.abs(gt - im))   # :359-364
        if has("dd"):
            out["dd"] = to8b_np(selfnorm_np(v["dd"][0]))                                      # :366-367
        if has("phasor") and v["phasor"].shape[0] == 7:
            quads = v["phasor"][3:]
            out["quad"] = np.stack([to8b_np(np.abs(quads[i])) for i in range(4)])             # :372
            if has("gt_quad"):
                perm, qi = [int(k) for k in v["permutation"]], int(v["quad_index"])
                out["quad_gt"] = np.stack([to8b_np(np.abs(v["gt_quad"][perm[i]])) for i in range(4)])          # :378
                out["quad_error"] = np.stack([to8b_np(selfnorm_np(np.abs(quads[i] - v["gt_quad"][perm[i]]))) if perm[i] == qi
                                              else np.zeros(quads[i].shape, np.uint8) for i in range(4)])     # :373-377
    return {k: out[k] for k in IMAGES if k in out}


def red_blue_np(plane):
    """graphics_utils.py:125-137 for one [H, W] plane: the positive part in red, nothing in green, the negated negative part in blue"""
    zero = np.zeros_like(plane)
    return np.stack([np.where(plane <= 0, zero, plane), zero, -np.where(plane >= 0, zero, plane)], axis=-1)


def depth_from_tof_np(tof, depth_range, phase_offset):
    """torf_utils.py:53-57 on [3, H, W], float32"""
    phase = np.arctan2(tof[1], tof[0]) - np.float32(phase_offset)
    phase = np.where(phase < 0, phase + np.float32(2 * np.pi), phase)
    return phase * np.float32(depth_range) / np.float32(4 * np.pi)


def ranges_np(views, depth_range, phase_offset):
    """train.py:57-64: np.min / np.max over the training views of gt_reals, gt_imags, gt_amps and gt_scattering_phases.  The
    last pair hangs on numpy's arctan2; it stays on the host and is an input of debug_images."""
    reals, imags, amps = [red_blue_np(g[0]) for g in views], [red_blue_np(g[1]) for g in views], [g[2] for g in views]
    sps = [g[2] * depth_from_tof_np(g, depth_range, phase_offset) ** 2 for g in views]
    return np.array([f(seq) for seq in (reals, imags, amps, sps) for f in (np.min, np.max)], np.float32)


def tof_depth_np(tof, depth_range, phase_offset):
    """torf_utils.py:59-64 (depth_from_tof_torch, with its 1e-6 guard) in numpy float32: the ToF depths of a case the tests
    draw themselves.  They are inputs of the block either way; the fixture's come from the reference's torch function."""
    re = np.where(np.abs(tof[0]) < 1e-6, np.float32(1e-6), tof[0])
    phase = np.arctan2(tof[1], re) - np.float32(phase_offset)
    phase = np.where(phase < 0, phase + np.float32(2 * np.pi), phase)
    return (phase * np.float32(depth_range) / np.float32(4 * np.pi)).astype(np.float32)


# ---- inputs --------------------------------------------------------------------------------------------------------------

SPECIALS = 11           # pixels of a ragged case that carry a special value


def draw_debug(rng, H, W, perm, qi, kind, tof_depth=tof_depth_np):
    """One iteration's inputs as the `.cpu()` copies hold them, float32: a rendered view near its ground truth, so the errors
    are not all saturated.  `kind` "ragged" places the special values of the module's fixture notes and makes gt_amps constant
    (a range with hi == lo); "flat" makes every self-normalised plane constant and amp_error identically 0."""
    f32 = np.float32
    dr = np.array(DEPTH_RANGE, f32)
    views = []
    for _ in range(3):
        theta = rng.uniform(0.05, 2 * np.pi - 0.05, (H, W)) + PHASE_OFFSET
        length = rng.uniform(0.05, 1.0, (H, W))
        amp = np.full((H, W), 0.25) if kind == "ragged" else rng.uniform(0.02, 0.3, (H, W))
        if kind == "flat":
            amp = rng.integers(2, 20, (H, W)) / 64
        views.append(np.stack([length * np.cos(theta), length * np.sin(theta), amp]).astype(f32))
    gt = views[0]
    gt_quad = rng.uniform(-1, 1, (4, H, W)).astype(f32)
    phasor = np.empty((7, H, W), f32)
    phasor[:2] = gt[:2] * (1 + 0.05 * rng.normal(size=(2, H, W))) / MULT
    phasor[2] = gt[2] / MULT * (1 + 0.1 * rng.normal(size=(H, W)))
    phasor[3:] = gt_quad[list(perm)] + 0.1 * rng.normal(size=(4, H, W))
    gpd = np.asarray(tof_depth(gt, DEPTH_RANGE, PHASE_OFFSET), f32)
    pd = np.asarray(tof_depth(phasor[:3], DEPTH_RANGE, PHASE_OFFSET), f32)
    depth = (gpd * (1 + 0.03 * rng.normal(size=(H, W))))[None].astype(f32)
    dd = rng.uniform(0, 0.2, (1, H, W)).astype(f32)
    gt_image = rng.uniform(0, 1, (3, H, W)).astype(f32)
    image = (gt_image + 0.1 * rng.normal(size=(3, H, W))).astype(f32)
    if kind == "flat":                  # exact in float32: eighths and sixty-fourths
        gpd = (rng.integers(4, 29, (H, W)) / 8).astype(f32)
        depth, pd = (gpd + f32(0.5))[None], gpd - f32(0.25)
        phasor[2] = gt[2] / f32(MULT)
        dd[:] = 0.7
        gt_quad = (rng.integers(-64, 65, (4, H, W)) / 64).astype(f32)
        phasor[3:] = gt_quad[list(perm)] + f32(0.125)
    if kind == "ragged":
        at = [np.unravel_index(k, (H, W)) for k in rng.permutation(H * W)[:SPECIALS]]
        nan, inf = f32(np.nan), f32(np.inf)
        depth[0][at[0]] = nan                                   # zeroes depth_error; scattering_phase_error's cast, see the docstring
        dd[0][at[1]] = nan                                      # zeroes dd
        gt_quad[qi][at[2]] = nan                                # zeroes the shown plane of quad_error; quad_gt's cast
        pd[at[3]] = inf                                         # zeroes phase_depth_error
        dd[0][at[4]], image[0][at[4]], phasor[4][at[4]] = f32(-0.0), f32(-0.0), f32(-0.0)
        phasor[2][at[5]], phasor[2][at[6]] = 5.0, -0.5          # amp, sp and sp_tof above hi and below lo
        gpd[at[7]], gpd[at[8]] = 50.0, 0.0                      # gt_sp above hi and below lo
        depth[0][at[9]], depth[0][at[10]] = 0.01, 100.0         # nearer than znear, farther than zfar
    znear, zfar = zplanes_np(dr)
    v = dict(phasor=phasor, gt_phasor=gt, depth=depth, phase_depth=pd, gt_phase_depth=gpd, dd=dd, image=image, gt_image=gt_image,
             gt_quad=gt_quad, permutation=np.array(perm, np.int32), quad_index=np.int32(qi), ranges=ranges_np(views, DEPTH_RANGE, PHASE_OFFSET),
             znear=znear, zfar=zfar, tof_multiplier=f32(MULT))
    return v, np.stack(views)


def subset(v, *names):
    """`v` with only the tensors named (and every scalar)"""
    return {k: a for k, a in v.items() if k not in TENSORS or k in names}


def groups_of(v):
    g = sum(bit for bit, k in ((P, "phasor"), (GP, "gt_phasor"), (D, "depth"), (PD, "phase_depth"), (GPD, "gt_phase_depth"), (DD, "dd"),
                               (C, "image"), (GQ, "gt_quad")) if k in v)
    return g | (Q if "phasor" in v and v["phasor"].shape[0] == 7 else 0)


@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    out = {c: {k[len(c) + 1:]: z[k] for k in z.files if k.startswith(c + "_")} for c in CASES}
    out["magma_u8"], out["numpy"] = z["magma_u8"], str(z["numpy"])
    for g in out.values():
        if isinstance(g, dict):
            for a in g.values():
                a.setflags(write=False)
    return out


def golden_inputs(g):
    return {k: g[k] for k in TENSORS + ("permutation", "quad_index", "ranges", "znear", "zfar", "tof_multiplier")}


_NP = {}


def restated(case, golden):
    """`debug_np` of a fixture case, computed once and shared"""
    if case not in _NP:
        _NP[case] = debug_np(golden_inputs(golden[case]), golden["magma_u8"])
    return _NP[case]


def check_images(got, want, what):
    """device images (tensors or arrays) against the expected ones: the same keys in the same order, every byte; prints first"""
    assert list(got) == list(want), (what, list(got), list(want))
    for k, w in want.items():
        have = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        assert have.shape == w.shape and have.dtype == np.uint8, (what, k, have.shape, have.dtype)
        bad = np.argwhere(have != w)
        print("%s %s: %d of %d bytes differ" % (what, k, len(bad), w.size))
        assert not len(bad), (what, k, len(bad), bad[:4].tolist(), have[tuple(bad[0])], w[tuple(bad[0])])


# ---- CPU-runnable checks -------------------------------------------------------------------------------------------------

def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c_and_every_symbol_is_exported(tmp_path, lib):
    from gftorf_amd import _lib, build, present
    names = declared_functions()
    assert set(names) == set(_lib.DEBUGVIZ_EXPORTS) == {"gft_debugviz_blocks", "gft_debugviz_sheet_bytes", "gft_debugviz_images"}, names
    others = [t for t in dir(_lib) if t.endswith("EXPORTS") and t != "DEBUGVIZ_EXPORTS"]
    assert len(others) >= 12 and "PRESENT_EXPORTS" in others and "FLOWVIZ_EXPORTS" in others
    for t in others:
        assert not set(names) & set(getattr(_lib, t)), t
    for n in names:
        assert hasattr(lib, n), n
    assert "k_debugviz.hip" in build.SOURCES and callable(present.debug_images) and callable(present.ViewSheets.submit_debug)
    assert "struct" not in re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    prog = tmp_path / "debugviz_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_debugviz.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "debugviz_abi.o")])
    words = ["GFT_DEBUGVIZ_IMAGES", "GFT_DEBUGVIZ_ALIGN", "GFT_DEBUGVIZ_PARTIAL_WORDS", "GFT_DEBUGVIZ_RANGE_WORDS", "GFT_DEBUGVIZ_RUN"]
    words += ["GFT_DEBUGVIZ_HAS_" + n for n in ("PHASOR", "GT_PHASOR", "DEPTH", "PHASE_DEPTH", "GT_PHASE_DEPTH", "DD", "COLOR", "QUAD", "GT_QUAD")]
    out = subprocess.check_output(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-include", "gftorf_debugviz.h",
                                   "-x", "c", "-"], input="DEBUGVIZ_WORDS_ARE %s\n" % " ".join(words), text=True)
    consts = [int(x) for x in out.split("DEBUGVIZ_WORDS_ARE", 1)[1].split()]
    assert consts == [len(_lib.DEBUGVIZ_IMAGES), _lib.DEBUGVIZ_ALIGN, _lib.DEBUGVIZ_PARTIAL_WORDS, _lib.DEBUGVIZ_RANGE_WORDS, _lib.DEBUGVIZ_RUN,
                      P, GP, D, PD, GPD, DD, C, Q, GQ] == [19, 16, 16, 8, 4, 1, 2, 4, 8, 16, 32, 64, 128, 256]
    assert (_lib.DEBUGVIZ_HAS_PHASOR, _lib.DEBUGVIZ_HAS_GT_PHASOR, _lib.DEBUGVIZ_HAS_DEPTH, _lib.DEBUGVIZ_HAS_PHASE_DEPTH,
            _lib.DEBUGVIZ_HAS_GT_PHASE_DEPTH, _lib.DEBUGVIZ_HAS_DD, _lib.DEBUGVIZ_HAS_COLOR, _lib.DEBUGVIZ_HAS_QUAD,
            _lib.DEBUGVIZ_HAS_GT_QUAD) == (P, GP, D, PD, GPD, DD, C, Q, GQ)
    # the image indices of the header are the order of the Python table
    src = open(HEADER).read()
    index = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define GFT_DEBUGVIZ_([A-Z_]+) (\d+)\n", src)
             if not m.group(1).startswith("HAS_")}
    short = {"scattering_phase": "sp", "scattering_phase_error": "sp_error", "scattering_phase_tof_depth": "sp_tof",
             "scattering_phase_tof_depth_error": "sp_tof_error", "scattering_phase_gt": "sp_gt"}
    assert [index[short.get(k, k)] for k in IMAGES] == list(range(19))
    assert tuple(n for n, _, _ in _lib.DEBUGVIZ_IMAGES) == IMAGES == present.DEBUG_IMAGES
    assert [b for _, b, _ in _lib.DEBUGVIZ_IMAGES] == [BPP[k] for k in IMAGES] and sum(BPP.values()) == 43
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16


def test_the_numpy_statements_give_the_reference_bytes(golden):
    """`debug_np` against what the reference's own statements wrote into the fixture, every byte of every image; and the
    fixture holds the cases and special values it is meant to"""
    assert int(golden["numpy"].split(".")[0]) >= 2, golden["numpy"]
    table = golden["magma_u8"]
    assert table.shape == (257, 4) and table.dtype == np.uint8
    for c, (H, W, perm, qi, kind) in CASES.items():
        g = golden[c]
        v = golden_inputs(g)
        assert v["phasor"].shape == (7, H, W) and v["gt_phasor"].shape == (3, H, W) and v["depth"].shape == v["dd"].shape == (1, H, W), c
        assert v["phase_depth"].shape == v["gt_phase_depth"].shape == (H, W) and v["gt_quad"].shape == (4, H, W), c
        assert v["image"].shape == v["gt_image"].shape == (3, H, W) and all(v[k].dtype == np.float32 for k in TENSORS), c
        assert tuple(v["permutation"]) == perm and int(v["quad_index"]) == qi and sorted(perm) == [0, 1, 2, 3]
        zn, zf = zplanes_np(g["depth_range"])
        assert zn.dtype == np.float32 and zn == v["znear"] and zf == v["zfar"]
        got = restated(c, golden)
        assert list(got) == list(IMAGES)
        for k in IMAGES:
            want = g["out_" + k]
            assert want.dtype == np.uint8 and got[k].shape == want.shape, (c, k)
            assert np.array_equal(got[k], want), (c, k, np.argwhere(got[k] != want)[:4].tolist())
        # the ranges come from lists of three views, the first of them this iteration's; the first six are IEEE statements
        views = g["gt_views"]
        assert views.shape == (3, 3, H, W) and np.array_equal(views[0], v["gt_phasor"])
        r = ranges_np(list(views), g["depth_range"], g["phase_offset"])
        assert np.array_equal(r[:6], v["ranges"][:6]) and np.allclose(r[6:], v["ranges"][6:], rtol=1e-4) and v["ranges"].shape == (8,)
    one, flat, rag = golden["one"], golden["flat"], golden["ragged"]
    assert all(not one["out_" + k].any() for k in SELFNORM)                  # max == min
    # flat: every self-normalised plane is constant, so all 0; amp_error's plane is identically 0
    f = golden_inputs(flat)
    amp = f["phasor"][2] * np.float32(MULT)
    assert not (f["gt_phasor"][2] - amp).any()
    for plane in (np.abs(f["gt_phase_depth"] - f["depth"][0]), np.abs(f["gt_phase_depth"] - f["phase_depth"]), f["dd"][0],
                  np.abs(f["phasor"][3:] - f["gt_quad"][list(CASES["flat"][2])])):
        assert plane.min() == plane.max() != 0
    assert all(not flat["out_" + k].any() for k in SELFNORM)
    assert golden["small"]["out_amp_error"].max() == 255 and golden["small"]["out_quad_error"].max() == 255
    # ragged: the special values, and what each does
    v = golden_inputs(rag)
    qi, perm = int(v["quad_index"]), list(v["permutation"])
    assert np.isnan(v["depth"]).sum() == np.isnan(v["dd"]).sum() == np.isnan(v["gt_quad"]).sum() == np.isnan(v["gt_quad"][qi]).sum() == 1
    assert not any(np.isnan(v[k]).any() for k in TENSORS if k not in ("depth", "dd", "gt_quad"))
    assert np.isposinf(v["phase_depth"]).sum() == 1 and not any(np.isinf(v[k]).any() for k in TENSORS if k != "phase_depth")
    for k in ("depth_error", "dd", "quad_error", "phase_depth_error"):
        assert not rag["out_" + k].any(), k
    assert rag["out_amp_error"].max() == 255 and rag["out_depth"][np.isnan(v["depth"][0])].tolist() == [table[256].tolist()]
    for k in ("dd", "image", "phasor"):
        assert ((v[k] == 0) & np.signbit(v[k])).any(), k
    r = v["ranges"]
    amp = v["phasor"][2] * np.float32(MULT)
    with np.errstate(invalid="ignore"):
        planes = (amp, amp * v["depth"][0] ** 2, amp * v["phase_depth"] ** 2, v["gt_phasor"][2] * v["gt_phase_depth"] ** 2)
        for k, plane in enumerate(planes):
            assert (plane < r[2 * k]).any() and (plane > r[2 * k + 1]).any(), k
    assert r[4] == r[5] and r[0] < r[1] and r[2] < r[3] and r[6] < r[7]
    assert (v["depth"] < v["znear"]).any() and (v["depth"] > v["zfar"]).any()
    assert (rag["out_depth"] == table[255]).all(-1).any() and (rag["out_depth"] == table[0]).all(-1).any()
    # the two casts of the module docstring gave 0
    assert rag["out_scattering_phase_error"][np.isnan(v["depth"][0])].tolist() == [0]
    assert rag["out_quad_gt"][perm.index(qi)][np.isnan(v["gt_quad"][qi])].tolist() == [0]


def test_the_sheet_layout_of_every_combination_of_groups(lib):
    from gftorf_amd import present
    seen = 0
    for H, W in ((1, 1), (7, 13), (37, 53)):
        n = H * W
        for groups in range(1, 512):
            valid = not (groups & Q and not groups & P) and not (groups & GQ and not groups & Q)
            names = [k for k in IMAGES if groups & NEEDS[k] == NEEDS[k]] if valid else []
            if not names:
                assert lib.gft_debugviz_sheet_bytes(H, W, groups, None) == 0, groups
                with pytest.raises(ValueError, match="no debug sheet"):
                    present.debug_sheet_layout(H, W, groups)
                continue
            total, offsets = present.debug_sheet_layout(H, W, groups)
            assert list(offsets) == names, groups
            end = 0
            for k in names:                                       # in order, aligned, no overlap
                assert offsets[k] % 16 == 0 and offsets[k] == -(-end // 16) * 16, (groups, k)
                end = offsets[k] + BPP[k] * n
            assert total == -(-end // 16) * 16, groups
            seen += 1
    assert seen > 3 * 200
    every = present.debug_sheet_layout(480, 640, 511)
    assert list(every[1]) == list(IMAGES) and every[0] == 43 * 480 * 640
    for bad in ((0, 5, 511), (5, 0, 511), (-1, 5, 511), (5, 5, 0), (5, 5, 512), (5, 5, -1), (5, 5, GP), (5, 5, GP | Q), (5, 5, P | GQ)):
        assert lib.gft_debugviz_sheet_bytes(*bad, None) == 0, bad
        with pytest.raises(ValueError, match="no debug sheet"):
            present.debug_sheet_layout(*bad)


def test_blocks_and_c_argument_checks(lib):
    import ctypes as C
    from gftorf_amd import _lib, present
    assert present.debug_blocks(0) == 0 and lib.gft_debugviz_blocks(-5) == 0
    assert [present.debug_blocks(n) for n in (1, 1024, 1025, 2048, 2049, 1 << 30)] == [1, 1, 2, 2, 3, 512]
    counts = [present.debug_blocks(n) for n in range(0, 5000, 7)]
    assert counts == sorted(counts)
    assert present.debug_blocks(three_block_shape()[0] * three_block_shape()[1]) == 3
    x, perm, rg = C.c_void_p(256), (C.c_int32 * 4)(0, 1, 2, 3), (C.c_float * 8)()     # never dereferenced: the calls fail before any launch

    def call(H=4, W=4, ph=x, ps=16, planes=7, gph=x, gps=16, d=x, pd=x, gpd=x, dd=x, im=x, ims=16, gim=x, gims=16, gq=x, gqs=16, perm=perm,
             rg=rg, part=x, sheet=x):
        return lib.gft_debugviz_images(None, H, W, ph, ps, planes, gph, gps, d, pd, gpd, dd, im, ims, gim, gims, gq, gqs, perm, None, 0,
                                       None, rg, 0.3, 4.5, 1.0, part, sheet)
    for bad, msg in ((dict(H=0), "bad size"), (dict(W=-1), "bad size"), (dict(planes=2), "at least 3 planes"), (dict(ph=None), "0 are given without one"),
                     (dict(im=None), "given together"), (dict(gim=None), "given together"), (dict(planes=3), "exactly 7 planes"),
                     (dict(ps=-1), "bad plane stride"), (dict(gqs=-4), "bad plane stride"), (dict(sheet=None), "sheet is NULL"),
                     (dict(sheet=C.c_void_p(264)), "16-byte aligned"), (dict(rg=None), "need ranges"), (dict(part=None), "need partials"),
                     (dict(part=C.c_void_p(260)), "need partials"), (dict(perm=None), "needs a permutation"),
                     (dict(perm=(C.c_int32 * 4)(0, 1, 4, 3)), r"permutation[2]=4"), (dict(perm=(C.c_int32 * 4)(-1, 1, 2, 3)), r"permutation[0]=-1"),
                     (dict(ph=None, planes=0, gq=None, d=None, pd=None, gpd=None, dd=None, im=None, gim=None), "produce no image")):
        assert call(**bad) != 0, bad
        assert msg in _lib.last_error(), (bad, _lib.last_error())


def test_wrapper_rejects_bad_arguments_before_any_launch(lib, monkeypatch):
    """every validation error names its argument and comes before the library is asked to launch; on CPU tensors the shapes,
    the pairs, the permutation and the ranges are judged first, then the device"""
    from gftorf_amd import present
    v, _ = draw_debug(np.random.default_rng(5), 4, 6, (1, 0, 3, 2), 1, "plain")
    t = {k: torch.tensor(v[k]) for k in TENSORS}
    kw = dict(t, permutation=(1, 0, 3, 2), quad_index=1, ranges=v["ranges"], zplanes=(0.3, 4.5), tof_multiplier=2.0)

    class NoLaunch:
        def __getattr__(self, name):
            assert name != "gft_debugviz_images", name
            return getattr(lib, name)
    monkeypatch.setattr(present._lib, "load", lambda: NoLaunch())

    def call(**over):
        return present.debug_images(**{k: a for k, a in dict(kw, **over).items() if a is not None or k in ("ranges", "zplanes", "quad_index")})
    with pytest.raises(RuntimeError, match="phasor is on cpu; the display kernels run on a HIP device only, there is no CPU path"):
        call()
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        present.ViewSheets(slots=1).submit_debug(0, **kw)
    for over, msg in [(dict(phasor=t["phasor"][:2]), r"phasor must be \[>=3, H, W\], got \[2, 4, 6\]"),
                      (dict(phasor=t["phasor"][0]), r"phasor must be \[>=3, H, W\]"),
                      (dict(gt_phasor=t["gt_phasor"][:, :3]), "gt_phasor is 3 x 6, phasor 4 x 6: the inputs of one call have one size"),
                      (dict(depth=t["depth"][0]), r"depth must be \[1, H, W\], got \[4, 6\]"),
                      (dict(depth=t["image"]), r"depth must be \[1, H, W\], got \[3, 4, 6\]"),
                      (dict(phase_depth=t["depth"]), r"phase_depth must be \[H, W\], got \[1, 4, 6\]"),
                      (dict(gt_phase_depth=t["gt_phase_depth"][:, :5]), "gt_phase_depth is 4 x 5, phasor 4 x 6"),
                      (dict(dd=t["image"]), r"dd must be \[1, H, W\]"),
                      (dict(image=t["image"][:2], gt_image=t["gt_image"]), r"image must be \[3, H, W\], got \[2, 4, 6\]"),
                      (dict(gt_image=t["gt_image"][:, :, :5]), "gt_image is 4 x 5, phasor 4 x 6"),
                      (dict(gt_quad=t["gt_quad"][:3]), r"gt_quad must be \[4, H, W\], got \[3, 4, 6\]"),
                      (dict(phasor=t["phasor"][:3]), r"gt_quad needs a phasor of exactly 7 planes, got \[3, 4, 6\]"),
                      (dict(ranges=v["ranges"][:6]), "ranges must be eight numbers or a contiguous tensor \\[8\\], got 6 numbers"),
                      (dict(ranges=torch.zeros(6)), r"ranges must be eight numbers or a contiguous tensor \[8\], got \[6\]"),
                      (dict(ranges=torch.zeros(16)[::2]), r"ranges must be eight numbers or a contiguous tensor \[8\]"),
                      (dict(quad_index=torch.zeros(2, dtype=torch.int32)), "quad_index must be an integer or a one-element tensor")]:
        with pytest.raises(RuntimeError, match=msg):
            call(**over)
    for over, msg in [(dict(gt_image=None), "image and gt_image are given together, got only image"),
                      (dict(image=None), "image and gt_image are given together, got only gt_image"),
                      (dict(permutation=(0, 1, 2, 4)), r"permutation must be four integers in 0..3, got \[0, 1, 2, 4\]"),
                      (dict(permutation=(-1, 1, 2, 3)), "permutation must be four integers in 0..3"),
                      (dict(permutation=(0, 1, 2)), "permutation must be four integers in 0..3"),
                      (dict(quad_index=None), "needs quad_index"), (dict(ranges=None), "need ranges"), (dict(zplanes=None), "needs zplanes")]:
        with pytest.raises(ValueError, match=msg):
            call(**over)
    for over, msg in [(dict(phasor=v["phasor"]), "phasor must be a tensor"), (dict(depth=t["depth"].double()), "depth must be torch.float32"),
                      (dict(phase_depth=t["phase_depth"].half()), "phase_depth must be torch.float32"),
                      (dict(permutation=5), "permutation must be four integers"), (dict(ranges=torch.zeros(8).double()), "ranges must be torch.float32"),
                      (dict(quad_index=torch.zeros(1)), "quad_index must be torch.int32")]:
        with pytest.raises(TypeError, match=msg):
            call(**over)
    with pytest.raises(ValueError, match="nothing to show"):
        present.debug_images(ranges=v["ranges"], zplanes=(0.3, 4.5))
    with pytest.raises(ValueError, match="no debug sheet"):
        present.debug_images(gt_phasor=t["gt_phasor"])
    with pytest.raises(ValueError, match="nothing to show"):
        present.ViewSheets(slots=1).submit_debug(0, ranges=v["ranges"])


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def three_block_shape():
    """(H, W) of the smallest frame that spans three workgroups of launch 1 with H * W % 4 == 1 and an odd width"""
    from gftorf_amd import present
    n = 1
    while True:
        if present.debug_blocks(n) >= 3 and n % 4 == 1:
            H = next((h for h in range(2, 64) if n % h == 0 and (n // h) % 2 == 1), None)
            if H is not None:
                return H, n // H
        n += 1


def on(dev, a):
    return torch.tensor(np.ascontiguousarray(a), device=dev)


def kwargs_on(dev, v, **over):
    kw = {k: on(dev, v[k]) for k in TENSORS if k in v}
    kw.update(ranges=v["ranges"], zplanes=(float(v["znear"]), float(v["zfar"])), tof_multiplier=float(v["tof_multiplier"]))
    if "gt_quad" in v:
        kw.update(permutation=tuple(int(k) for k in v["permutation"]), quad_index=int(v["quad_index"]))
    kw.update(over)
    return kw


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_debug_images_are_the_reference_bytes(case, gpu, golden):
    """every fixture case: every byte of every image, views into one sheet on 16-byte boundaries, the inputs untouched"""
    from gftorf_amd import present
    g = golden[case]
    H, W = CASES[case][:2]
    v = golden_inputs(g)
    kw = kwargs_on(gpu, v)
    got = present.debug_images(**kw)
    want = {k: g["out_" + k] for k in IMAGES}
    check_images(got, want, case)
    total, offsets = present.debug_sheet_layout(H, W, 511)
    base = got["depth"].data_ptr()
    assert base % 16 == 0 and [t.data_ptr() - base for t in got.values()] == [offsets[k] for k in IMAGES]
    assert all(t.dtype == torch.uint8 and t.device == gpu for t in got.values())
    for k in TENSORS:
        assert np.array_equal(kw[k].cpu().numpy().view(np.uint32), v[k].view(np.uint32)), k


@pytest.mark.gpu
def test_three_workgroups_match_the_numpy_statements(gpu, golden):
    """the smallest frame over three workgroups, H * W % 4 == 1, an odd width: against the restatement, specials placed; two runs
    are bit-equal and write every word of the partials"""
    from gftorf_amd import _lib, present
    H, W = three_block_shape()
    assert (H * W) % 4 == 1 and W % 2 == 1 and present.debug_blocks(H * W) == 3 and present.debug_blocks(H * W - 4) == 2
    assert -(-H * W // RUN_PIXELS) == 3
    v, _ = draw_debug(np.random.default_rng(20261021), H, W, (3, 1, 0, 2), 0, "ragged")
    want = debug_np(v, golden["magma_u8"])
    kw = kwargs_on(gpu, v)
    partials = torch.full((3, _lib.DEBUGVIZ_PARTIAL_WORDS), 7.0, device=gpu)
    got = present.debug_images(_partials=partials, **kw)
    check_images(got, want, "three workgroups")
    rows = partials.cpu().numpy()
    assert not (rows == 7.0).any()
    again = present.debug_images(**kw)
    assert all(torch.equal(got[k], again[k]) for k in IMAGES)
    # without the special values the self-normalised images are alive, across the workgroups
    v, _ = draw_debug(np.random.default_rng(20261022), H, W, (3, 1, 0, 2), 0, "plain")
    want = debug_np(v, golden["magma_u8"])
    assert all(want[k].max() == 255 for k in SELFNORM)
    check_images(present.debug_images(**kwargs_on(gpu, v)), want, "three workgroups, plain")


SUBSETS = {"tof": ("phasor", "gt_phasor", "depth", "phase_depth", "gt_phase_depth"), "colour": ("image", "gt_image"),
           "quad": ("phasor",), "quad_gt": ("phasor", "gt_quad"), "dd": ("dd",), "depth": ("depth",),
           "gt": ("gt_phasor", "gt_phase_depth"), "amp_error": ("phasor", "gt_phasor")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SUBSETS))
def test_group_subsets(name, gpu, golden):
    """what is absent produces no key and changes no byte of what is present"""
    from gftorf_amd import present
    v = subset(golden_inputs(golden["small"]), *SUBSETS[name])
    if name == "tof":
        v["phasor"] = v["phasor"][:3]
    groups = groups_of(v)
    keys = [k for k in IMAGES if groups & NEEDS[k] == NEEDS[k]]
    full = {k: golden["small"]["out_" + k] for k in keys}
    want = debug_np(v, golden["magma_u8"])
    assert list(want) == keys and all(np.array_equal(want[k], full[k]) for k in keys)
    expect = {"tof": IMAGES[:12], "colour": ("color", "color_gt", "color_error"), "quad": ("amp", "quad"),
              "quad_gt": ("amp", "quad", "quad_gt", "quad_error"), "dd": ("dd",), "depth": ("depth",),
              "gt": ("scattering_phase_gt", "phase_depth_gt"), "amp_error": ("amp", "amp_error", "quad")}[name]
    assert tuple(keys) == expect
    kw = kwargs_on(gpu, v)
    if name in ("colour", "dd"):                     # nothing else is needed
        kw = {k: kw[k] for k in SUBSETS[name]}
    got = present.debug_images(**kw)
    check_images(got, full, name)
    H, W = CASES["small"][:2]
    offsets = present.debug_sheet_layout(H, W, groups)[1]
    base = got[keys[0]].data_ptr()
    assert [t.data_ptr() - base for t in got.values()] == [offsets[k] for k in keys]


@pytest.mark.gpu
def test_planes_in_place_and_every_quad_index(gpu, golden, monkeypatch):
    """`phasor` as whole rows cut from the planes of a larger tensor and `depth` as a [1:2] slice are read where they lie;
    every quad_index with a permutation that is not the identity puts the normalised plane where the reference does"""
    from gftorf_amd import present
    H, W = CASES["ragged"][:2]
    v = golden_inputs(golden["ragged"])
    want = {k: golden["ragged"]["out_" + k] for k in IMAGES}
    kw = kwargs_on(gpu, v)
    real, seen = present._lib.load(), []

    class Spy:
        def __getattr__(self, name):
            def f(*args):
                seen.append((name, args))
                return getattr(real, name)(*args)
            return f
    monkeypatch.setattr(present._lib, "load", lambda: Spy())
    wide = torch.full((9, H + 2, W), float("nan"), device=gpu)
    wide[1:8, :H] = kw["phasor"]
    three = torch.full((3, H, W), float("nan"), device=gpu)
    three[1:2] = kw["depth"]
    before = wide.clone(), three.clone()
    view = wide[1:8, :H]
    assert not view.is_contiguous()
    got = present.debug_images(**dict(kw, phasor=view, depth=three[1:2]))
    calls = [args for name, args in seen if name == "gft_debugviz_images"]
    assert len(calls) == 1 and calls[0][3:6] == (view.data_ptr(), (H + 2) * W, 7) and calls[0][8] == three[1:2].data_ptr()
    monkeypatch.undo()
    check_images(got, want, "in place")
    assert torch.equal(wide.view(torch.int32), before[0].view(torch.int32)) and torch.equal(three.view(torch.int32), before[1].view(torch.int32))
    # a column slice has no contiguous planes: it is copied, and gives the same bytes
    cols = torch.cat([kw["dd"], kw["dd"]], dim=2)[:, :, :W]
    assert not cols.is_contiguous()
    check_images(present.debug_images(**dict(kw, dd=cols)), want, "copied")
    s = golden_inputs(golden["small"])
    perm = tuple(int(k) for k in s["permutation"])
    assert perm != (0, 1, 2, 3)
    skw = kwargs_on(gpu, s)
    for qi in range(4):
        w = debug_np(dict(s, quad_index=np.int32(qi)), golden["magma_u8"])
        shown = [i for i in range(4) if w["quad_error"][i].any()]
        assert shown == [perm.index(qi)]
        check_images(present.debug_images(**dict(skw, quad_index=qi)), w, "quad_index %d" % qi)
    # a quad_index no plane has: all 0
    got = present.debug_images(**dict(skw, quad_index=7))
    assert not got["quad_error"].any().item()
    # a table with a repeated entry shows two planes, each normalised by its own min and max (one near its ground truth, one not)
    rep = (1, 1, 3, 2)
    w = debug_np(dict(s, permutation=np.array(rep, np.int32), quad_index=np.int32(1)), golden["magma_u8"])
    assert [i for i in range(4) if w["quad_error"][i].any()] == [0, 1] and all(w["quad_error"][i].max() == 255 for i in (0, 1))
    both = np.abs(s["phasor"][3:5] - s["gt_quad"][1])
    assert both[0].max() < 0.5 * both[1].max()
    check_images(present.debug_images(**dict(skw, permutation=rep, quad_index=1)), w, "repeated entry")


@pytest.mark.gpu
def test_ranges_and_quad_index_from_the_device(gpu, golden):
    """device tensors give the bytes of the by-value call, and a second call follows their new contents"""
    from gftorf_amd import present
    s = golden_inputs(golden["small"])
    kw = kwargs_on(gpu, s)
    ranges, qi = on(gpu, s["ranges"]), torch.tensor([int(s["quad_index"])], device=gpu, dtype=torch.int32)
    check_images(present.debug_images(**dict(kw, ranges=ranges, quad_index=qi)), restated("small", golden), "device scalars")
    moved = dict(s, ranges=(s["ranges"] * np.float32(0.5) + np.float32(0.01)).astype(np.float32), quad_index=np.int32((int(s["quad_index"]) + 1) % 4))
    want = debug_np(moved, golden["magma_u8"])
    assert not np.array_equal(want["amp"], restated("small", golden)["amp"])
    assert not np.array_equal(want["quad_error"], restated("small", golden)["quad_error"])
    ranges.copy_(on(gpu, moved["ranges"]))
    qi.fill_(int(moved["quad_index"]))
    check_images(present.debug_images(**dict(kw, ranges=ranges, quad_index=qi)), want, "moved device scalars")
    check_images(present.debug_images(**kwargs_on(gpu, moved)), want, "moved by value")


@pytest.mark.gpu
def test_out_with_guards(gpu, golden):
    """64 guard bytes on either side of the sheet stay, the views lie in `out`, every byte between the guards that belongs to
    an image is written"""
    from gftorf_amd import present
    for case in ("ragged", "one"):
        H, W = CASES[case][:2]
        kw = kwargs_on(gpu, golden_inputs(golden[case]))
        total, offsets = present.debug_sheet_layout(H, W, 511)
        for fill in (0x5A, 0xA5):
            buf = torch.full((total + 128,), fill, device=gpu, dtype=torch.uint8)
            got = present.debug_images(out=buf[64:64 + total], **kw)
            assert got["depth"].data_ptr() == buf.data_ptr() + 64
            assert [t.data_ptr() - buf.data_ptr() - 64 for t in got.values()] == [offsets[k] for k in IMAGES]
            assert bool((buf[:64] == fill).all()) and bool((buf[64 + total:] == fill).all())
            check_images(got, {k: golden[case]["out_" + k] for k in IMAGES}, "%s guards %x" % (case, fill))
            sheet = buf[64:64 + total].cpu().numpy()
            owned = np.zeros(total, bool)
            for k in IMAGES:
                owned[offsets[k]:offsets[k] + BPP[k] * H * W] = True
            assert (sheet[~owned] == fill).all()                   # the padding between two images is not written
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        present.debug_images(out=buf[65:], **kw)
    with pytest.raises(RuntimeError, match="the sheet needs"):
        present.debug_images(out=buf[:16], **kw)
    with pytest.raises(TypeError, match="out must be a contiguous one-dimensional torch.uint8"):
        present.debug_images(out=buf.float(), **kw)


@pytest.mark.gpu
def test_no_host_sync_and_a_captured_graph(gpu, golden):
    """debug_images with every device-to-host synchronisation an error; one capture replayed twice, the inputs rewritten in
    place between the replays, equals the eager result both times"""
    from gftorf_amd import _lib, present
    a, b = golden_inputs(golden["small"]), golden_inputs(golden["flat"])
    assert CASES["small"][:3] == CASES["flat"][:3]                 # one size, one (host) permutation
    H, W = CASES["small"][:2]
    kw = kwargs_on(gpu, a)
    kw["ranges"] = on(gpu, a["ranges"])
    kw["quad_index"] = torch.tensor([int(a["quad_index"])], device=gpu, dtype=torch.int32)
    total = present.debug_sheet_layout(H, W, 511)[0]
    out = torch.zeros((total,), device=gpu, dtype=torch.uint8)
    partials = torch.zeros((present.debug_blocks(H * W), _lib.DEBUGVIZ_PARTIAL_WORDS), device=gpu)
    eager = {}
    for name, v in (("small", a), ("flat", b)):
        eager[name] = {k: t.cpu().numpy() for k, t in present.debug_images(**kwargs_on(gpu, v)).items()}
        check_images(eager[name], restated(name, golden), "eager " + name)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        present.debug_images(out=out, _partials=partials, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = present.debug_images(out=out, _partials=partials, **kw)

    def rewrite(v):
        for k in TENSORS:
            kw[k].copy_(on(gpu, v[k]))
        kw["ranges"].copy_(on(gpu, v["ranges"]))
        kw["quad_index"].fill_(int(v["quad_index"]))
    for name, v in (("flat", b), ("small", a)):
        rewrite(v)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        check_images(captured, eager[name], "replayed " + name)


@pytest.mark.gpu
def test_view_sheets(gpu, golden):
    """submit, submit_debug and submit_flow in turn on the same two slots: every one comes out of ready(wait=True) with the
    bytes of its direct call; a third submit_debug with both slots in flight raises"""
    from gftorf_amd import present
    r, s = golden_inputs(golden["ragged"]), golden_inputs(golden["small"])
    rkw, skw = kwargs_on(gpu, r), kwargs_on(gpu, s)
    depth = torch.rand(1, 5, 7, device=gpu) + 0.5
    flow, gt_flow = torch.randn(3, 9, 11, device=gpu), torch.randn(2, 9, 11, device=gpu)
    direct_view = present.view_images(depth=depth, dd=depth, zplanes=(0.3, 4.5))
    direct_flow = present.flow_images(flow, gt_flow)
    sheets = present.ViewSheets(slots=2)
    sheets.submit("view", depth=depth, dd=depth, zplanes=(0.3, 4.5))            # sizes slot 0 for a 5 x 7 view
    sheets.submit_debug("ragged", **rkw)                                          # sizes slot 1
    back = {tag: {k: a.copy() for k, a in images.items()} for tag, images in sheets.ready(wait=True)}
    assert list(back) == ["view", "ragged"]
    sheets.submit_debug("small", **skw)                                           # slot 0, sized by submit: too small, grows
    sheets.submit_flow("flow", flow, gt_flow)                                     # slot 1, sized by submit_debug
    back.update({tag: {k: a.copy() for k, a in images.items()} for tag, images in sheets.ready(wait=True)})
    sheets.submit("view2", depth=depth, dd=depth, zplanes=(0.3, 4.5))            # slot 0, sized by submit_debug
    sheets.submit_debug("dd", dd=rkw["dd"])
    back.update({tag: {k: a.copy() for k, a in images.items()} for tag, images in sheets.ready(wait=True)})
    assert list(back) == ["view", "ragged", "small", "flow", "view2", "dd"]
    check_images(back["ragged"], restated("ragged", golden), "sheets ragged")
    check_images(back["small"], restated("small", golden), "sheets small")
    check_images(back["dd"], {"dd": golden["ragged"]["out_dd"]}, "sheets dd")
    for tag in ("view", "view2"):
        assert all(np.array_equal(back[tag][k], direct_view[k].cpu().numpy()) for k in direct_view)
    assert all(np.array_equal(back["flow"][k], direct_flow[k].cpu().numpy()) for k in direct_flow)
    sheets.submit_debug("a", **skw)
    sheets.submit_debug("b", **skw)
    with pytest.raises(RuntimeError, match="all 2 slots"):
        sheets.submit_debug("c", **skw)
    assert [tag for tag, _ in sheets.ready(wait=True)] == ["a", "b"]


@pytest.mark.gpu
def test_mixed_devices_are_refused_before_any_launch(gpu, golden, monkeypatch):
    from gftorf_amd import present
    real = present._lib.load()

    class NoLaunch:
        def __getattr__(self, name):
            assert name != "gft_debugviz_images", name
            return getattr(real, name)
    monkeypatch.setattr(present._lib, "load", lambda: NoLaunch())
    kw = kwargs_on(gpu, golden_inputs(golden["small"]))
    with pytest.raises(RuntimeError, match="gt_quad is on cpu; the display kernels run on a HIP device only"):
        present.debug_images(**dict(kw, gt_quad=kw["gt_quad"].cpu()))
    with pytest.raises(RuntimeError, match="ranges is on cpu"):
        present.debug_images(**dict(kw, ranges=torch.zeros(8)))
    with pytest.raises(RuntimeError, match="quad_index is on cpu"):
        present.debug_images(**dict(kw, quad_index=torch.zeros(1, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="the images are on cuda:0, out on cpu"):
        present.debug_images(out=torch.zeros(1 << 16, dtype=torch.uint8), **kw)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="depth is on cuda:1, phasor on cuda:0"):
            present.debug_images(**dict(kw, depth=kw["depth"].to("cuda:1")))
