"""gftorf_amd.present.flow_images: the optical-flow debug images of F-ToRF training (train.py:380-398; scene/torf_utils.py:
150-305 make_color_wheel, compute_color, flow_to_image).  The yardstick is the reference's own bytes
(tests/golden/present_flow.npz, written by tests/golden/make_golden_present_flow.py from the reference's flow_to_image called
three times in train.py's order on (R, T), (T, T) and (T - R, T)) and `flow_np` below, the same sequence restated in numpy.

flow_to_image writes into its arguments: the first call zeroes the unknown (> 200) pixels of R and the unknown and NaN pixels
of T in place, so the second call meets no unknown pixel any more (a target's unknown or NaN pixel comes out white) and the
third subtracts the cleaned arrays.  Under numpy >= 2 the float32 `maxrad * 1.1` plus `np.finfo(float).eps` is a float64, and
so is everything behind the division by it; numpy 1.x would stay in float32.  The fixture records the numpy it was written
with, and the restatement pins the float64 route whatever numpy runs the tests.

Every statement except arctan2 is an IEEE operation.  The device's atan2 may differ from numpy's in its last bits, which moves
fk by a few ulp and a byte only where 255 * col lies that close to an integer.  A pixel is *fragile* when the restatement
changes any of its bytes with fk moved by +1e-9 or by -1e-9 (over 1e5 ulp of fk: far beyond any atan2's error, far below a
colour step).  The device tests assert: every byte within 1 of the fixture; outside the fragile pixels every byte equal; and
-- on the CPU too, for the reference alone -- at most 5 % of an image's pixels fragile, so the exclusion cannot hide a
failure.  (Measured for the fixture: no fragile pixel in five cases, 3 of 5883 in `zero_gt`, where the division by 2^-52 puts
every vector far outside the wheel; a saturated channel is not fragile, since f is a multiple of 2^-52 and (1 - f) + f is
exactly 1.)  Black (unknown) and NaN pixels are never fragile and must be exact.  maxrad, the last word of the partials, must
be numpy's float32 value bit for bit.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_flowviz.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "present_flow.npz")
IMAGES = ("flow", "gt", "error")
RUN_PIXELS = 1024                       # pixels of one workgroup's run in the second launch: 256 lanes of 4
THREE = (3, 683)                        # 2049 pixels: the smallest count over three runs; odd width, 2049 % 4 == 1
# name: (H, W, scale of the flows, special values placed, what the target is)
CASES = {"one": (1, 1, 3.0, False, "normal"), "small": (7, 13, 3.0, False, "normal"), "ragged": (37, 53, 60.0, True, "normal"),
         "three": THREE + (150.0, True, "normal"), "zero_gt": (37, 53, 3.0, True, "zero"), "tiny": (37, 53, 0.01, True, "tiny")}
FRAGILE_CAP = 0.05
SHIFT = 1e-9


# ---- the restatement -----------------------------------------------------------------------------------------------------

def wheel_np():
    """the 55 x 3 Middlebury wheel: segments of 15, 6, 4, 11, 13 and 6 entries; one channel at 255, one a floor(255 j / n) ramp"""
    rows = []
    for n, full, ramp, down in ((15, 0, 1, False), (6, 1, 0, True), (4, 1, 2, False), (11, 2, 1, True), (13, 2, 0, False), (6, 0, 2, True)):
        for j in range(n):
            row = [0, 0, 0]
            row[full] = 255
            row[ramp] = 255 - (255 * j) // n if down else (255 * j) // n
            rows.append(row)
    return np.array(rows, np.uint8)


def unknown_np(x0, x1):
    with np.errstate(invalid="ignore"):
        return (np.abs(x0) > 200) | (np.abs(x1) > 200)


def image_np(x0, x1, den, black, wheel, shift=0.0):
    """image(X) of the module docstring for a float32 field whose unknown pixels are already zeroed: uint8 [H, W, 3]"""
    den = np.float64(den)
    with np.errstate(invalid="ignore", over="ignore"):
        u, v = x0.astype(np.float64) / den, x1.astype(np.float64) / den
    nan = np.isnan(u) | np.isnan(v)
    u, v = np.where(nan, 0.0, u), np.where(nan, 0.0, v)
    rad = np.sqrt(u * u + v * v)
    a = np.arctan2(-v, -u) / np.pi
    fk = (a + 1) / 2 * 54 + 1 + shift
    k0 = np.floor(fk).astype(np.int64)
    k1 = np.where(k0 + 1 == 56, 1, k0 + 1)
    f = fk - k0
    out = np.zeros(x0.shape + (3,), np.uint8)
    table = wheel.astype(np.float64)
    for i in range(3):
        c0, c1 = table[k0 - 1, i] / 255, table[k1 - 1, i] / 255
        col = (1 - f) * c0 + f * c1
        col = np.where(rad <= 1, 1 - rad * (1 - col), col * 0.75)
        out[..., i] = np.floor(255 * col * (1 - nan))
    out[black] = 0
    return out


def flow_np(R, T, wheel, shift=0.0):
    """train.py:382-386 for R, T [2, H, W] float32 (not written): dict of the three images, `Rc` and `Tc` (the arrays as the
    calls leave them), `maxrad` (float32) and `den`"""
    assert R.dtype == np.float32 and T.dtype == np.float32
    unk_r = unknown_np(R[0], R[1])
    Rc = np.where(unk_r, np.float32(0), R)
    Tc = np.where(unknown_np(T[0], T[1]), np.float32(0), T)
    Tc = np.where(np.isnan(Tc[0]) | np.isnan(Tc[1]), np.float32(0), Tc)
    maxrad = np.max(np.sqrt(Tc[0] * Tc[0] + Tc[1] * Tc[1]))
    assert maxrad.dtype == np.float32
    den = np.float64(np.float32(maxrad * np.float32(1.1))) + 2.0 ** -52
    with np.errstate(invalid="ignore"):
        E = Tc - Rc
    unk_e = unknown_np(E[0], E[1])
    Ec = np.where(unk_e, np.float32(0), E)
    no = np.zeros(unk_r.shape, bool)
    return dict(flow=image_np(Rc[0], Rc[1], den, unk_r, wheel, shift), gt=image_np(Tc[0], Tc[1], den, no, wheel, shift),
                error=image_np(Ec[0], Ec[1], den, unk_e, wheel, shift), Rc=Rc, Tc=Tc, maxrad=maxrad, den=den, black=dict(flow=unk_r, error=unk_e))


def fragile_np(R, T, wheel):
    """{image: [H, W] bool}: the pixels whose bytes hang on the last bits of arctan2 (the module docstring)"""
    base, up, down = (flow_np(R, T, wheel, s) for s in (0.0, SHIFT, -SHIFT))
    return {k: ((base[k] != up[k]) | (base[k] != down[k])).any(-1) for k in IMAGES}


# ---- inputs --------------------------------------------------------------------------------------------------------------

def special_pairs():
    """(R, T) pixels: a NaN and both infinities in R, a NaN in T, |x| of 250 and 1e3 on either side, an error beyond 200 of two
    known vectors, vectors on the four half-axes, zero vectors with every sign"""
    nan, inf = np.nan, np.inf
    return np.array([((nan, 1.0), (1.0, 2.0)), ((1.0, nan), (0.5, -0.5)), ((inf, 1.0), (1.0, 1.0)), ((2.0, -inf), (-1.0, 1.0)),
                     ((1.0, 2.0), (nan, 1.0)), ((-1.0, 0.5), (2.0, nan)), ((250.0, 1.0), (1.0, 1.0)), ((1.0, -250.0), (1.0, -1.0)),
                     ((1e3, 1e3), (0.5, 0.5)), ((1.0, 1.0), (250.0, 0.0)), ((0.5, 0.25), (1.0, -1e3)), ((-1e3, 0.0), (1e3, 0.0)),
                     ((150.0, 0.0), (-150.0, 0.0)), ((0.0, -120.0), (0.0, 120.0)), ((nan, nan), (nan, nan)), ((inf, inf), (inf, -inf)),
                     ((1.0, 0.0), (0.0, 1.0)), ((-1.0, 0.0), (0.0, -1.0)), ((0.0, 2.0), (-2.0, 0.0)), ((0.0, -2.0), (2.0, 0.0)),
                     ((1.0, -0.0), (-0.0, 1.0)), ((-1.0, -0.0), (-0.0, -1.0)), ((-0.0, 0.0), (-0.0, 0.0)), ((0.0, -0.0), (0.0, -0.0)),
                     ((0.0, 0.0), (0.0, 0.0)), ((-0.0, -0.0), (-0.0, -0.0)), ((-0.0, 0.0), (1.0, 1.0)), ((1.0, 1.0), (-0.0, 0.0))], np.float32)


def draw_flow(rng, H, W, scale, special, target):
    """R, T [2, H, W] float32: normal flows of `scale` (the rendered one the target plus a tenth of it); `target` "zero" makes
    T all zero, "tiny" scales it to a maxrad below 1e-3; with `special` the special pairs are spread over the frame"""
    T = (scale * rng.normal(size=(2, H, W))).astype(np.float32)
    R = (T + 0.1 * scale * rng.normal(size=(2, H, W))).astype(np.float32)
    if target == "zero":
        T[:] = 0
    elif target == "tiny":
        T *= np.float32(1e-2)
    if special:
        sp = special_pairs()
        if target == "tiny":                  # the unknown and NaN values stay; the finite ones shrink with the target
            small = np.abs(sp) < 200
            sp = np.where(small, sp * np.float32(1e-6), sp).astype(np.float32)
        at = rng.permutation(H * W)[:len(sp)]
        R.reshape(2, -1)[:, at] = sp[:, 0].T
        if target != "zero":
            T.reshape(2, -1)[:, at] = sp[:, 1].T
    return R, T


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
    out["wheel"], out["numpy"] = z["wheel"], str(z["numpy"])
    for g in out.values():
        if isinstance(g, dict):
            for a in g.values():
                a.setflags(write=False)
    return out


_NP = {}


def restated(case, g, wheel):
    """`flow_np` and `fragile_np` of a fixture case, computed once and shared"""
    if case not in _NP:
        _NP[case] = (flow_np(g["R"], g["T"], wheel), fragile_np(g["R"], g["T"], wheel))
    return _NP[case]


def check_images(got, g, fragile, what):
    """device images against the fixture's: within 1 everywhere, equal outside the fragile pixels; prints the figures first"""
    for k in IMAGES:
        have = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        want = g["out_" + k]
        assert have.shape == want.shape and have.dtype == np.uint8, (what, k, have.shape, have.dtype)
        diff = np.abs(have.astype(np.int16) - want.astype(np.int16)).max(-1)
        print("%s %s: %d of %d pixels differ (max %d), %d fragile, %d differ outside them"
              % (what, k, int((diff > 0).sum()), diff.size, int(diff.max()), int(fragile[k].sum()), int(((diff > 0) & ~fragile[k]).sum())))
        assert diff.max() <= 1, (what, k, int(diff.max()), np.argwhere(diff > 1)[:4].tolist())
        bad = np.argwhere((diff > 0) & ~fragile[k])
        assert not len(bad), (what, k, len(bad), bad[:4].tolist(), have[tuple(bad[0])], want[tuple(bad[0])])


# ---- CPU-runnable checks -------------------------------------------------------------------------------------------------

def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c_and_every_symbol_is_exported(tmp_path, lib):
    from gftorf_amd import _lib, build, present
    names = declared_functions()
    assert set(names) == set(_lib.FLOWVIZ_EXPORTS) == {"gft_flowviz_blocks", "gft_flowviz_wheel", "gft_flowviz_images"}, names
    others = [t for t in dir(_lib) if t.endswith("EXPORTS") and t != "FLOWVIZ_EXPORTS"]
    assert len(others) >= 11 and "PRESENT_EXPORTS" in others and "EXPORTS" in others
    for t in others:
        assert not set(names) & set(getattr(_lib, t)), t
    for n in names:
        assert hasattr(lib, n), n
    assert "k_flowviz.hip" in build.SOURCES and callable(present.flow_images) and callable(present.ViewSheets.submit_flow)
    assert "struct" not in re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    prog = tmp_path / "flowviz_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_flowviz.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "flowviz_abi.o")])
    out = subprocess.check_output(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-include", "gftorf_flowviz.h",
                                   "-x", "c", "-"], input="FLOWVIZ_WORDS_ARE GFT_FLOWVIZ_WHEEL_ROWS GFT_FLOWVIZ_IMAGES GFT_FLOWVIZ_RUN\n", text=True)
    consts = [int(x) for x in out.split("FLOWVIZ_WORDS_ARE", 1)[1].split()]
    assert consts == [_lib.FLOWVIZ_WHEEL_ROWS, _lib.FLOWVIZ_IMAGES, _lib.FLOWVIZ_RUN] == [55, 3, 4]
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16


def test_the_wheel_is_the_fixtures(lib, golden):
    from gftorf_amd import present
    wheel = present.flow_wheel()
    assert wheel.shape == (55, 3) and wheel.dtype == np.uint8
    assert np.array_equal(wheel, golden["wheel"]) and np.array_equal(wheel, wheel_np())
    assert (wheel.max(1) == 255).all() and wheel[0].tolist() == [255, 0, 0] and wheel[15].tolist() == [255, 255, 0]


def test_the_numpy_statements_give_the_reference_bytes(golden):
    """`flow_np` against what the reference's three flow_to_image calls wrote into the fixture: the three images exactly, R and T
    as the calls left them, and at most 5 % fragile pixels per image for the reference alone"""
    assert int(golden["numpy"].split(".")[0]) >= 2, golden["numpy"]
    wheel = golden["wheel"]
    seen = set()
    for c, (H, W, scale, special, target) in CASES.items():
        g = golden[c]
        R, T = g["R"], g["T"]
        assert R.shape == T.shape == (2, H, W) and R.dtype == T.dtype == np.float32, c
        res, fragile = restated(c, g, wheel)
        for k in IMAGES:
            want = g["out_" + k]
            assert want.shape == (H, W, 3) and want.dtype == np.uint8
            assert np.array_equal(res[k], want), (c, k, np.argwhere(res[k] != want)[:4].tolist())
            share = float(fragile[k].mean())
            print("%s %s: %.2f %% fragile" % (c, k, 100 * share))
            assert share <= FRAGILE_CAP, (c, k, share)
        for k in ("flow", "error"):
            assert not (fragile[k] & res["black"][k]).any() and not g["out_" + k][res["black"][k]].any(), (c, k)
        assert np.array_equal(res["Rc"].view(np.uint32), g["R_after"].view(np.uint32)), c
        assert np.array_equal(res["Tc"].view(np.uint32), g["T_after"].view(np.uint32)), c
        assert not np.isnan(g["T_after"]).any() and np.abs(g["T_after"]).max() <= 200
        if special:
            assert H * W >= 37 * 53
            assert np.isnan(R).any() and np.isposinf(R).any() and np.isneginf(R).any() and np.isnan(g["R_after"]).any()
            assert (np.abs(R) == 250).any() and (np.abs(R) == 1e3).any() and res["black"]["flow"].sum() >= 6
            if target != "zero":
                assert np.isnan(T).any() and (np.abs(T) == 250).any() and (np.abs(T) == 1e3).any()
                # a NaN or unknown target pixel is white in gt
                lost = np.isnan(T).any(0) | unknown_np(T[0], T[1])
                assert lost.sum() >= 6 and (g["out_gt"][lost] == 255).all()
            if target == "normal":
                assert res["black"]["error"].sum() >= 2          # two known vectors more than 200 apart
            assert ((R[0] == 0) & (R[1] == 0) & np.signbit(R[0]) & ~np.signbit(R[1])).any()            # (-0.0, 0.0)
            for axis, sign in ((0, 1), (0, -1), (1, 1), (1, -1)):
                assert ((np.sign(R[axis]) == sign) & (R[1 - axis] == 0)).any(), (c, axis, sign)
            seen.add(target)
        if target == "zero":
            assert not T.any() and res["maxrad"] == 0 and res["den"] == 2.0 ** -52
        elif target == "tiny":
            assert 0 < res["maxrad"] < 1e-3
    assert seen == {"normal", "zero", "tiny"}
    H, W = THREE
    assert W % 2 == 1 and (H * W) % 4 != 0 and -(-H * W // RUN_PIXELS) == 3 and -(-(H * W - 1) // RUN_PIXELS) == 2
    # the restatement does not write its inputs (the fixture's arrays are read-only) and the sequence matters: with a target
    # pixel unknown, gt on the untouched T would be black there
    assert (golden["three"]["out_gt"].reshape(-1, 3) == 255).all(1).sum() >= 6


def test_size_queries_and_c_argument_checks(lib):
    import ctypes as C
    from gftorf_amd import _lib, present
    assert present.flow_blocks(0) == 0 and lib.gft_flowviz_blocks(-5) == 0
    assert [present.flow_blocks(n) for n in (1, 1024, 1025, 2048, 2049, 1 << 30)] == [1, 1, 2, 2, 3, 1024]
    assert present.flow_blocks(THREE[0] * THREE[1]) == 3
    x = C.c_void_p(16)                                         # never dereferenced: the calls fail before any launch

    def call(H=4, W=4, flow=x, fs=16, gt=x, gs=16, part=x, out=x):
        return lib.gft_flowviz_images(None, H, W, flow, fs, gt, gs, part, out)
    for bad, msg in ((dict(H=0), "bad size"), (dict(W=-1), "bad size"), (dict(flow=None), "NULL"), (dict(gt=None), "NULL"),
                     (dict(out=None), "NULL"), (dict(part=None), "partials is NULL"), (dict(part=C.c_void_p(18)), "4-byte aligned"),
                     (dict(fs=-1), "bad plane stride"), (dict(gs=-4), "bad plane stride")):
        assert call(**bad) != 0, bad
        assert msg in _lib.last_error(), (bad, _lib.last_error())


def test_wrapper_rejects_bad_arguments_before_any_launch(lib, monkeypatch):
    from gftorf_amd import present
    fl, gt = torch.rand(3, 4, 6), torch.rand(2, 4, 6)

    class NoLaunch:
        def __getattr__(self, name):
            assert name != "gft_flowviz_images", name
            return getattr(lib, name)
    monkeypatch.setattr(present._lib, "load", lambda: NoLaunch())
    with pytest.raises(RuntimeError, match="flow is on cpu; the display kernels run on a HIP device only, there is no CPU path"):
        present.flow_images(fl, gt)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        present.ViewSheets(slots=1).submit_flow(0, fl, gt)
    for c, msg in [(lambda: present.flow_images(fl[:1], gt), r"flow must be \[>=2, H, W\], got \[1, 4, 6\]"),
                   (lambda: present.flow_images(fl[0], gt), r"flow must be \[>=2, H, W\]"),
                   (lambda: present.flow_images(fl, fl), r"gt_flow must be \[2, H, W\], got \[3, 4, 6\]"),
                   (lambda: present.flow_images(fl, gt[:, :3]), "gt_flow is 3 x 6, flow 4 x 6: the inputs of one call have one size"),
                   (lambda: present.flow_images(fl, gt[:, :, :5]), "gt_flow is 4 x 5, flow 4 x 6")]:
        with pytest.raises(RuntimeError, match=msg):
            c()
    for c, msg in [(lambda: present.flow_images(fl.numpy(), gt), "flow must be a tensor"),
                   (lambda: present.flow_images(fl.double(), gt), "flow must be torch.float32"),
                   (lambda: present.flow_images(fl, gt.half()), "gt_flow must be torch.float32"),
                   (lambda: present.flow_images(fl, gt, out=torch.zeros(3, 4, 6, 3)), r"out must be a contiguous torch.uint8 tensor \[3, 4, 6, 3\]"),
                   (lambda: present.flow_images(fl, gt, out=torch.zeros(3, 4, 5, 3, dtype=torch.uint8)), r"out must be a contiguous torch.uint8 tensor \[3, 4, 6, 3\]"),
                   (lambda: present.flow_images(fl, gt, out=torch.zeros(3, 4, 6, 6, dtype=torch.uint8)[..., ::2]), "out must be a contiguous")]:
        with pytest.raises(TypeError, match=msg):
            c()
    with pytest.raises(ValueError, match="give flow as a"):
        present.ViewSheets(slots=1).submit_flow(0, fl[0], gt)


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def on(dev, a):
    return torch.tensor(np.ascontiguousarray(a), device=dev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_flow_images_are_the_reference_bytes(case, gpu, golden):
    """every fixture case: the three images (the module docstring's three assertions), maxrad bit for bit, the inputs untouched"""
    from gftorf_amd import present
    g = golden[case]
    H, W = CASES[case][:2]
    res, fragile = restated(case, g, golden["wheel"])
    for k in IMAGES:
        assert fragile[k].mean() <= FRAGILE_CAP, (case, k)
    R, T = on(gpu, g["R"]), on(gpu, g["T"])
    blocks = present.flow_blocks(H * W)
    assert blocks == -(-H * W // RUN_PIXELS)
    partials = torch.full((blocks + 1,), -1.0, device=gpu)
    got = present.flow_images(R, T, _partials=partials)
    assert list(got) == list(IMAGES) and all(t.shape == (H, W, 3) and t.dtype == torch.uint8 and t.device == gpu for t in got.values())
    assert got["gt"].data_ptr() - got["flow"].data_ptr() == 3 * H * W == got["error"].data_ptr() - got["gt"].data_ptr()
    maxrad = partials.cpu().numpy()
    print("%s maxrad: device %r numpy %r" % (case, float(maxrad[-1]), float(res["maxrad"])))
    assert maxrad[-1:].view(np.uint32)[0] == np.array([res["maxrad"]], np.float32).view(np.uint32)[0] and (maxrad[:-1] <= maxrad[-1]).all()
    check_images(got, g, fragile, case)
    for k in ("flow", "error"):                              # black pixels are exact
        assert not got[k].cpu().numpy()[res["black"][k]].any(), (case, k)
    assert np.array_equal(R.cpu().numpy().view(np.uint32), g["R"].view(np.uint32))
    assert np.array_equal(T.cpu().numpy().view(np.uint32), g["T"].view(np.uint32))


@pytest.mark.gpu
def test_planes_in_place_out_and_reproducible(gpu, golden, monkeypatch):
    """`flow` as planes 0:2 of a [3, H, W] tensor and as whole rows cut from wider planes is read where it lies and gives the
    bytes of a contiguous copy; `out` is written in place at any address; two runs are bit-equal"""
    from gftorf_amd import present
    case = "three"
    H, W = CASES[case][:2]
    g = golden[case]
    fragile = restated(case, g, golden["wheel"])[1]
    R, T = on(gpu, g["R"]), on(gpu, g["T"])
    plain = present.flow_images(R, T)
    again = present.flow_images(R, T)
    assert all(torch.equal(plain[k], again[k]) for k in IMAGES)
    real, seen = present._lib.load(), []

    class Spy:
        def __getattr__(self, name):
            def f(*args):
                seen.append((name, args))
                return getattr(real, name)(*args)
            return f
    monkeypatch.setattr(present._lib, "load", lambda: Spy())
    three = torch.full((3, H, W), float("nan"), device=gpu)
    three[:2] = R
    wide = torch.full((3, H + 2, W), float("nan"), device=gpu)
    wide[:2, :H] = R
    wide_gt = torch.full((2, H + 5, W), float("nan"), device=gpu)
    wide_gt[:, :H] = T
    before = [t.clone() for t in (three, wide, wide_gt)]
    a = present.flow_images(three, T)
    b = present.flow_images(three[:2], T)
    c = present.flow_images(wide[:, :H], wide_gt[:, :H])
    assert not wide[:, :H].is_contiguous() and not wide_gt[:, :H].is_contiguous()
    calls = [args for name, args in seen if name == "gft_flowviz_images"]
    assert [x[3:7] for x in calls] == [(three.data_ptr(), H * W, T.data_ptr(), H * W)] * 2 + \
                                      [(wide.data_ptr(), (H + 2) * W, wide_gt.data_ptr(), (H + 5) * W)]
    monkeypatch.undo()
    for other in (a, b, c):
        assert all(torch.equal(plain[k], other[k]) for k in IMAGES)
    for t, was in zip((three, wide, wide_gt), before):
        assert torch.equal(t.view(torch.int32), was.view(torch.int32))
    # a column slice has no contiguous planes: it is copied, and gives the same bytes
    cols = torch.cat([R, R], dim=2)[:, :, :W]
    assert not cols.is_contiguous() and all(torch.equal(plain[k], x) for k, x in present.flow_images(cols, T).items())
    n = 3 * H * W * 3
    buf = torch.full((n + 8,), 7, device=gpu, dtype=torch.uint8)
    for shift in (0, 1, 2, 3):                                # every offset of the images within a dword
        buf.fill_(7)
        target = buf[shift:shift + n].view(3, H, W, 3)
        got = present.flow_images(R, T, out=target)
        assert got["flow"].data_ptr() == target.data_ptr() and bool((buf[:shift] == 7).all()) and bool((buf[shift + n:] == 7).all())
        assert all(torch.equal(plain[k], got[k]) for k in IMAGES), shift
    check_images(plain, g, fragile, "three again")


@pytest.mark.gpu
def test_no_host_sync_capture_and_view_sheets(gpu, golden):
    """flow_images and ViewSheets.submit_flow with every device-to-host synchronisation an error; a captured graph replayed
    with new input contents gives the new images; submit_flow + ready(wait=True) returns flow_images' bytes, also in slots that
    submit has used"""
    from gftorf_amd import present
    ga, gb = golden["ragged"], golden["tiny"]
    H, W = CASES["ragged"][:2]
    assert CASES["tiny"][:2] == (H, W)
    R, T = on(gpu, ga["R"]), on(gpu, ga["T"])
    out = torch.zeros((3, H, W, 3), device=gpu, dtype=torch.uint8)
    partials = torch.zeros((present.flow_blocks(H * W) + 1,), device=gpu)
    sheets = present.ViewSheets(slots=2)
    want_a = {k: t.clone() for k, t in present.flow_images(R, T).items()}       # warm-up: the library's load, the pinned buffers
    sheets.submit_flow("warm", R, T)
    list(sheets.ready(wait=True))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        present.flow_images(R, T, out=out, _partials=partials)
        sheets.submit_flow("a", R, T)
        sheets.submit_flow("b", R[:, :7], T[:, :7])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert all(torch.equal(out[i], want_a[k]) for i, k in enumerate(IMAGES))
    done = [(tag, {k: a.copy() for k, a in images.items()}) for tag, images in sheets.ready(wait=True)]
    assert [tag for tag, _ in done] == ["a", "b"] and list(done[0][1]) == list(IMAGES)
    small = present.flow_images(R[:, :7], T[:, :7])
    for (tag, images), want in zip(done, (want_a, small)):
        for k in IMAGES:
            assert images[k].dtype == np.uint8 and np.array_equal(images[k], want[k].cpu().numpy()), (tag, k)
    with pytest.raises(RuntimeError, match="all 2 slots"):
        sheets.submit_flow("c", R, T), sheets.submit_flow("d", R, T), sheets.submit_flow("e", R, T)
    list(sheets.ready(wait=True))
    # a slot sized by submit_flow serves submit, and the other way round
    depth = torch.rand(1, 5, 7, device=gpu) + 0.5
    direct = present.view_images(depth=depth, dd=depth, zplanes=(0.3, 4.5))
    sheets.submit("view", depth=depth, dd=depth, zplanes=(0.3, 4.5))
    sheets.submit_flow("flow", R, T)
    back = {tag: {k: a.copy() for k, a in images.items()} for tag, images in sheets.ready(wait=True)}
    assert all(np.array_equal(back["view"][k], direct[k].cpu().numpy()) for k in direct)
    assert all(np.array_equal(back["flow"][k], want_a[k].cpu().numpy()) for k in IMAGES)
    # capture, then other contents in the same tensors
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = present.flow_images(R, T, out=out, _partials=partials)
    R.copy_(on(gpu, gb["R"]))
    T.copy_(on(gpu, gb["T"]))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    res, fragile = restated("tiny", gb, golden["wheel"])
    assert not torch.equal(captured["gt"], want_a["gt"])
    check_images(captured, gb, fragile, "replayed")
    assert partials.cpu().numpy()[-1:].view(np.uint32)[0] == np.array([res["maxrad"]], np.float32).view(np.uint32)[0]
