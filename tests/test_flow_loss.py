"""gftorf_amd.flow: the F-ToRF scene-flow term of train.py:243-261 (scene/torf_utils.py distance_to_points3d, project_points,
project_flow and the squared-error mean) against the reference's values and gradients (tests/golden/flow.npz,
tests/golden/make_golden_flow.py) and against the formulas restated in float64 on the CPU; bit-reproducible, free of host
reads, captured in a graph, and composed with the rasterizer in an ftorf-shaped iteration."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_flow.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "flow.npz")
CASES = ("ident", "ragged", "fwdonly")


# ---- the float64 restatement ---------------------------------------------------------------------------------------

def ref_points3d(depth, K, w2v):
    """distance_to_points3d: the colour intrinsics, then inverse(world_view_transform) AS STORED, rows 0..2"""
    H, W = depth.shape[1:]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    u = torch.arange(W, dtype=depth.dtype, device=depth.device).view(1, W).expand(H, W)
    v = torch.arange(H, dtype=depth.dtype, device=depth.device).view(H, 1).expand(H, W)
    z = depth / torch.sqrt(((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2 + 1)
    x, y = (u - cx) * z / fx, (v - cy) * z / fy
    p = torch.cat([x, y, z], 0).reshape(3, -1)
    p = torch.linalg.inv(w2v) @ torch.cat([p, torch.ones_like(p[:1])], 0)
    return p[:3].reshape(3, H, W)


def ref_project(p3, K_tof, w2v_tof):
    """project_points: K_tof @ (world_view_transform_tof^T @ [p, 1])[:3], then xy / (z + 1e-7)"""
    H, W = p3.shape[1:]
    p = p3.reshape(3, -1)
    q = K_tof @ (w2v_tof.T @ torch.cat([p, torch.ones_like(p[:1])], 0))[:3]
    return (q[:2] / (q[2:] + 1e-7)).reshape(2, H, W)


def ref_flow_l2(depth, K, w2v, K_tof, w2v_tof, f3, gt):
    p3 = ref_points3d(depth, K, w2v)
    p2 = ref_project(p3, K_tof, w2v_tof)
    flow2d = ref_project(p3 + f3, K_tof, w2v_tof) - p2
    return ((flow2d - gt) ** 2).mean(), flow2d


def d64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def golden(case):
    z = np.load(GOLDEN)
    g = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + "_")}
    g["dirs"] = [d for d in ("fwd", "bwd") if "flow3d_" + d in g]
    return g


def ref_case(inp, dirs):
    """(points3d, points2d, {dir: (l2, flow2d, grad)}) in float64 from the float32 inputs"""
    depth, K, w2v, K_tof, w2v_tof = (d64(inp[k]) for k in ("depth", "K", "w2v", "K_tof", "w2v_tof"))
    p3 = ref_points3d(depth, K, w2v)
    out = {}
    for d in dirs:
        f = d64(inp["flow3d_" + d]).requires_grad_()
        l2, flow2d = ref_flow_l2(depth, K, w2v, K_tof, w2v_tof, f, d64(inp["gt_" + d]))
        (g,) = torch.autograd.grad(l2, f)
        out[d] = (float(l2.detach()), flow2d.detach(), g)
    return p3, ref_project(p3, K_tof, w2v_tof), out


def test_restatement_reproduces_the_golden_vectors():
    """the reference ran in float32; the float64 restatement of the same inputs agrees to float32 rounding"""
    for case in CASES:
        g = golden(case)
        p3, p2, per = ref_case(g, g["dirs"])
        assert np.abs(p3.numpy() - g["points3d"]).max() <= 2e-6 * np.abs(g["points3d"]).max(), case
        assert np.abs(p2.numpy() - g["points2d"]).max() <= 2e-6 * np.abs(g["points2d"]).max(), case
        for d in g["dirs"]:
            l2, flow2d, grad = per[d]
            assert abs(l2 - float(g["l2_" + d])) <= 1e-5 * l2, (case, d)
            assert np.abs(flow2d.numpy() - g["flow2d_" + d]).max() <= 1e-4, (case, d)
            assert np.abs(grad.numpy() - g["grad_" + d]).max() <= 1e-4 * np.abs(grad.numpy()).max(), (case, d)
    # the quirk kept from the reference: inverse(world_view_transform) of the stored (transposed) matrix, rows 0..2, is the
    # world-to-view rotation applied to the camera-space point, with no translation
    g = golden("ragged")
    w2v = d64(g["w2v"])
    p3 = ref_points3d(d64(g["depth"]), d64(g["K"]), w2v).reshape(3, -1)
    pc = ref_points3d(d64(g["depth"]), d64(g["K"]), torch.eye(4, dtype=torch.float64)).reshape(3, -1)
    assert torch.allclose(p3, w2v[:3, :3].T @ pc, rtol=0, atol=1e-6)          # (R in float32 is orthogonal to ~1e-7)
    assert float(w2v[3, :3].abs().max()) > 0.1


# ---- CPU-runnable checks: errors, C header -------------------------------------------------------------------------

def _cam(K, w2v, K_tof=None, w2v_tof=None, fwd=None, bwd=None):
    return types.SimpleNamespace(K=K, world_view_transform=w2v, K_tof=K if K_tof is None else K_tof,
                                 world_view_transform_tof=w2v if w2v_tof is None else w2v_tof, forward_flow=fwd,
                                 backward_flow=bwd)


def test_new_functions_reject_cpu_tensors():
    from gftorf_amd import flow
    H, W = 6, 8
    K, w2v = torch.eye(3), torch.eye(4)
    depth, f3, gt = torch.ones(1, H, W), torch.zeros(3, H, W), torch.zeros(2, H, W)
    cam = _cam(K, w2v, fwd=gt, bwd=gt)
    calls = [lambda: flow.flow_loss(depth, cam, f3, f3), lambda: flow.scene_flow_l2(depth, K, w2v, K, w2v, f3, gt),
             lambda: flow.distance_to_points3d(depth, cam), lambda: flow.project_points(f3, cam),
             lambda: flow.project_flow(gt, f3, f3, cam)]
    for c in calls:
        with pytest.raises(RuntimeError, match="HIP device only, there is no CPU path"):
            c()


def test_shapes_and_gradients_are_checked():
    from gftorf_amd import flow
    H, W = 6, 8
    K, w2v = torch.eye(3), torch.eye(4)
    depth, f3, gt = torch.ones(1, H, W), torch.zeros(3, H, W), torch.zeros(2, H, W)
    with pytest.raises(RuntimeError, match=r"depth must be \[1, H, W\]"):
        flow.scene_flow_l2(torch.ones(H, W), K, w2v, K, w2v, f3, gt)
    with pytest.raises(RuntimeError, match=r"flow3d_forward must be \[3, 6, 8\]"):
        flow.scene_flow_l2(depth, K, w2v, K, w2v, torch.zeros(3, H, W + 1), gt)
    with pytest.raises(RuntimeError, match=r"gt_backward must be \[2, 6, 8\]"):
        flow.scene_flow_l2(depth, K, w2v, K, w2v, None, None, f3, torch.zeros(3, H, W))
    with pytest.raises(RuntimeError, match=r"world_view_transform_tof must be \[4, 4\]"):
        flow.scene_flow_l2(depth, K, w2v, K, torch.eye(3), f3, gt)
    with pytest.raises(RuntimeError, match=r"K must be \[3, 3\]"):
        flow.scene_flow_l2(depth, torch.eye(4), w2v, K, w2v, f3, gt)
    with pytest.raises(RuntimeError, match=r"points2d_curr must be \[2, 6, 8\]"):
        flow.project_flow(torch.zeros(2, H, 3), f3, f3, _cam(K, w2v))
    with pytest.raises(NotImplementedError, match="depth requires grad"):
        flow.scene_flow_l2(depth.clone().requires_grad_(), K, w2v, K, w2v, f3, gt)
    with pytest.raises(NotImplementedError, match="gt_forward requires grad"):
        flow.scene_flow_l2(depth, K, w2v, K, w2v, f3, gt.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="distance_map requires grad"):
        flow.distance_to_points3d(depth.clone().requires_grad_(), _cam(K, w2v))
    with pytest.raises(NotImplementedError, match="points3d_curr requires grad"):
        flow.project_flow(gt, f3.clone().requires_grad_(), f3, _cam(K, w2v))


@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c_and_every_symbol_is_exported(tmp_path, lib):
    from gftorf_amd import _lib
    names = declared_functions()
    assert set(names) == set(_lib.FLOW_EXPORTS), names
    assert not set(names) & set(_lib.EXPORTS)
    for n in names:
        assert hasattr(lib, n), n
    prog = tmp_path / "flow_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_flow.h"', '#include "gftorf_loss.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    exe = tmp_path / "flow_abi"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(exe) + ".o"])
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16


def test_size_query_and_argument_errors(lib):
    from gftorf_amd import _lib
    assert lib.gft_flow_loss_blocks(0, 5) == 0 and lib.gft_flow_loss_blocks(5, -1) == 0
    assert lib.gft_flow_loss_blocks(1, 1) == 1
    assert lib.gft_flow_loss_blocks(240, 320) == 300          # one pixel per thread, 256 threads per workgroup
    assert lib.gft_flow_loss_blocks(480, 640) == 1024         # then grid-stride
    x = C.c_void_p(16)                                         # never dereferenced: the calls fail before any launch
    assert lib.gft_flow_loss_forward(None, 0, 8, x, x, x, x, x, None, None, None, None, 1.0, x) != 0
    assert "bad sizes" in _lib.last_error()
    assert lib.gft_flow_loss_forward(None, 4, 8, x, x, None, x, x, None, None, None, None, 1.0, x) != 0
    assert "NULL" in _lib.last_error()
    assert lib.gft_flow_loss_forward(None, 4, 8, x, x, x, x, x, x, None, None, None, 1.0, x) != 0
    assert "without its gt" in _lib.last_error()
    assert lib.gft_flow_loss_backward(None, 4, 8, x, x, x, x, x, None, None, x, None, None, None, 1.0, None, x) != 0
    assert "without its gt" in _lib.last_error()
    assert lib.gft_flow_points(None, 4, 8, x, x, x, None, None, None, None) != 0
    assert "NULL" in _lib.last_error()
    assert lib.gft_flow_points(None, 4, 8, x, x, x, None, None, None, x) != 0
    assert "needs K_tof" in _lib.last_error()
    assert lib.gft_flow_project(None, 4, 8, x, x, None, None, None, x) != 0
    assert lib.gft_flow_project_backward(None, 4, 8, x, x, x, None, None, x) != 0
    # backward with no direction to write: nothing to launch, success
    assert lib.gft_flow_loss_backward(None, 4, 8, x, x, x, x, x, None, None, None, None, None, None, 1.0, x, x) == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------

MEASURED = {}          # largest error per check, printed at the end of the module's GPU tests (pytest -s)


def _note(key, err):
    MEASURED[key] = max(MEASURED.get(key, 0.0), float(err))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if MEASURED:
        print("\nflow errors measured:", {k: "%.3g" % v for k, v in sorted(MEASURED.items())})


def _dev_inputs(inp, dirs, dev):
    t = {k: torch.tensor(np.asarray(inp[k]), dtype=torch.float32, device=dev)
         for k in ["depth", "K", "w2v", "K_tof", "w2v_tof"] + ["%s_%s" % (a, d) for d in dirs for a in ("flow3d", "gt")]}
    return t


def _fused(t, dirs, up=(1.0, 1.0)):
    """scene_flow_l2 forward + backward with upstream gradients `up`: values and gradients"""
    from gftorf_amd import flow
    f = {d: t["flow3d_" + d].clone().requires_grad_() for d in dirs}
    lf, lb = flow.scene_flow_l2(t["depth"], t["K"], t["w2v"], t["K_tof"], t["w2v_tof"],
                                f.get("fwd"), t.get("gt_fwd"), f.get("bwd"), t.get("gt_bwd"))
    (up[0] * lf + up[1] * lb).backward()
    return float(lf.detach()), float(lb.detach()), {d: f[d].grad for d in dirs}


# Tolerances, from the errors measured on the MI355X (largest over all cases and shapes, relative to the largest |value|):
# loss 2.2e-7, loss gradients 2.1e-6, project_flow gradients 3.9e-7, points3d 1.8e-7, points2d 2.9e-7, 2-D flows 3.5e-6
# (the difference of two projections of ~100 px).  Each bound leaves a margin of 5-10x.
LOSS_RTOL, GRAD_RTOL, POINTS_RTOL, FLOW2D_RTOL = 2e-6, 2e-5, 2e-6, 2e-5


def _check_against(t, dirs, p3_ref, p2_ref, per_ref, what):
    from gftorf_amd import flow
    cam = _cam(t["K"], t["w2v"], t["K_tof"], t["w2v_tof"], t.get("gt_fwd"), t.get("gt_bwd"))
    # the drop-ins
    p3 = flow.distance_to_points3d(t["depth"], cam)
    p2 = flow.project_points(p3, cam)
    e3 = float((p3.double().cpu() - p3_ref).abs().max() / p3_ref.abs().max())
    e2 = float((p2.double().cpu() - p2_ref).abs().max() / p2_ref.abs().max())
    _note("points3d rel-max " + what, e3)
    _note("points2d rel-max " + what, e2)
    assert e3 <= POINTS_RTOL and e2 <= POINTS_RTOL, (what, e3, e2)
    for d in dirs:
        l2, flow2d_ref, grad_ref = per_ref[d]
        f = t["flow3d_" + d].clone().requires_grad_()
        flow2d = flow.project_flow(p2, p3, f, cam)
        ef = float((flow2d.detach().double().cpu() - flow2d_ref).abs().max() / flow2d_ref.abs().max())
        _note("flow2d rel-max " + what, ef)
        assert ef <= FLOW2D_RTOL, (what, d, ef)
        gout = torch.linspace(-1, 1, flow2d.numel(), device=flow2d.device).view_as(flow2d)
        (g,) = torch.autograd.grad(flow2d, f, gout)
        fr = d64(t["flow3d_" + d].cpu()).requires_grad_()
        yr = ref_project(p3_ref + fr, d64(t["K_tof"].cpu()), d64(t["w2v_tof"].cpu()))
        (gr,) = torch.autograd.grad(yr, fr, gout.double().cpu())
        eg = float((g.double().cpu() - gr).abs().max() / gr.abs().max())
        _note("project_flow grad rel-max " + what, eg)
        assert eg <= GRAD_RTOL, (what, d, eg)
    # the fused term: both directions, and each alone
    up = (2.5, -0.75)
    lf, lb, grads = _fused(t, dirs, up)
    for d, l in zip(("fwd", "bwd"), (lf, lb)):
        if d not in dirs:
            assert l == 0.0
            continue
        el = abs(l - per_ref[d][0]) / per_ref[d][0]
        _note("loss rel " + what, el)
        assert el <= LOSS_RTOL, (what, d, l, per_ref[d][0])
        gref = (up[0] if d == "fwd" else up[1]) * per_ref[d][2]
        eg = float((grads[d].double().cpu() - gref).abs().max() / gref.abs().max())
        _note("loss grad rel-max " + what, eg)
        assert eg <= GRAD_RTOL, (what, d, eg)
    for d in dirs:
        lf1, lb1, g1 = _fused(t, [d], up)
        assert (lf1, lb1) == ((lf, 0.0) if d == "fwd" else (0.0, lb)), (what, d)
        assert torch.equal(g1[d], grads[d]), (what, d)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_matches_the_golden_vectors(case, gpu):
    g = golden(case)
    t = _dev_inputs(g, g["dirs"], gpu)
    per = {d: (float(g["l2_" + d]), d64(g["flow2d_" + d]), d64(g["grad_" + d])) for d in g["dirs"]}
    _check_against(t, g["dirs"], d64(g["points3d"]), d64(g["points2d"]), per, "golden")


def random_case(H, W, seed):
    """random intrinsics and poses (the ToF camera a rotation and a baseline away), depth 0.5-8, 3-D flows of 0.01-0.2,
    ground truth of a few pixels; re-drawn while a current or next point comes within 0.1 of the ToF camera's plane"""
    rng = np.random.default_rng(seed)
    from gftorf_amd import synth
    for _ in range(50):
        f = rng.uniform(0.8, 1.2) * max(W, 8)
        K = np.array([[f, 0, rng.uniform(0.3, 0.7) * W], [0, f * rng.uniform(0.9, 1.1), rng.uniform(0.3, 0.7) * H], [0, 0, 1]],
                     np.float32)
        K_tof = K.copy()
        K_tof[:2] *= np.float32(rng.uniform(0.9, 1.1))
        K_tof[2] = [0, 0, 1]
        a = rng.uniform(-0.15, 0.15, 3)
        w2c = synth.look_at_w2c(*a, t=rng.uniform(-0.3, 0.3, 3))
        w2c_tof = synth.look_at_w2c(*(a + rng.uniform(-0.05, 0.05, 3)), t=w2c[:3, 3] + rng.uniform(-0.08, 0.08, 3))
        inp = dict(depth=rng.uniform(0.5, 8.0, (1, H, W)).astype(np.float32), K=K, K_tof=K_tof,
                   w2v=np.ascontiguousarray(w2c.T), w2v_tof=np.ascontiguousarray(w2c_tof.T))
        for d in ("fwd", "bwd"):
            inp["flow3d_" + d] = (rng.uniform(0.01, 0.2, (3, H, W)) * rng.choice([-1.0, 1.0], (3, H, W))).astype(np.float32)
            inp["gt_" + d] = (2.0 * rng.normal(size=(2, H, W))).astype(np.float32)
        p3 = ref_points3d(d64(inp["depth"]), d64(K), d64(inp["w2v"])).reshape(3, -1)
        M = d64(inp["w2v_tof"]).T
        zs = [M[2, :3] @ p + M[2, 3] for p in (p3, p3 + d64(inp["flow3d_fwd"]).reshape(3, -1),
                                                 p3 + d64(inp["flow3d_bwd"]).reshape(3, -1))]
        if min(float(z.abs().min()) for z in zs) >= 0.1:
            return inp
    raise RuntimeError("no admissible draw")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(240, 320), (480, 640), (1, 1), (17, 300), (37, 53)])
def test_matches_the_float64_formulas(shape, gpu):
    inp = random_case(*shape, seed=shape[0] * 1000 + shape[1])
    p3, p2, per = ref_case(inp, ("fwd", "bwd"))
    t = _dev_inputs(inp, ("fwd", "bwd"), gpu)
    _check_against(t, ("fwd", "bwd"), p3, p2, per, "f64")


@pytest.mark.gpu
def test_points_mode_writes_both_outputs(gpu):
    """gft_flow_points with both outputs: points3d bit for bit the drop-in's; points2d equal to project_points' to float32
    rounding (measured: a few ulp; the two kernels keep the points in registers or read them back, and the compiler may
    contract the projection's products differently)"""
    from gftorf_amd import _lib, flow
    lib = _lib.load()
    t = _dev_inputs(random_case(37, 53, 5), ("fwd",), gpu)
    cam = _cam(t["K"], t["w2v"], t["K_tof"], t["w2v_tof"])
    p3 = torch.empty((3, 37, 53), device=gpu)
    p2 = torch.empty((2, 37, 53), device=gpu)
    _lib.check(lib.gft_flow_points(_lib.raw_stream(gpu), 37, 53, t["depth"].data_ptr(), t["K"].data_ptr(), t["w2v"].data_ptr(),
                                   t["K_tof"].data_ptr(), t["w2v_tof"].data_ptr(), p3.data_ptr(), p2.data_ptr()))
    q3 = flow.distance_to_points3d(t["depth"], cam)
    assert torch.equal(p3, q3)
    q2 = flow.project_points(q3, cam)
    assert float((p2 - q2).abs().max()) <= 1e-6 * float(q2.abs().max())


@pytest.mark.gpu
def test_bit_reproducible(gpu):
    t = _dev_inputs(random_case(240, 320, 11), ("fwd", "bwd"), gpu)
    a = _fused(t, ("fwd", "bwd"), (1.0, 0.5))
    b = _fused(t, ("fwd", "bwd"), (1.0, 0.5))
    assert a[0] == b[0] and a[1] == b[1]
    assert all(torch.equal(a[2][d], b[2][d]) for d in ("fwd", "bwd"))


@pytest.mark.gpu
def test_no_host_sync(gpu):
    from gftorf_amd import flow
    t = _dev_inputs(random_case(240, 320, 12), ("fwd", "bwd"), gpu)
    cam = _cam(t["K"], t["w2v"], t["K_tof"], t["w2v_tof"], t["gt_fwd"], t["gt_bwd"])
    ff = t["flow3d_fwd"].clone().requires_grad_()
    fb = t["flow3d_bwd"].clone().requires_grad_()
    flow.flow_loss(t["depth"], cam, ff, fb)          # warm-up: the library's first load is not the question
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        f, b = flow.flow_loss(t["depth"], cam, ff, fb)
        (0.01 * (f + b)).backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert ff.grad is not None and fb.grad is not None


@pytest.mark.gpu
def test_captured_flow_term_follows_new_cameras(gpu):
    """scene_flow_l2 + backward captured on static tensors; replays after copy_-ing another camera (all four matrices),
    depth, flows and ground truth into them equal eager calls on the same values bit for bit"""
    from gftorf_amd import flow
    H, W = 48, 64
    keys = ["depth", "K", "w2v", "K_tof", "w2v_tof", "gt_fwd", "gt_bwd"]
    first = _dev_inputs(random_case(H, W, 100), ("fwd", "bwd"), gpu)
    static = {k: first[k].clone() for k in keys}
    ff = first["flow3d_fwd"].clone().requires_grad_()
    fb = first["flow3d_bwd"].clone().requires_grad_()

    def step(s, a, b):
        lf, lb = flow.scene_flow_l2(s["depth"], s["K"], s["w2v"], s["K_tof"], s["w2v_tof"], a, s["gt_fwd"], b, s["gt_bwd"])
        (lf + 0.5 * lb).backward()
        return torch.stack([lf.detach(), lb.detach()])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            ff.grad = fb.grad = None
            step(static, ff, fb)
    torch.cuda.current_stream().wait_stream(side)
    ff.grad = fb.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(static, ff, fb)
    for seed in (101, 102, 103):
        new = _dev_inputs(random_case(H, W, seed), ("fwd", "bwd"), gpu)
        with torch.no_grad():
            for k in keys:
                static[k].copy_(new[k])
            ff.copy_(new["flow3d_fwd"])
            fb.copy_(new["flow3d_bwd"])
        graph.replay()
        torch.cuda.synchronize()
        a = new["flow3d_fwd"].clone().requires_grad_()
        b = new["flow3d_bwd"].clone().requires_grad_()
        eager = step(new, a, b)
        assert torch.equal(out, eager), seed
        assert torch.equal(ff.grad, a.grad) and torch.equal(fb.grad, b.grad), seed
    assert float(out[0]) > 0 and float(out[1]) > 0


@pytest.mark.gpu
def test_ftorf_iteration(gpu):
    """The flow term of an ftorf iteration (train.py:243-261): the depth of a ToF-camera render, two colors_precomp renders
    of per-Gaussian 3-D flows on detached geometry (render_flow), flow_loss, backward.  The per-Gaussian flow gradients
    equal those of the same graph with the loss in stock torch (fp32, the formulas above)."""
    from gftorf_amd import GaussianRasterizer, flow
    P, W, H = 20_000, 320, 240
    scene = Hh.small_scene(P=P, W=W, H=H, seed=47, scale_lo=0.004, scale_hi=0.03, opacity=0.3,
                           w2c=Hh.synth.look_at_w2c(0.05, -0.02, 0.0, (0.05, 0.0, 0.1)))
    g = scene["gaussians"]
    geo = {k: torch.tensor(g[k], dtype=torch.float32, device=gpu) for k in ("means3D", "opacities", "scales", "rotations",
                                                                           "shs", "shs_p")}
    rast = GaussianRasterizer(raster_settings=Hh.gpu_settings(scene, gpu))
    flow_rast = GaussianRasterizer(raster_settings=Hh.gpu_settings(scene, gpu, bg=torch.zeros((7, H, W), device=gpu)))
    m2 = torch.zeros((P, 3), device=gpu)
    depth = rast(means3D=geo["means3D"], means2D=m2, opacities=geo["opacities"], shs=geo["shs"], shs_p=geo["shs_p"],
                 scales=geo["scales"], rotations=geo["rotations"], phase_offset=scene["phase_offset"],
                 dc_offset=scene["dc_offset"])[2].detach()
    assert depth.shape == (1, H, W) and float(depth.max()) > 0
    cam = scene["cam"]
    fx = W / (2 * cam["tanfovx"])
    K = torch.tensor([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], dtype=torch.float32, device=gpu)
    w2v = torch.tensor(cam["viewmatrix"], device=gpu)
    gen = torch.Generator().manual_seed(8)
    per_g = {d: (0.05 * torch.randn((P, 3), generator=gen)).to(gpu) for d in ("fwd", "bwd")}
    gt = {d: (2.0 * torch.randn((2, H, W), generator=gen)).to(gpu) for d in ("fwd", "bwd")}
    c = _cam(K, w2v, K, w2v, gt["fwd"], gt["bwd"])

    def render_flow(x):
        return flow_rast(means3D=geo["means3D"], means2D=m2, opacities=geo["opacities"], colors_precomp=x,
                         scales=geo["scales"], rotations=geo["rotations"])[0]

    def iteration(fused):
        leaves = {d: per_g[d].clone().requires_grad_() for d in per_g}
        f3 = {d: render_flow(leaves[d]) for d in leaves}
        if fused:
            lf, lb = flow.flow_loss(depth, c, f3["fwd"], f3["bwd"])
        else:
            p3 = ref_points3d(depth, K, w2v)
            p2 = ref_project(p3, K, w2v)
            lf, lb = (((ref_project(p3 + f3[d], K, w2v) - p2) - gt[d]).square().mean() for d in ("fwd", "bwd"))
        (0.01 * (lf + lb)).backward()
        torch.cuda.synchronize()
        return float(lf.detach()), float(lb.detach()), {d: leaves[d].grad.detach().clone() for d in leaves}

    lf, lb, gf = iteration(True)
    rf, rb, gs = iteration(False)
    assert abs(lf - rf) <= 1e-5 * rf and abs(lb - rb) <= 1e-5 * rb, (lf, rf, lb, rb)
    for d in gs:
        assert float(gs[d].abs().max()) > 0, d
        e = float((gf[d] - gs[d]).abs().max() / gs[d].abs().max())
        _note("ftorf per-Gaussian grad rel-max", e)
        assert e <= 1e-4, (d, e)
