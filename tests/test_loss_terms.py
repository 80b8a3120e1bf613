"""gftorf_amd.loss's pixel terms (l1_loss, weighted_l1_loss, weighted_l1_loss_quad, weighted_l2_loss_quad; utils/loss_utils.py
:17-33) alone and fused with SSIM (image_term), against the reference's values and gradients (tests/golden/loss.npz,
tests/golden/make_golden_loss.py) and against the formulas restated in float64 on the CPU; composed with the rasterizer
in a torf-shaped iteration, and captured in a graph."""
import os
from math import exp

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as Hh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss.npz")
KINDS = ["l2", "l1", "weighted_l1", "weighted_l1_quad", "weighted_l2_quad"]


# ---- the float64 restatement ---------------------------------------------------------------------------------------

def ref_pixel(kind, a, b, e=None, n=None):
    """utils/loss_utils.py:17-33, 51-53 (weights detached)"""
    if kind == "l1":
        return (a - b).abs().mean()
    if kind == "l2":
        return ((a - b) ** 2).mean()
    if kind == "weighted_l1":
        n = a.shape[0] if n is None else n
        w = e + torch.sqrt((a ** 2).sum(0)).detach()
        return ((a[:n] - b[:n]) / w).abs().mean()
    w = e + a.detach().abs()
    r = (a - b) / w
    return r.abs().mean() if kind == "weighted_l1_quad" else (r * r).mean()


def ref_ssim(a, b, size=11, sigma=1.5):
    """utils/loss_utils.py:76-123: the 1-D weights normalised in fp32, the 2-D window their outer product in fp32, zero
    padding, groups = channels"""
    g = torch.tensor([exp(-(x - size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(size)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    Cn = a.shape[0]
    win = (g @ g.t()).to(a.dtype).expand(Cn, 1, size, size).contiguous().to(a.device)
    a4, b4 = a.unsqueeze(0), b.unsqueeze(0)
    blur = lambda x: F.conv2d(x, win, padding=size // 2, groups=Cn)
    mu1, mu2 = blur(a4), blur(b4)
    s1, s2, s12 = blur(a4 * a4) - mu1 * mu1, blur(b4 * b4) - mu2 * mu2, blur(a4 * b4) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean()


def ref_value_grad(f, a_np, b_np):
    a = torch.tensor(a_np, dtype=torch.float64, requires_grad=True)
    v = f(a, torch.tensor(b_np, dtype=torch.float64))
    v.backward()
    return float(v.detach()), a.grad.numpy()


def golden_cases():
    z = np.load(GOLDEN)
    for pair in ("rgb", "quad", "tof", "equal"):
        a, b, e = z[pair + "_a"], z[pair + "_b"], float(z[pair + "_e"])
        fns = [(k, k, None) for k in KINDS] + [("ssim", "ssim", None)]
        if pair == "rgb":
            fns.append(("weighted_l1_n2", "weighted_l1", 2))
        for name, kind, n in fns:
            yield pair, name, kind, n, a, b, e, float(z["%s_%s" % (pair, name)]), z["%s_%s_grad" % (pair, name)]


def test_restatement_reproduces_the_golden_vectors():
    seen = 0
    for pair, name, kind, n, a, b, e, v, g in golden_cases():
        f = ref_ssim if kind == "ssim" else (lambda x, y, kind=kind, n=n: ref_pixel(kind, x, y, e, n))
        rv, rg = ref_value_grad(f, a, b)
        assert abs(rv - v) <= 1e-12, (pair, name, rv, v)
        assert np.abs(rg - g).max() <= 1e-12, (pair, name)
        seen += 1
    assert seen == 4 * 6 + 1


def test_new_functions_reject_cpu_tensors():
    from gftorf_amd import loss
    a, b = torch.zeros(2, 8, 8), torch.zeros(2, 8, 8)
    calls = [lambda: loss.l1_loss(a, b), lambda: loss.weighted_l1_loss(a, b, 0.1, 2),
             lambda: loss.weighted_l1_loss_quad(a, b, 0.1), lambda: loss.weighted_l2_loss_quad(a, b, 0.1)]
    for kind in KINDS:
        for wd in (0.0, 0.2):
            calls.append(lambda kind=kind, wd=wd: loss.image_term(a, b, kind, 0.8, wd, e=0.1))
    for c in calls:
        with pytest.raises(RuntimeError, match="HIP device only"):
            c()


def test_image_term_rejects_bad_arguments():
    from gftorf_amd import loss
    a, b = torch.zeros(2, 8, 8), torch.zeros(2, 8, 8)
    with pytest.raises(ValueError, match="pixel must be one of"):
        loss.image_term(a, b, "l3", 1.0, 0.0)
    with pytest.raises(ValueError, match="needs its weight offset"):
        loss.image_term(a, b, "weighted_l1", 1.0, 0.0)
    with pytest.raises(ValueError, match="weighted_l1' only"):
        loss.image_term(a, b, "l1", 1.0, 0.0, num_channels=1)
    with pytest.raises(NotImplementedError):
        loss.image_term(a, b.requires_grad_(), "l1", 1.0, 0.0)


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _call(kind, a, b, e, n, w_pixel, w_dssim):
    from gftorf_amd import loss
    return loss.image_term(a, b, kind, w_pixel, w_dssim, e=e if kind.startswith("weighted") else None,
                           num_channels=n)


def _drop_in(kind, a, b, e, n):
    from gftorf_amd import loss
    if kind == "l1":
        return loss.l1_loss(a, b)
    if kind == "l2":
        return loss.l2_loss(a, b)
    if kind == "weighted_l1":
        return loss.weighted_l1_loss(a, b, e, a.shape[-3] if n is None else n)
    return {"weighted_l1_quad": loss.weighted_l1_loss_quad, "weighted_l2_quad": loss.weighted_l2_loss_quad}[kind](a, b, e)


def _partials(kind, a, b, e, n):
    """[ssim mean, pixel mean] straight from gft_image_loss_forward's partials"""
    from gftorf_amd import _lib, loss
    lib = _lib.load()
    Cn, H, W = a.shape
    n = Cn if n is None else n
    blocks = int(lib.gft_ssim_blocks(Cn, H, W))
    p = torch.empty((blocks, 2), device=a.device)
    with _lib.on_device(a.device):
        _lib.check(lib.gft_image_loss_forward(_lib.raw_stream(a.device), loss.PIXEL_KINDS[kind], Cn, H, W, n, e, a.data_ptr(),
                                              b.data_ptr(), loss._WEIGHTS, None, p.data_ptr()))
    s = p.double().sum(0).cpu()
    return float(s[0]) / (Cn * H * W), float(s[1]) / (n * H * W)


def _check_kind(kind, a_np, b_np, e, n, pix_ref, gpix_ref, ssim_ref, gssim_ref, dev, what):
    a_d, b_d = torch.tensor(a_np, device=dev), torch.tensor(b_np, device=dev)
    # the kernel's two sums
    s, p = _partials(kind, a_d, b_d, e if kind.startswith("weighted") else 0.0, n)
    assert abs(s - ssim_ref) <= 2e-6, (what, kind, s, ssim_ref)
    assert abs(p - pix_ref) <= 1e-6 * abs(pix_ref), (what, kind, p, pix_ref)
    up = 2.5                                     # an upstream gradient other than 1
    # standalone (the drop-in: pixel-only kernels)
    a = a_d.clone().requires_grad_()
    v = _drop_in(kind, a, b_d, e, n)
    assert v.dim() == 0
    (up * v).backward()
    assert abs(float(v.detach()) - pix_ref) <= 1e-6 * abs(pix_ref), (what, kind, float(v.detach()), pix_ref)
    g = a.grad.double().cpu().numpy()
    assert np.abs(g - up * gpix_ref).max() <= 2e-5 * np.abs(up * gpix_ref).max(), (what, kind)
    # w_dssim == 0 is the pixel term alone
    a0 = a_d.clone().requires_grad_()
    v0 = _call(kind, a0, b_d, e, n, 0.7, 0.0)
    (up * v0).backward()
    torch.testing.assert_close(v0, 0.7 * v.detach(), rtol=1e-6, atol=0)
    torch.testing.assert_close(a0.grad, 0.7 * a.grad, rtol=1e-5, atol=1e-12)
    # fused with SSIM
    wp, wd = 0.8, 0.2
    af = a_d.clone().requires_grad_()
    vf = _call(kind, af, b_d, e, n, wp, wd)
    (up * vf).backward()
    ref = wp * pix_ref + wd * (1.0 - ssim_ref)
    assert abs(float(vf.detach()) - ref) <= 1e-6 * wp * abs(pix_ref) + 2e-6 * wd + 1e-7, (what, kind, float(vf.detach()), ref)
    gref = up * (wp * gpix_ref - wd * gssim_ref)
    assert np.abs(af.grad.double().cpu().numpy() - gref).max() <= 2e-5 * np.abs(gref).max(), (what, kind)
    return a.grad


@pytest.mark.gpu
def test_every_kind_matches_the_golden_vectors(gpu):
    cases = list(golden_cases())
    for pair in ("rgb", "quad", "tof", "equal"):
        ss = [c for c in cases if c[0] == pair and c[1] == "ssim"][0]
        for pr, name, kind, n, a, b, e, v, g in cases:
            if pr != pair or kind == "ssim":
                continue
            grad = _check_kind(kind, a, b, e, n, v, g, ss[7], ss[8], gpu, pair + "/" + name)
            if pair == "equal" and kind != "l2" and kind != "weighted_l2_quad":
                # |.|'s derivative at 0 is 0: exactly 0 on the pixels where the images agree
                eq = (a == b).all(0)
                assert eq.sum() == 8 * 12
                assert (grad[:, torch.tensor(eq, device=grad.device)] == 0).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 240, 320), (2, 240, 320), (1, 240, 320), (3, 37, 53), (7, 5, 70)])
def test_every_kind_matches_the_float64_formulas(shape, gpu):
    rng = np.random.default_rng(sum(shape) + 5)
    yy, xx = np.meshgrid(np.linspace(0, 3, shape[1]), np.linspace(0, 4, shape[2]), indexing="ij")
    base = np.stack([np.sin(yy * (c + 1)) * np.cos(xx * (c + 2)) for c in range(shape[0])])
    a_np = (0.5 * base + 0.1 * rng.normal(size=shape)).astype(np.float32)
    b_np = (0.5 * base + 0.05 * rng.normal(size=shape) + 0.02).astype(np.float32)
    b_np[:, :4, :6] = a_np[:, :4, :6]
    ssim_ref, gssim_ref = ref_value_grad(ref_ssim, a_np, b_np)
    e = 0.1
    ns = [(k, None) for k in KINDS]
    if shape[0] > 1:
        ns.append(("weighted_l1", shape[0] - 1 if shape[0] < 4 else 4))     # n < C
    for kind, n in ns:
        v, g = ref_value_grad(lambda x, y: ref_pixel(kind, x, y, e, n), a_np, b_np)
        grad = _check_kind(kind, a_np, b_np, e, n, v, g, ssim_ref, gssim_ref, gpu, str(shape))
        if n is not None:
            assert (grad[n:] == 0).all()
        if kind in ("l1", "weighted_l1", "weighted_l1_quad"):
            assert (grad[:n, :4, :6] == 0).all()


@pytest.mark.gpu
def test_image_term_l2_is_weighted_loss(gpu):
    from gftorf_amd import loss
    gen = torch.Generator().manual_seed(21)
    shape = (2, 96, 128)
    gt = torch.rand(shape, generator=gen).to(gpu)
    img0 = (gt.cpu() + 0.1 * torch.randn(shape, generator=gen)).to(gpu)
    a, b = img0.clone().requires_grad_(), img0.clone().requires_grad_()
    one = loss.weighted_loss(a, gt, 0.8, 0.2)
    two = loss.image_term(b, gt, "l2", 0.8, 0.2)
    (3.0 * one).backward()
    (3.0 * two).backward()
    assert torch.equal(one, two) and torch.equal(a.grad, b.grad)


@pytest.mark.gpu
def test_input_rules(gpu):
    from gftorf_amd import loss
    gen = torch.Generator().manual_seed(5)
    phasor = torch.rand((7, 40, 56), generator=gen).to(gpu).requires_grad_()
    gt = torch.rand((4, 40, 56), generator=gen).to(gpu)
    perm = torch.tensor([2, 0, 3, 1], device=gpu)
    # train.py:214-215's view of the quad planes: non-contiguous, [1, 1, H, W] after unsqueeze
    y = gt[1].unsqueeze(0)
    for wd in (0.0, 0.2):
        x = phasor[3:][perm][1].unsqueeze(0)
        v = loss.image_term(x, y, "weighted_l2_quad", 0.8, wd, e=0.1)
        (g,) = torch.autograd.grad(v, phasor)
        xr = phasor.detach()[3:][perm][1].unsqueeze(0).double().cpu().requires_grad_()
        vr = 0.8 * ref_pixel("weighted_l2_quad", xr, y.double().cpu(), 0.1) + wd * (1 - ref_ssim(xr, y.double().cpu()))
        (gr,) = torch.autograd.grad(vr, xr)
        assert abs(float(v.detach()) - float(vr.detach())) < 2e-6
        gfull = torch.zeros((7, 40, 56), dtype=torch.float64)
        gfull[3 + int(perm[1])] = gr[0]
        assert (g.double().cpu() - gfull).abs().max() <= 2e-5 * gfull.abs().max()
    # [1, C, H, W] in, [1, C, H, W] gradient out
    a = torch.rand((1, 3, 20, 30), device=gpu, requires_grad=True)
    loss.image_term(a, torch.rand((1, 3, 20, 30), device=gpu), "l1", 1.0, 0.2).backward()
    assert a.grad.shape == (1, 3, 20, 30)
    with pytest.raises(NotImplementedError):
        loss.l1_loss(a, torch.rand((1, 3, 20, 30), device=gpu, requires_grad=True))


def _torch_ssim32(a, b):
    return ref_ssim(a, b)           # the same formulas on the device in fp32: stock torch's grouped convolutions


@pytest.mark.gpu
def test_torf_iteration_after_tof_iters(gpu):
    """The colour term (l1 + SSIM) and the ToF term (l2 + SSIM) of a torf iteration after tof_iters (train.py:205-206, 228)
    on a colour camera and a ToF camera over the same Gaussians: gradients on the leaves through image_term equal those of
    the stock-torch fp32 formulas."""
    from gftorf_amd import GaussianRasterizer, loss, synth
    P, W, H = 20_000, 320, 240
    cams = [synth.look_at_w2c(0.05, -0.02, 0.0, (0.05, 0.0, 0.1)), synth.look_at_w2c(-0.08, 0.03, 0.01, (-0.1, 0.02, 0.15))]
    scenes = [Hh.small_scene(P=P, W=W, H=H, seed=43, scale_lo=0.004, scale_hi=0.03, opacity=0.2, w2c=c) for c in cams]
    g = scenes[0]["gaussians"]
    leaf = {k: torch.tensor(v, dtype=torch.float32, device=gpu, requires_grad=True) for k, v in g.items() if v is not None}
    m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
    rasts = [GaussianRasterizer(raster_settings=Hh.gpu_settings(sc, gpu)) for sc in scenes]

    def render(i):
        return rasts[i](means3D=leaf["means3D"], means2D=m2, opacities=leaf["opacities"], shs=leaf["shs"],
                        shs_p=leaf["shs_p"], scales=leaf["scales"], rotations=leaf["rotations"],
                        phase_offset=scenes[i]["phase_offset"], dc_offset=scenes[i]["dc_offset"])

    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        c0, t0 = render(0)[0], render(1)[1][:2]
        gt_c = (0.9 * c0 + 0.05 + 0.03 * torch.randn(c0.shape, generator=gen).to(gpu)).contiguous()
        gt_t = (1.1 * t0 + 0.02 * torch.randn(t0.shape, generator=gen).to(gpu)).contiguous()
    lam_color, lam_tof, lam_dssim = 1.0, 1.0, 0.2

    def iteration(fused):
        for v in leaf.values():
            v.grad = None
        image, tof = render(0)[0], render(1)[1][:2]
        if fused:
            L = (loss.image_term(image, gt_c, "l1", lam_color * (1 - lam_dssim), lam_color * lam_dssim)
                 + loss.image_term(tof, gt_t, "l2", lam_tof * (1 - lam_dssim), lam_tof * lam_dssim))
        else:
            L = (lam_color * ((1 - lam_dssim) * (image - gt_c).abs().mean() + lam_dssim * (1 - _torch_ssim32(image, gt_c)))
                 + lam_tof * ((1 - lam_dssim) * ((tof - gt_t) ** 2).mean() + lam_dssim * (1 - _torch_ssim32(tof, gt_t))))
        L.backward()
        torch.cuda.synchronize()
        return float(L), {k: v.grad.detach().clone() for k, v in leaf.items()}

    lf, gf = iteration(True)
    ls, gs = iteration(False)
    assert abs(lf - ls) <= 1e-5 * abs(ls)
    for k in gs:
        ref = gs[k]
        assert ref.abs().max() > 0, k
        assert float((gf[k] - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), k


@pytest.mark.gpu
def test_captured_image_terms_follow_new_images(gpu):
    """image_term forward + backward (one fused term, one pixel-only term) captured in a graph: replays after new image
    contents equal eager calls bit for bit."""
    from gftorf_amd import loss
    shape_c, shape_t = (3, 64, 80), (3, 48, 72)
    img_c = torch.zeros(shape_c, device=gpu, requires_grad=True)
    img_t = torch.zeros(shape_t, device=gpu, requires_grad=True)
    gt_c, gt_t = torch.zeros(shape_c, device=gpu), torch.zeros(shape_t, device=gpu)
    gen = torch.Generator().manual_seed(9)

    def fill(seed):
        gen.manual_seed(seed)
        with torch.no_grad():
            for t in (img_c, img_t, gt_c, gt_t):
                t.copy_(torch.rand(t.shape, generator=gen).to(gpu))

    def step(a, b):
        L = loss.image_term(a, gt_c, "l1", 0.8, 0.2) + loss.image_term(b, gt_t, "weighted_l1", 1.0, 0.0, e=0.1, num_channels=2)
        L.backward()
        return L

    fill(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            img_c.grad = img_t.grad = None
            step(img_c, img_t)
    torch.cuda.current_stream().wait_stream(s)
    img_c.grad = img_t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_L = step(img_c, img_t)
    static_L = static_L.detach()
    for seed in (1, 2, 3):
        fill(seed)
        graph.replay()
        torch.cuda.synchronize()
        a = img_c.detach().clone().requires_grad_()
        b = img_t.detach().clone().requires_grad_()
        L = step(a, b)
        assert torch.equal(static_L, L.detach()), seed
        assert torch.equal(img_c.grad, a.grad) and torch.equal(img_t.grad, b.grad), seed
        assert float(img_t.grad[2].abs().max()) == 0.0
