"""The ToF phase / DC offsets read from device memory (C ABI 15: gft_forward_io / gft_backward_io .phase_offset_dev,
.dc_offset_dev).  A one-element float32 tensor on the device -- the reference's learnable ``_phase_offset`` / ``_dc_offset``
(gaussian_model.py:225-226) -- goes to the kernels by address: no ``.item()``, so an eager call never waits for the host and a
captured iteration follows the values the optimiser writes between replays.  Every result must equal the host path (a
Python float, a float64 or CPU tensor read with ``.item()``) for the same number, bit for bit."""
import contextlib

import numpy as np
import pytest
import torch

import helpers as Hh

pytestmark = pytest.mark.gpu

PH, DC = -2.7, 0.4           # (the second pair of values; the scenes carry 0.1 / 0.05)


def _abi():
    from gftorf_amd import _lib
    assert _lib.ABI_VERSION >= 15


@contextlib.contextmanager
def _modes(binning=-1, render=-1, deterministic=True, reuse=False):
    """Binning and forward-blend kernels, the deterministic backward, and whether gradient tensors are kept from call to
    call.  (Off by default: a backward into kept tensors writes the blended rows only, and the offset gradients' partial
    sums then group differently -- to the rounding of the sum, with either kind of offset.)"""
    from gftorf_amd import _lib, api
    lib = _lib.load()
    keep = api._DETERMINISTIC, api._GRADS_REUSE
    lib.gft_set_binning_mode(int(binning))
    lib.gft_set_render_mode(int(render))
    api._DETERMINISTIC = deterministic
    api._GRADS_REUSE = reuse and keep[1]
    api._grad_pool.clear()
    try:
        yield
    finally:
        api._DETERMINISTIC, api._GRADS_REUSE = keep
        api._grad_pool.clear()
        lib.gft_set_binning_mode(-1)
        lib.gft_set_render_mode(-1)


def _offset(v, kind, dev):
    """'float': a Python float; 'device': a float32 Parameter on the device (read by address); 'f64': a float64 Parameter on
    the device (read with .item(): the host path, offset gradients returned); 'cpu': a float32 tensor on the host (host path)."""
    if kind == "float":
        return v
    if kind == "cpu":
        return torch.tensor([v], dtype=torch.float32)
    return torch.nn.Parameter(torch.tensor([v], dtype=torch.float64 if kind == "f64" else torch.float32, device=dev))


def _leaves(scene, dev):
    g = scene["gaussians"]
    leaf = {k: torch.tensor(v, dtype=torch.float32, device=dev, requires_grad=True) for k, v in g.items() if v is not None}
    return leaf, torch.zeros((g["means3D"].shape[0], 3), device=dev, requires_grad=True)


def _call(rast, leaf, m2, ph, dc):
    return rast(means3D=leaf["means3D"], means2D=m2, opacities=leaf["opacities"], shs=leaf["shs"], shs_p=leaf["shs_p"],
                scales=leaf["scales"], rotations=leaf["rotations"], phase_offset=ph, dc_offset=dc)


def _ups(scene, dev):
    return [torch.tensor(scene["grads"][k], device=dev) for k in Hh.GRAD_KEYS]


def _diff(o):
    return [o[0], o[1], o[2], o[4], o[6]]


def _frame(scene, dev, kind, ph=None, dc=None):
    """One forward + backward through GaussianRasterizer with the offsets as `kind`: (outputs, gradients) as host arrays."""
    from gftorf_amd import GaussianRasterizer
    ph = scene["phase_offset"] if ph is None else ph
    dc = scene["dc_offset"] if dc is None else dc
    leaf, m2 = _leaves(scene, dev)
    p, d = _offset(ph, kind, dev), _offset(dc, kind, dev)
    o = _call(GaussianRasterizer(Hh.gpu_settings(scene, dev, optimize_offsets=True)), leaf, m2, p, d)
    torch.autograd.backward(_diff(o), _ups(scene, dev))
    torch.cuda.synchronize()
    outs = [t.detach().cpu().numpy() for t in o]
    grads = {k: v.grad.cpu().numpy() for k, v in leaf.items()}
    grads["means2D"] = m2.grad.cpu().numpy()
    if kind in ("device", "f64"):
        grads["phase_offset"] = p.grad.double().cpu().numpy()
        grads["dc_offset"] = d.grad.double().cpu().numpy()
    return outs, grads


def _same(a, b, what):
    """Outputs and the gradients `b` has: equal bit for bit."""
    (oa, ga), (ob, gb) = a, b
    for name, x, y in zip(Hh.OUT_NAMES, oa, ob):
        np.testing.assert_array_equal(x, y, err_msg="%s: %s" % (what, name))
    for k in gb:
        np.testing.assert_array_equal(ga[k], gb[k], err_msg="%s: grad %s" % (what, k))


SCENES = {
    "small": dict(P=400, seed=3),
    "dense": dict(P=20_000, W=128, H=96, seed=21, scale_lo=0.005, scale_hi=0.04),
}
MODES = {
    "whole_frame": dict(binning=0, render=0),
    "tile_pull": dict(binning=1, render=0),
    "segmented": dict(binning=1, render=1),          # (fewer than 768 tiles: the segment-parallel forward)
}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(SCENES))
def test_device_offsets_equal_the_host_path(name, mode, gpu):
    """Outputs and every gradient, the two offset gradients included, bit for bit against the same call with the offsets
    read on the host (Python floats; float64 tensors for the offset gradients), at two pairs of values, in the deterministic
    backward; then three calls in a row, which hand the backward kept gradient tensors (cfg.grads_zeroed 2 / 3)."""
    _abi()
    from gftorf_amd import api
    scene = Hh.small_scene(**SCENES[name])
    with _modes(**MODES[mode]):
        for ph, dc in ((None, None), (PH, DC)):
            host = _frame(scene, gpu, "f64", ph, dc)
            flt = _frame(scene, gpu, "float", ph, dc)
            _same(host, flt, "%s %s: float" % (mode, ph))      # (no offset gradients with floats)
            dev = _frame(scene, gpu, "device", ph, dc)
            _same(dev, host, "%s %s" % (mode, ph))
    runs = {}
    for kind in ("device", "f64"):
        with _modes(reuse=True, **MODES[mode]):         # (the same history of kept tensors for both kinds)
            runs[kind] = [(_frame(scene, gpu, kind), api.last_call_stats.get("grads_reused"),
                           api.last_call_stats.get("grads_rows_only")) for _ in range(3)]
    for i, (d, h) in enumerate(zip(runs["device"], runs["f64"])):
        assert d[1:] == h[1:]
        _same(d[0], h[0], "kept gradients, call %d" % i)
    if api._GRADS_REUSE:
        assert (True, True) in [d[1:] for d in runs["device"]], runs["device"]


def test_device_offsets_against_the_oracle(oracle, gpu):
    """The device path against the CPU oracle, with the tolerances of the parity tests, at offsets other than the scene's."""
    _abi()
    scene = Hh.small_scene(P=400, seed=3)
    scene.update(phase_offset=PH, dc_offset=DC)
    f, b = Hh.run_oracle(oracle, scene)
    outs, grads = _frame(scene, gpu, "device")
    out = dict(zip(Hh.OUT_NAMES, outs))
    np.testing.assert_array_equal(out["radii"], f.radii)
    for k in ["color", "phasor", "depth", "acc", "depth_distortion"]:
        Hh.assert_close(k, f[k], out[k], rtol_max=2e-4, atol=1e-6, frac_bad=1e-3)
    for key, ref in [("means3D", "dL_dmeans3D"), ("shs", "dL_dsh"), ("shs_p", "dL_dsh_p"), ("scales", "dL_dscales"),
                     ("rotations", "dL_drotations"), ("means2D", "dL_dmeans2D")]:
        Hh.assert_close(ref, b[ref], grads[key], rtol_max=3e-4)
    Hh.assert_close("dL_dphase_offset", b["dL_dphase_offset"], grads["phase_offset"], rtol_max=3e-4, atol=1e-5)
    Hh.assert_close("dL_ddc_offset", b["dL_ddc_offset"], grads["dc_offset"], rtol_max=3e-4, atol=1e-5)


def _pair_frame(a, b, dev, kind, vals):
    from gftorf_amd import GaussianRasterizerPair
    leaf, m2 = _leaves(a, dev)
    offs = [(_offset(p, kind, dev), _offset(d, kind, dev)) for p, d in vals]
    oa, ob = GaussianRasterizerPair(Hh.gpu_settings(a, dev, optimize_offsets=True), Hh.gpu_settings(b, dev, optimize_offsets=True))(
        means3D=leaf["means3D"], means2D=m2, opacities=leaf["opacities"], shs=leaf["shs"], shs_p=leaf["shs_p"],
        scales=leaf["scales"], rotations=leaf["rotations"], phase_offset=(offs[0][0], offs[1][0]), dc_offset=(offs[0][1], offs[1][1]))
    torch.autograd.backward(_diff(oa) + _diff(ob), _ups(a, dev) + _ups(b, dev))
    torch.cuda.synchronize()
    outs = [t.detach().cpu().numpy() for t in tuple(oa) + tuple(ob)]
    grads = {k: v.grad.cpu().numpy() for k, v in leaf.items()}
    grads["means2D"] = m2.grad.cpu().numpy()
    for v in range(2):
        grads["phase_%d" % v] = offs[v][0].grad.double().cpu().numpy()
        grads["dc_%d" % v] = offs[v][1].grad.double().cpu().numpy()
    return outs, grads


def _two_views():
    from gftorf_amd import synth
    cams = [synth.look_at_w2c(0.05, -0.02, 0.0, (0.05, 0.0, 0.1)), synth.look_at_w2c(-0.08, 0.03, 0.01, (-0.1, 0.02, 0.15))]
    return [Hh.small_scene(P=3000, W=96, H=64, seed=41, scale_lo=0.01, scale_hi=0.06, w2c=c) for c in cams]


def test_pair_device_offsets_equal_the_host_path(gpu):
    """GaussianRasterizerPair (the second view's backward adds to the first one's gradient tensors: cfg.grads_accumulate):
    per-view device offsets equal the host path bit for bit, each view's own offset gradients included."""
    _abi()
    a, b = _two_views()
    with _modes():
        for vals in (((0.0, 0.0), (0.1, 0.05)), ((0.3, -0.2), (PH, DC))):
            _same(_pair_frame(a, b, gpu, "device", vals), _pair_frame(a, b, gpu, "f64", vals), "pair %s" % (vals,))


def test_offset_semantics(gpu):
    """An in-place edit of a device offset between forward and backward raises (the backward would read the new value); a
    second backward through one forward reads the same offsets; CPU and float64 offsets still work through the host path."""
    _abi()
    from gftorf_amd import GaussianRasterizer
    scene = Hh.small_scene(P=400, seed=5)
    rast = GaussianRasterizer(Hh.gpu_settings(scene, gpu, optimize_offsets=True))
    leaf, m2 = _leaves(scene, gpu)
    ph, dc = _offset(0.1, "device", gpu), _offset(0.05, "device", gpu)
    o = _call(rast, leaf, m2, ph, dc)
    with torch.no_grad():
        ph.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.backward(_diff(o), _ups(scene, gpu))
    with torch.no_grad():
        ph.sub_(1.0)

    with _modes():
        leaf, m2 = _leaves(scene, gpu)
        o = _call(rast, leaf, m2, ph, dc)
        loss = sum((t * u).sum() for t, u in zip(_diff(o), _ups(scene, gpu)))
        params = list(leaf.values()) + [ph, dc]
        first = [g.clone() for g in torch.autograd.grad(loss, params, retain_graph=True)]
        second = torch.autograd.grad(loss, params)
        for x, y in zip(first, second):
            torch.testing.assert_close(y, x, rtol=1e-5, atol=1e-6 * float(x.abs().max()))
        ref = _frame(scene, gpu, "f64")
        for kind in ("cpu", "f64"):
            _same(ref, _frame(scene, gpu, kind), kind)


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fn()
    return graph, static


def test_captured_call_follows_offset_parameters(gpu):
    """Forward and backward of the ToF camera captured with Parameter offsets; new values written into the Parameters (copy_
    under no_grad) reach the replay: outputs, offset gradients and per-Gaussian gradients equal an eager call at the new
    values bit for bit (deterministic backward).  Then the same with GaussianRasterizerPair."""
    _abi()
    from gftorf_amd import api, GaussianRasterizer, GaussianRasterizerPair
    scene = Hh.small_scene(P=20_000, W=128, H=96, seed=21, scale_lo=0.005, scale_hi=0.04)
    rast = GaussianRasterizer(Hh.gpu_settings(scene, gpu, optimize_offsets=True))
    a, b = _two_views()
    pair = GaussianRasterizerPair(Hh.gpu_settings(a, gpu, optimize_offsets=True), Hh.gpu_settings(b, gpu, optimize_offsets=True))
    api._instance_hint.clear()
    try:
        with _modes():
            # ---- one camera
            leaf, m2 = _leaves(scene, gpu)
            ph, dc = _offset(0.1, "device", gpu), _offset(0.05, "device", gpu)
            params = list(leaf.values()) + [m2, ph, dc]
            ups = _ups(scene, gpu)

            def single():
                for p in params:
                    p.grad = None
                o = _call(rast, leaf, m2, ph, dc)
                torch.autograd.backward(_diff(o), ups)
                return o

            single()                                            # eager frame of the shape: the capture sizes its buffers from it
            torch.cuda.synchronize()
            for p in params:
                p.grad = None
            graph, static = _capture(single)
            static_g = [p.grad for p in params]
            for p_v, d_v in ((PH, DC), (0.7, -0.3)):
                with torch.no_grad():
                    ph.copy_(torch.tensor([p_v]))
                    dc.copy_(torch.tensor([d_v]))
                graph.replay()
                torch.cuda.synchronize()
                got = [t.detach().clone() for t in static], [g.clone() for g in static_g]
                ref_o = single()
                torch.cuda.synchronize()
                for x, y in zip(got[0], ref_o):
                    assert torch.equal(x, y.detach()), p_v
                for p, g in zip(params, got[1]):
                    assert torch.equal(g, p.grad), (p_v, tuple(p.shape))
                for p in params:
                    p.grad = None
                del ref_o
            del graph, static, static_g

            # ---- the camera pair
            leaf, m2 = _leaves(a, gpu)
            offs = [_offset(v, "device", gpu) for v in (0.0, 0.0, 0.1, 0.05)]
            params = list(leaf.values()) + [m2] + offs
            ups = _ups(a, gpu) + _ups(b, gpu)

            def both():
                for p in params:
                    p.grad = None
                oa, ob = pair(means3D=leaf["means3D"], means2D=m2, opacities=leaf["opacities"], shs=leaf["shs"],
                              shs_p=leaf["shs_p"], scales=leaf["scales"], rotations=leaf["rotations"],
                              phase_offset=(offs[0], offs[2]), dc_offset=(offs[1], offs[3]))
                torch.autograd.backward(_diff(oa) + _diff(ob), ups)
                return tuple(oa) + tuple(ob)

            both()
            torch.cuda.synchronize()
            for p in params:
                p.grad = None
            graph, static = _capture(both)
            static_g = [p.grad for p in params]
            with torch.no_grad():
                for t, v in zip(offs, (0.2, -0.1, PH, DC)):
                    t.copy_(torch.tensor([v]))
            graph.replay()
            torch.cuda.synchronize()
            got = [t.detach().clone() for t in static], [g.clone() for g in static_g]
            ref_o = both()
            torch.cuda.synchronize()
            for x, y in zip(got[0], ref_o):
                assert torch.equal(x, y.detach())
            for p, g in zip(params, got[1]):
                assert torch.equal(g, p.grad), tuple(p.shape)
    finally:
        api._instance_hint.clear()


def _training(dev, graph, iters=12, open_at=5):
    """A small loop of the training shape: ToF render with Parameter offsets, L2 loss against a fixed target, backward,
    FusedAdam(capturable) over the Gaussians and the two offsets.  The offsets' learning rates are 0 until `open_at`
    (optimize_offset_start), then set and refresh_lr()'d.  Returns the losses and the offsets after every iteration."""
    from gftorf_amd import FusedAdam, GaussianRasterizer, api
    scene = Hh.small_scene(P=3000, W=96, H=64, seed=7, scale_lo=0.01, scale_hi=0.06)
    rast = GaussianRasterizer(Hh.gpu_settings(scene, dev, optimize_offsets=True))
    g = scene["gaussians"]
    par = {k: torch.nn.Parameter(torch.tensor(g[k], dtype=torch.float32, device=dev))
           for k in ("means3D", "opacities", "shs", "shs_p", "scales", "rotations")}
    par["phase_offset"] = torch.nn.Parameter(torch.tensor([0.1], device=dev))
    par["dc_offset"] = torch.nn.Parameter(torch.tensor([0.05], device=dev))
    m2 = torch.zeros((g["means3D"].shape[0], 3), device=dev, requires_grad=True)
    lrs = dict(means3D=1e-4, opacities=1e-3, shs=1e-3, shs_p=1e-3, scales=1e-3, rotations=1e-3, phase_offset=0.0, dc_offset=0.0)
    opt = FusedAdam([{"params": [par[k]], "lr": lrs[k], "name": k} for k in lrs], lr=0.0, eps=1e-15, capturable=graph)
    target = torch.tensor(np.random.default_rng(5).uniform(-0.5, 0.5, (7, 64, 96)), dtype=torch.float32, device=dev)

    def body():
        o = rast(means3D=par["means3D"], means2D=m2, opacities=torch.sigmoid(par["opacities"]), shs=par["shs"], shs_p=par["shs_p"],
                 scales=torch.exp(par["scales"]), rotations=torch.nn.functional.normalize(par["rotations"]),
                 phase_offset=par["phase_offset"], dc_offset=par["dc_offset"])
        loss = ((o[1] - target) ** 2).mean()
        loss.backward()
        with torch.no_grad():
            opt.step()
            opt.zero_grad(set_to_none=True)
            m2.grad = None
        return loss.detach()

    with torch.no_grad():
        par["opacities"].copy_(torch.logit(par["opacities"].clamp(1e-4, 1 - 1e-4)))
        par["scales"].copy_(torch.log(par["scales"]))
    api._instance_hint.clear()
    losses, traj, cg, static = [], [], None, None
    for it in range(1, iters + 1):
        if it == open_at:
            for gr in opt.param_groups:
                if gr["name"] in ("phase_offset", "dc_offset"):
                    gr["lr"] = 0.01
        if not graph or it <= 2:
            loss = body()
        else:
            if cg is None:
                torch.cuda.synchronize()
                cg = torch.cuda.CUDAGraph()
                with torch.cuda.graph(cg):
                    static = body()
            opt.refresh_lr()
            cg.replay()
            loss = static
        torch.cuda.synchronize()
        losses.append(float(loss))
        traj.append((float(par["phase_offset"]), float(par["dc_offset"])))
    api._instance_hint.clear()
    return np.array(losses), np.array(traj)


def test_captured_training_moves_the_offsets(gpu):
    """FusedAdam(capturable=True) holds the offsets at lr 0, then (optimize_offset_start) at lr 0.01: in the replayed
    iterations the offsets stay put, then move, as in the same loop run eagerly (losses and trajectories within the bound
    test_loop_graph.py uses for parameters)."""
    _abi()
    eager_l, eager_t = _training(gpu, graph=False)
    graph_l, graph_t = _training(gpu, graph=True)
    assert (eager_t[:4] == eager_t[0]).all() and (graph_t[:4] == graph_t[0]).all()          # lr 0: fixed
    assert np.abs(eager_t[-1] - eager_t[3]).min() > 0.005 and np.abs(graph_t[-1] - graph_t[3]).min() > 0.005   # then moving
    np.testing.assert_allclose(graph_l, eager_l, rtol=2e-3)
    moved = np.abs(eager_t[-1] - eager_t[0])
    assert (np.abs(graph_t - eager_t).max(axis=0) <= 0.05 * moved).all(), (graph_t, eager_t)


def test_eager_call_with_device_offsets_reads_nothing_on_the_host(gpu):
    """api.no_host_read with torch's sync debug mode set to "error": forward and backward with Parameter offsets after a
    warm-up frame raise nothing -- no more than the same call with float offsets (with them, .item() raised here)."""
    _abi()
    from gftorf_amd import api, GaussianRasterizer
    scene = Hh.small_scene(P=3000, W=96, H=64, seed=9)
    rast = GaussianRasterizer(Hh.gpu_settings(scene, gpu, optimize_offsets=True))
    leaf, m2 = _leaves(scene, gpu)
    ups = _ups(scene, gpu)
    keep = api.no_host_read
    api.no_host_read = True
    api._instance_hint.clear()

    def trips(ph, dc):
        o = _call(rast, leaf, m2, ph, dc)                       # warm-up frame of the shape
        torch.autograd.backward(_diff(o), ups)
        torch.cuda.synchronize()
        try:
            torch.cuda.set_sync_debug_mode("error")
            o = _call(rast, leaf, m2, ph, dc)
            torch.autograd.backward(_diff(o), ups)
            return None
        except RuntimeError as ex:
            return str(ex)
        finally:
            torch.cuda.set_sync_debug_mode(0)
            torch.cuda.synchronize()

    try:
        ph, dc = _offset(0.1, "device", gpu), _offset(0.05, "device", gpu)
        base = trips(0.1, 0.05)
        got = trips(ph, dc)
        assert got is None or got == base, (got, base)
        assert ph.grad is not None and dc.grad is not None
    finally:
        api.no_host_read = keep
        api._instance_hint.clear()
