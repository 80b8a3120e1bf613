"""Helpers of tests/test_loop_densify.py and tests/test_loop_dynamic.py: the pieces of the teacher-forced training loop that need no device -- the model from
a scene, the learning-rate schedule, the thresholds an event is given, the torch.optim.Adam twin of one step and the composed
reference of one iteration (eager activations under CPU autograd, the C oracle of the rasterizer, its gradients pushed back
through autograd: the reference tests/test_train_step.py uses), with a motion mask and the deformation network's offsets in
:func:`composed_reference_dynamic`."""
import numpy as np
import torch

from oracle import assemble_ref, densify_ref
from tests import helpers

# the reference's groups (scene/gaussian_model.py:247-272); the rest coefficients learn at a twentieth of the dc ones
LRS = {"xyz": 2e-4, "f_dc_color": 2e-3, "f_rest_color": 2e-3 / 20, "phase_f_dc": 2e-3, "phase_f_rest": 2e-3 / 20, "amp_f_dc": 2e-3,
       "amp_f_rest": 2e-3 / 20, "opacity": 1e-2, "scaling": 2e-3, "rotation": 1e-3, "f_seg_color": 1e-3}
NAMES = [name for name, _, _ in densify_ref.EagerGaussians.GROUPS]
ATTR = {name: attr for name, attr, _ in densify_ref.EagerGaussians.GROUPS}
ADAM_RTOL, ADAM_ATOL = 3e-6, 3e-7          # tests/test_optim.py: FusedAdam against torch.optim.Adam (atol times max |ref|)


def xyz_lr(it, steps=40, lr_init=LRS["xyz"], lr_final=LRS["xyz"] * 0.01):
    """get_expon_lr_func without a delay (utils/general_utils.py:41-70): log-linear from lr_init to lr_final over `steps`
    iterations -- about 11 % less every iteration, so a step that used another iteration's rate misses the Adam check."""
    t = min(max(it / steps, 0.0), 1.0)
    return float(np.exp(np.log(lr_init) * (1.0 - t) + np.log(lr_final) * t))


def perturbed(gaussians, seed=3):
    """The scene's Gaussians moved away from the truth (as tests/test_train_step.py starts its loop), the rotations off the
    unit sphere so that the normalisation inside the assembly has work to do."""
    rng = np.random.default_rng(seed)
    g = dict(gaussians)
    P = g["means3D"].shape[0]
    g["means3D"] = (g["means3D"] + rng.normal(0, 0.01, (P, 3))).astype(np.float32)
    g["opacities"] = (g["opacities"] * 0.8).astype(np.float32)
    g["scales"] = (g["scales"] * 1.15).astype(np.float32)
    g["rotations"] = (g["rotations"] * rng.uniform(0.5, 2.0, (P, 1))).astype(np.float32)
    g["shs"] = (g["shs"] * 0.8).astype(np.float32)
    g["shs_p"] = (g["shs_p"] * 0.9).astype(np.float32)
    return g


def make_model(gaussians, dev, optimizer_cls, cls=densify_ref.EagerGaussians, **optimizer_kw):
    return cls.from_scene(perturbed(gaussians), dev, optimizer_cls, LRS, **optimizer_kw)


class DynamicGaussians(densify_ref.EagerGaussians):
    """The model with the reference's motion mask: a Gaussian is dynamic where the first seg colour is above one half."""
    get_motion_mask = property(lambda self: (self._features_seg_color[:, 0] > 0.5).detach())      # gaussian_model.py:160-161


def seg_colors(P, share=0.35, on_threshold=(3, 40, 41, 700), seed=4):
    """Seg colours [P, 3] whose first column makes about `share` of the rows dynamic (1.0 against 0.0) and puts the rows
    `on_threshold` exactly on 0.5: `> 0.5` leaves them static."""
    rng = np.random.default_rng(seed)
    seg = np.zeros((P, 3), np.float32)
    seg[:, 0] = rng.random(P) < share
    seg[:, 1:] = rng.random((P, 2))
    seg[[r for r in on_threshold if r < P], 0] = 0.5
    return torch.tensor(seg)


# ---- events --------------------------------------------------------------------------------------------------------------
def thresholds(pc):
    """Thresholds taken from the model's state so that every branch of densify_and_prune selects rows: the gradient threshold
    is the median of the mean view-space gradient over the rows that were seen, `percent_dense * extent` the median of the
    largest scaling (half of the hot rows are cloned, half split), `min_opacity` the 5 % quantile of the opacity."""
    seen = pc.denom[:, 0] > 0
    grads = (pc.xyz_gradient_accum[:, 0] / pc.denom[:, 0])[seen]
    big = pc.get_scaling.detach().max(dim=1).values
    return dict(max_grad=float(grads.median()), extent=float(big.median()) / pc.percent_dense,
                min_opacity=float(torch.quantile(pc.get_opacity.detach().reshape(-1), 0.05)))


def selections(pc, th):
    """(clone mask, split mask, prune mask of the rows as they are) of densify_and_prune under `th`: the reference's
    expressions (scene/gaussian_model.py:573-579, 605-608, 629).  A cloned row's padded gradient is zero, so the split mask
    over the grown model is this one followed by False."""
    grads = pc.xyz_gradient_accum / pc.denom
    grads[grads.isnan()] = 0.0
    hot = torch.norm(grads, dim=-1) >= th["max_grad"]
    big = torch.max(pc.get_scaling.detach(), dim=1).values > pc.percent_dense * th["extent"]
    return hot & ~big, hot & big, (pc.get_opacity.detach() < th["min_opacity"]).squeeze()


def assert_same_snapshot(a, b, what):
    sa, sb = a.snapshot(), b.snapshot()
    assert set(sa) == set(sb), (what, sorted(set(sa) ^ set(sb)))
    for k in sa:
        assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), (what, k)


# ---- one Adam step ----------------------------------------------------------------------------------------------------------
def optimizer_state(pc):
    """Deep copy (CPU) of what a step reads and writes: group name -> dict(param, exp_avg, exp_avg_sq, step); the moments
    and the count are None for a group that has no state yet."""
    out = {}
    for grp in pc.optimizer.param_groups:
        p = grp["params"][0]
        st = pc.optimizer.state.get(p, None)
        has = st is not None and "exp_avg" in st
        out[grp["name"]] = dict(param=p.detach().cpu().clone(), exp_avg=st["exp_avg"].cpu().clone() if has else None,
                                exp_avg_sq=st["exp_avg_sq"].cpu().clone() if has else None, step=float(st["step"]) if has else None)
    return out


def adam_twin_step(before, grads, lrs):
    """torch.optim.Adam (CPU) started from `before` (optimizer_state), one step on `grads` (group name -> tensor; a group
    without one takes no step) under the learning rates `lrs`: the state after it, in optimizer_state's form."""
    groups, params = [], {}
    for name, s in before.items():
        params[name] = torch.nn.Parameter(s["param"].clone())
        groups.append({"params": [params[name]], "lr": float(lrs[name]), "name": name})
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for name, s in before.items():
        if s["step"] is not None:
            opt.state[params[name]] = {"step": torch.tensor(s["step"], dtype=torch.float32), "exp_avg": s["exp_avg"].clone(),
                                       "exp_avg_sq": s["exp_avg_sq"].clone()}
        if grads.get(name) is not None:
            params[name].grad = grads[name].detach().cpu().clone()
    opt.step()
    out = {}
    for name, p in params.items():
        st = opt.state.get(p, None)
        has = st is not None and "exp_avg" in st
        out[name] = dict(param=p.detach(), exp_avg=st["exp_avg"] if has else None, exp_avg_sq=st["exp_avg_sq"] if has else None,
                         step=float(st["step"]) if has else None)
    return out


def assert_adam_step(before, grads, lrs, after, what):
    """`after` (optimizer_state of the product after its step) against the torch twin's step from `before`."""
    ref = adam_twin_step(before, grads, lrs)
    for name in before:
        if grads.get(name) is None:          # no gradient: parameter and state stay as they are, bit for bit
            for k in ("param", "exp_avg", "exp_avg_sq"):
                assert (after[name][k] is None) == (before[name][k] is None), (what, name, k)
                assert before[name][k] is None or torch.equal(after[name][k], before[name][k]), (what, name, k)
            assert after[name]["step"] == before[name]["step"], (what, name)
            continue
        assert after[name]["step"] == ref[name]["step"] == (before[name]["step"] or 0.0) + 1.0, (what, name, after[name]["step"])
        for k in ("param", "exp_avg", "exp_avg_sq"):
            r = ref[name][k].numpy()
            np.testing.assert_allclose(after[name][k].numpy(), r, rtol=ADAM_RTOL, atol=ADAM_ATOL * float(np.abs(r).max()),
                                       err_msg="%s: %s of group %s" % (what, k, name))


# ---- one iteration: the composed reference ------------------------------------------------------------------------------
def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def l1_upstream(image, target, weight):
    """d(weight * mean |image - target|) / d image (torch: the sign, zero at zero)."""
    return (np.sign(np.asarray(image, np.float64) - np.asarray(target, np.float64)) * (weight / image.size)).astype(np.float32)


def composed_reference(oracle, scene, raw, up_color, up_phasor):
    """One iteration's render and gradients from the raw parameters `raw` (group name -> CPU tensor): pc.get_* eagerly
    (scene/gaussian_model.py:123-153), the eager assembly (static region, no offsets), the C oracle of the rasterizer under
    the upstream gradients `up_color` / `up_phasor`, its gradients pushed back through autograd.  Returns (oracle forward,
    gradients by group name + "ssp")."""
    cl = {k: v.detach().clone().requires_grad_(True) for k, v in raw.items() if k != "f_seg_color"}
    P = cl["xyz"].shape[0]
    ssp = torch.zeros((P, 3), requires_grad=True)
    fc = torch.cat((cl["f_dc_color"], cl["f_rest_color"]), dim=1)
    fp = torch.cat((torch.cat((cl["phase_f_dc"], cl["phase_f_rest"]), dim=1), torch.cat((cl["amp_f_dc"], cl["amp_f_rest"]), dim=1)), dim=2)
    a = assemble_ref.assemble_eager(cl["xyz"], ssp, torch.sigmoid(cl["opacity"]), torch.exp(cl["scaling"]),
                                    torch.nn.functional.normalize(cl["rotation"]), cl["rotation"], fc, fp,
                                    torch.zeros((P,), dtype=torch.bool), render_regions=("static",))
    f = _through_the_rasterizer(oracle, scene, a, up_color, up_phasor)
    out = {k: v.grad.numpy() for k, v in cl.items()}
    out["ssp"] = ssp.grad.numpy()
    return f, out


def _through_the_rasterizer(oracle, scene, a, up_color, up_phasor):
    """The C oracle of the rasterizer on the assembled inputs `a` (CPU tensors under autograd) under the upstream gradients
    `up_color` / `up_phasor`; its gradients are pushed back through `a`.  Returns the oracle's forward."""
    inputs = dict(means3D=a[0].detach().numpy(), opacities=a[2].detach().numpy(), scales=a[3].detach().numpy(),
                  rotations=a[4].detach().numpy(), shs=a[5].detach().numpy(), shs_p=a[6].detach().numpy())
    grads = {k: np.zeros_like(v) for k, v in scene["grads"].items()}
    grads["color"], grads["phasor"] = up_color, up_phasor
    sc = dict(scene, grads=grads)
    sc["cfg"] = dict(scene["cfg"], P=a[0].shape[0])
    f, b = helpers.run_oracle(oracle, sc, inputs=inputs)
    up = [b["dL_dmeans3D"], b["dL_dmeans2D"], b["dL_dopacity"], b["dL_dscales"], b["dL_drotations"], b["dL_dsh"], b["dL_dsh_p"]]
    torch.autograd.backward(list(a), [torch.tensor(np.asarray(u, np.float32).reshape(tuple(o.shape))) for u, o in zip(up, a)])
    return f


def dynamic_inputs(raw, mask, d_xyz=None, d_sh=None, render_regions=("static", "dynamic")):
    """The rasterizer's inputs of a model with a motion mask, under CPU autograd: clones of the raw parameters `raw` (group
    name -> CPU tensor) and of the network's offsets `d_xyz` [n, 3] / `d_sh` [n, 16, 3] (arrays; None: the scalar 0.0 of
    train.py:164) as leaves, pc.get_* eagerly (scene/gaussian_model.py:123-153), then the reference's assembly
    (gaussian_renderer/__init__.py:81-105; d_rot and d_sh_p are the zeros the network returns).  Returns (assembled
    tensors, leaves by group name + "ssp" + "d_xyz" + "d_sh")."""
    cl = {k: v.detach().clone().requires_grad_(True) for k, v in raw.items() if k != "f_seg_color"}
    P = cl["xyz"].shape[0]
    cl["ssp"] = torch.zeros((P, 3), requires_grad=True)
    for k, d in (("d_xyz", d_xyz), ("d_sh", d_sh)):
        if d is not None:
            cl[k] = torch.tensor(np.asarray(d, np.float32), requires_grad=True)
    fc = torch.cat((cl["f_dc_color"], cl["f_rest_color"]), dim=1)
    fp = torch.cat((torch.cat((cl["phase_f_dc"], cl["phase_f_rest"]), dim=1), torch.cat((cl["amp_f_dc"], cl["amp_f_rest"]), dim=1)), dim=2)
    a = assemble_ref.assemble_eager(cl["xyz"], cl["ssp"], torch.sigmoid(cl["opacity"]), torch.exp(cl["scaling"]),
                                    torch.nn.functional.normalize(cl["rotation"]), cl["rotation"], fc, fp,
                                    torch.as_tensor(mask, dtype=torch.bool), cl.get("d_xyz", 0.0), 0.0, cl.get("d_sh", 0.0), 0.0,
                                    render_regions=render_regions)
    return a, cl


def composed_reference_dynamic(oracle, scene, raw, mask, d_xyz, d_sh, up_color, up_phasor, render_regions=("static", "dynamic")):
    """:func:`composed_reference` for a model with a motion mask `mask` [P] and the network's offsets on its dynamic rows
    (:func:`dynamic_inputs`).  Returns (oracle forward, gradients by group name + "ssp" + "d_xyz" (+ "d_sh")); a leaf that
    nothing reached (the offsets of no dynamic row) has a zero gradient."""
    a, cl = dynamic_inputs(raw, mask, d_xyz, d_sh, render_regions)
    f = _through_the_rasterizer(oracle, scene, a, up_color, up_phasor)
    return f, {k: (v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape), np.float32)) for k, v in cl.items()}
