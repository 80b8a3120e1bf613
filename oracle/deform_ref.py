"""ORACLE (test infrastructure only) of the deformation network -- SURVEY section 8(f) row 2.

CPU restatement (numpy) of ``utils/time_utils.py`` of the reference:

* :func:`embed`        -- ``get_embedder`` / ``Embedder.embed`` (time_utils.py:8-53): include_input,
  log-sampled frequencies 2^0 .. 2^(multires-1), per frequency sin then cos of all input dims.
* :func:`forward`      -- ``DeformNetwork.forward`` (time_utils.py:103-127): 8 x (Linear + ReLU) of width
  256, the embedded input concatenated IN FRONT of the activations after layer 4 (``skips = [D // 2]``),
  heads ``xyz_warp`` and ``r``/``g``/``b`` (stacked on the last axis); ``d_rot`` and ``d_sh_p`` are
  returned as ZEROS by the reference (time_utils.py:127), the ``rot`` and ``a`` heads never reach an output.
* :func:`backward`     -- the adjoint of the above, written out by hand (chain rule of Linear / ReLU);
  inputs are not differentiated (the reference detaches them, scene/gaussian_model.py:172).  :func:`relu_margin` and
  :func:`relu_edges` say where a pre-activation is within rounding of zero and the gradient is not one value.

Parameters are a dict with the reference's ``state_dict`` names (``linear.0.weight`` ... ``b.bias``), numpy
arrays in torch's ``[out, in]`` layout.  ``dtype=np.float64`` gives the accuracy reference of the float32
comparisons.  Pinned against the reference's own module by ``tests/golden/deform.npz``
(``tests/golden/make_golden.py``).

* :func:`deform_eager` -- the same statements on torch tensors (eager ``F.linear`` / ``relu`` / ``cat``, autograd
  for the backward): what the reference's module runs on a GPU; bench.py times it beside the HIP path.

Only tests/, __graft_entry__.smoke() and bench.py's baseline leg may import this module.
"""
import numpy as np

D, W, XYZ_MULTIRES, NUM_SHS = 8, 256, 10, 16
# The reference constructs the network with t_multires = 10 (scene/deform_model.py:9-16 from
# arguments/__init__.py:66-69, configs/torf.json:9-12, configs/ftorf.json): 84 encoded inputs.  The class
# signature's default is 6 (time_utils.py:57): 76.  Every function takes ``t_multires``.
T_MULTIRES = 10
T_MULTIRES_CLASS_DEFAULT = 6
SKIP = D // 2                                    # time_utils.py:62
XYZ_CH = 3 + 3 * 2 * XYZ_MULTIRES                # 63


def in_ch(t_multires=T_MULTIRES, xyz_multires=XYZ_MULTIRES):
    """Columns of cat([x_emb, t_emb]) (time_utils.py:64-65): 84 for (10, 10), 76 for (10, 6)."""
    return 3 + 6 * xyz_multires + 1 + 2 * t_multires


IN_CH = in_ch()                                  # 84
HEADS = ("xyz_warp", "r", "g", "b")              # heads that reach an output
UNUSED = ("rot", "a")                            # computed by the reference, discarded (time_utils.py:118-127)


def param_shapes(t_multires=T_MULTIRES, xyz_multires=XYZ_MULTIRES):
    """state_dict names -> shapes (time_utils.py:68-81)."""
    s = {}
    n_in = in_ch(t_multires, xyz_multires)
    for i in range(D):
        fan_in = n_in if i == 0 else (W + n_in if i == SKIP + 1 else W)
        s["linear.%d.weight" % i] = (W, fan_in)
        s["linear.%d.bias" % i] = (W,)
    for name, out in (("xyz_warp", 3), ("rot", 4), ("r", NUM_SHS), ("g", NUM_SHS), ("b", NUM_SHS), ("a", NUM_SHS)):
        s[name + ".weight"] = (out, W)
        s[name + ".bias"] = (out,)
    return s


def arch_of(params):
    """(xyz_multires, t_multires) of a parameter dict, from the width of ``linear.0.weight`` (xyz_multires is 10
    in every configuration of the reference)."""
    n_in = params["linear.0.weight"].shape[1]
    t2 = n_in - XYZ_CH - 1
    assert t2 >= 0 and t2 % 2 == 0, n_in
    return XYZ_MULTIRES, t2 // 2


def random_params(seed, head_std=0.05, t_multires=T_MULTIRES):
    """Seeded parameters (synthetic data: the generator lives with the other synthetic inputs in ``gftorf_amd.synth``, so that
    the benches' HIP legs need nothing from this package; re-exported here for the tests)."""
    from gftorf_amd import synth
    p = synth.random_deform_params(seed, head_std=head_std, t_multires=t_multires)
    assert {k: v.shape for k, v in p.items()} == param_shapes(t_multires)
    return p


def reference_init_params(seed, t_multires=T_MULTIRES, head_std=1e-5):
    """Seeded parameters drawn as the reference's ``initialize_weights`` draws them (time_utils.py:85-101): Xavier-normal
    trunk, every bias zero, heads N(0, 1e-5).  ``head_std`` moves the heads alone."""
    from gftorf_amd import synth
    p = synth.random_deform_params(seed, head_std=head_std, t_multires=t_multires, bias_std=0.0)
    assert {k: v.shape for k, v in p.items()} == param_shapes(t_multires)
    return p


# Named input sets of the domain the reference queries the network on: world coordinates, signed and as large as the scene
# (scene/gaussian_model.py:170-174), times fid / (N - 1) including 0 and 1 exactly and a little beyond the last view
# (train.py:169-176).  x 2^f is exact in float32 and float64 alike, so forward(..., dtype=np.float64) on these float32
# values is the reference of every row.
DOMAIN_SETS = ("signed_unit", "room", "far", "reduction_switch", "time_switch", "plane_edge_below", "plane_edge_above",
               "guard_edge_below", "guard_edge_above")
# The fp16 walk takes an encoded input v while |16 v| <= 65504, i.e. |x| <= 4094.  plane_edge_* sit where 16 |x| passes
# 4094 (|x| = 255.875: both sides are still inside the planes), guard_edge_* at the guard itself: 4094 is the last value
# the walk keeps, 16 * 4096 = 65536 is beyond the largest fp16 and the call has to leave for the fp32-range walk.
EDITED = {"plane_edge_above": 300.0, "guard_edge_above": 4096.0}


def domain_inputs(name, n, seed):
    """(x[n,3], t[n,1], shared_t) of the input set ``name``, float32; the rows with exact values come first."""
    rng = np.random.default_rng(seed)
    sign = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    t = rng.uniform(0.0, 1.0, (n, 1))
    shared_t = False
    if name in ("signed_unit", "time_switch"):
        x = rng.uniform(-1.0, 1.0, (n, 3))
    elif name in ("room", "plane_edge_above", "guard_edge_above"):
        x = rng.uniform(-8.0, 8.0, (n, 3))
    elif name == "far":
        x = rng.uniform(-60.0, 60.0, (n, 3))
        t[:] = rng.uniform(0.0, 1.0)
        shared_t = True
    elif name == "reduction_switch":
        # 2^9 * 64 = 2^8 * 128 = 32768: where the encoding goes from its own reduction to the library's
        centre = np.where(rng.random((n, 3)) < 0.5, 64.0, 128.0)
        x = sign((n, 3)) * (centre + rng.uniform(-0.1, 0.1, (n, 3)))
    elif name == "plane_edge_below":
        x = sign((n, 3)) * rng.uniform(255.0, 255.87, (n, 3))
    elif name == "guard_edge_below":
        x = sign((n, 3)) * rng.uniform(4090.0, 4094.0, (n, 3))
    else:
        raise KeyError(name)
    x, t = x.astype(np.float32), t.astype(np.float32)
    if name in ("signed_unit", "time_switch") and n >= 4:
        x[0], x[1], x[2, 1], x[3, 2] = 0.0, -0.0, 0.0, -0.0
    if name == "reduction_switch" and n >= 4:
        x[0], x[1], x[2], x[3] = 64.0, -64.0, 128.0, (64.0, -128.0, 128.0)
    if name == "time_switch":
        # 2^15 t: 0, the last value below the encoding's switch, the switch itself (t_multires = 16), past the last view
        t[:, 0] = np.resize(np.array([0.0, 1.0 - 2.0 ** -16, 1.0, 1.04], np.float32), n)
    elif not shared_t and n >= 4:
        t[0], t[1] = 0.0, 1.0
        if name != "signed_unit":
            t[2], t[3] = -0.04, 1.04
    if name == "guard_edge_below" and n >= 4:
        x[0], x[1] = 4094.0, -4094.0
    if name in EDITED:
        x[n // 2, 1] = EDITED[name]                      # one coordinate of one row; every other value is `room`'s
    return x, t, shared_t


def embed_one(v, multires, dtype):
    """Embedder.embed (time_utils.py:24-53) of v[n, d]."""
    v = np.asarray(v, dtype)
    parts = [v]
    for f in range(multires):
        freq = dtype(2.0 ** f)                   # 2 ** linspace(0, multires-1, multires), exact
        parts.append(np.sin(v * freq))
        parts.append(np.cos(v * freq))
    return np.concatenate(parts, axis=-1)


def embed(x, t, dtype=np.float32, t_multires=T_MULTIRES):
    """cat([x_emb, t_emb]) (time_utils.py:104-107): [n, 63 + 1 + 2 t_multires]."""
    return np.concatenate([embed_one(x, XYZ_MULTIRES, dtype), embed_one(t, t_multires, dtype)], axis=-1)


def _trunk(params, x, t, dtype):
    emb = embed(x, t, dtype, arch_of(params)[1])
    h = emb
    inputs, outs = [], []
    for i in range(D):                           # time_utils.py:109-113
        w = params["linear.%d.weight" % i].astype(dtype)
        b = params["linear.%d.bias" % i].astype(dtype)
        inputs.append(h)
        z = h @ w.T + b
        a = np.maximum(z, 0)
        outs.append(a)
        h = np.concatenate([emb, a], axis=-1) if i == SKIP else a
    return emb, inputs, outs, h


def relu_margin(params, x, t):
    """Per point, the smallest |pre-activation| over all 8 x 256 units (float64).  The gradient is
    discontinuous where a pre-activation crosses zero, so comparisons of gradients between two
    arithmetics leave out the points whose margin is within rounding distance of that edge."""
    emb = embed(x, t, np.float64, arch_of(params)[1])
    h = emb
    margin = np.full(emb.shape[0], np.inf)
    for i in range(D):
        z = h @ params["linear.%d.weight" % i].astype(np.float64).T + params["linear.%d.bias" % i].astype(np.float64)
        margin = np.minimum(margin, np.abs(z).min(axis=1))
        a = np.maximum(z, 0)
        h = np.concatenate([emb, a], axis=-1) if i == SKIP else a
    return margin


def relu_edges(params, x, t, eps):
    """The units whose pre-activation is within ``eps`` of zero (float64), as (layer, point, unit) triples: where another
    arithmetic may take the ReLU on its other side (:func:`relu_margin`); :func:`backward` takes them as ``flip``."""
    emb = embed(x, t, np.float64, arch_of(params)[1])
    h = emb
    edges = []
    for i in range(D):
        z = h @ params["linear.%d.weight" % i].astype(np.float64).T + params["linear.%d.bias" % i].astype(np.float64)
        edges += [(i, int(r), int(u)) for r, u in zip(*np.nonzero(np.abs(z) < eps))]
        a = np.maximum(z, 0)
        h = np.concatenate([emb, a], axis=-1) if i == SKIP else a
    return edges


def forward(params, x, t, dtype=np.float32):
    """Returns (d_xyz[n,3], d_rot[n,4] = 0, d_sh[n,16,3], d_sh_p[n,16,2] = 0) (time_utils.py:115-127)."""
    _, _, _, h = _trunk(params, x, t, dtype)
    head = lambda n: h @ params[n + ".weight"].astype(dtype).T + params[n + ".bias"].astype(dtype)
    d_xyz = head("xyz_warp")
    d_sh = np.stack([head("r"), head("g"), head("b")], axis=-1)
    n = d_xyz.shape[0]
    return d_xyz, np.zeros((n, 4), dtype), d_sh, np.zeros((n, NUM_SHS, 2), dtype)


def backward(params, x, t, g_dxyz, g_dsh, dtype=np.float32, flip=()):
    """Gradients of sum(d_xyz * g_dxyz) + sum(d_sh * g_dsh) w.r.t. every parameter that reaches an output;
    the ``rot`` / ``a`` heads get None as under the reference's autograd.  ``flip``: (layer, point, unit) triples whose
    ReLU derivative is taken on the other side of zero (:func:`relu_edges`; the activation itself, about 0 there, stays)."""
    emb, inputs, outs, h = _trunk(params, x, t, dtype)
    on = [o > 0 for o in outs]
    for i, r, u in flip:
        on[i][r, u] = not on[i][r, u]
    g = {n + s: None for n in UNUSED for s in (".weight", ".bias")}
    g_dxyz = np.asarray(g_dxyz, dtype)
    g_dsh = np.asarray(g_dsh, dtype)
    dh = np.zeros_like(h)
    for name, go in (("xyz_warp", g_dxyz), ("r", g_dsh[:, :, 0]), ("g", g_dsh[:, :, 1]), ("b", g_dsh[:, :, 2])):
        g[name + ".weight"] = go.T @ h
        g[name + ".bias"] = go.sum(axis=0)
        dh = dh + go @ params[name + ".weight"].astype(dtype)
    for i in reversed(range(D)):
        dz = dh * on[i]
        g["linear.%d.weight" % i] = dz.T @ inputs[i]
        g["linear.%d.bias" % i] = dz.sum(axis=0)
        dh = dz @ params["linear.%d.weight" % i].astype(dtype)
        if i == SKIP + 1:
            dh = dh[:, emb.shape[1]:]            # the embedded part of the skip input has no parameters
    return g


def deform_eager(params, x, t):
    """time_utils.py:103-127 on torch tensors (``params``: name -> tensor, torch layout), including the two
    heads the reference computes and throws away."""
    import torch
    import torch.nn.functional as F

    def emb_one(v, multires):
        parts = [v]
        for f in range(multires):
            parts += [torch.sin(v * float(2 ** f)), torch.cos(v * float(2 ** f))]
        return torch.cat(parts, -1)

    t_multires = (params["linear.0.weight"].shape[1] - XYZ_CH - 1) // 2
    emb = torch.cat([emb_one(x, XYZ_MULTIRES), emb_one(t, t_multires)], dim=-1)
    h = emb
    for i in range(D):
        h = F.relu(F.linear(h, params["linear.%d.weight" % i], params["linear.%d.bias" % i]))
        if i == SKIP:
            h = torch.cat([emb, h], -1)
    head = lambda n: F.linear(h, params[n + ".weight"], params[n + ".bias"])
    d_xyz = head("xyz_warp")
    d_sh_a = head("a")                                   # time_utils.py:119, unused
    d_rot = head("rot")                                  # time_utils.py:125, replaced by zeros
    d_sh = torch.stack([head("r"), head("g"), head("b")], dim=-1)
    return d_xyz, torch.zeros_like(d_rot), d_sh, torch.zeros(d_sh_a.shape + (2,), device=x.device)
