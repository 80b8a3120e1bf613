"""The layout of one densify_and_prune event, one row at a time (test infrastructure of tests/test_densify_fused.py).

The event (scene/gaussian_model.py:571-640) is a function of per-row quantities: which rows are cloned, which are split,
which of the originals, clones and children survive the final prune, and where every survivor lands.  `classify` and `layout`
restate that in plain Python over numpy float32 values; `apply` builds the event's result from the input by plain indexing.
"""
import numpy as np
import torch

f32 = np.float32


def classify(grad_norm, grad, max_scaling, max_grad, dense_threshold):
    """Per row 0 (neither), 1 (cloned) or 2 (split).  The thresholds meet the float32 values as float32."""
    mg, thr = f32(max_grad), f32(dense_threshold)
    cls = np.zeros(len(grad), np.uint8)
    for i in range(len(grad)):
        if grad_norm[i] >= mg and max_scaling[i] <= thr:
            cls[i] = 1
        elif grad[i] >= mg and max_scaling[i] > thr:
            cls[i] = 2
    return cls


def layout(cls, opacity, max_scaling, child_max_scaling, N, min_opacity, extent, max_screen_size):
    """(source_row, kind, child) of the survivors, in the order of the virtual rows: the P originals, the clones in the order
    of their sources, the children (child k * S + j belongs to the j-th split row)."""
    P = len(cls)
    clones = [i for i in range(P) if cls[i] == 1]
    splits = [i for i in range(P) if cls[i] == 2]
    S = len(splits)
    virtual = [(i, 0, -1) for i in range(P)] + [(i, 1, -1) for i in clones] + [(splits[c % S], 2, c) for c in range(N * S)]
    mo = f32(min_opacity)
    source_row, kind, child = [], [], []
    for src, kd, ch in virtual:
        if kd == 0 and cls[src] == 2:
            continue                                             # densify_and_split removes the parents
        dead = opacity[src] < mo
        if max_screen_size:
            m = child_max_scaling[ch] if kd == 2 else max_scaling[src]
            # max_radii2D is all zeros at that point: densification_postfix cleared it
            dead = dead or f32(0.0) > f32(max_screen_size) or m > f32(0.05 * extent) or m < f32(0.001 * extent)
        if not dead:
            source_row.append(src)
            kind.append(kd)
            child.append(ch)
    return np.asarray(source_row, np.int64), np.asarray(kind, np.uint8), np.asarray(child, np.int64)


def row_quantities(pc):
    """(grad_norm, grad, max_scaling, opacity) of the model, float32 numpy [P]: the reference's statements."""
    with torch.no_grad():
        grads = pc.xyz_gradient_accum / pc.denom
        grads[grads.isnan()] = 0.0
        return (torch.norm(grads, dim=-1).cpu().numpy(), grads.reshape(-1).cpu().numpy(),
                torch.max(pc.get_scaling, dim=1).values.cpu().numpy(), pc.get_opacity.reshape(-1).cpu().numpy())


def children_scaling(pc, cls, N):
    """The children's raw scaling [N * S, cols] (densify_and_split's statement on the split rows)."""
    with torch.no_grad():
        sel = torch.as_tensor(cls == 2, device=pc._scaling.device)
        return pc.scaling_inverse_activation(pc.get_scaling[sel].repeat(N, 1) / (0.8 * N))


def plan(pc, max_grad, min_opacity, extent, max_screen_size, N=2):
    """dict(cls, source_row, kind, child, new_scaling) of the event on `pc` (not modified)."""
    grad_norm, grad, max_scaling, opacity = row_quantities(pc)
    cls = classify(grad_norm, grad, max_scaling, max_grad, pc.percent_dense * extent)
    new_scaling = children_scaling(pc, cls, N)
    with torch.no_grad():
        child_ms = pc.scaling_activation(new_scaling).max(dim=1).values.cpu().numpy()
    source_row, kind, child = layout(cls, opacity, max_scaling, child_ms, N, min_opacity, extent, max_screen_size)
    return dict(cls=cls, source_row=source_row, kind=kind, child=child, new_scaling=new_scaling.cpu())


def apply(snapshot, pl):
    """The event's result from `snapshot` (EagerGaussians.snapshot() before the event) by plain indexing: parameters by
    their source row (a child's scaling is its new one; a child's xyz is left as its parent's: the caller exempts those
    rows), moments by their source row with zeros for new rows, zero statistics."""
    src, kind, child = torch.as_tensor(pl["source_row"]), torch.as_tensor(pl["kind"]), torch.as_tensor(pl["child"])
    out = {}
    for k, v in snapshot.items():
        if k in ("xyz_gradient_accum", "denom", "max_radii2D"):
            out[k] = torch.zeros((len(src),) + tuple(v.shape[1:]))
        elif k.startswith("step:") or k.split(":")[-1] in ("phase_offset", "dc_offset"):
            out[k] = v                                           # (the event leaves the two offsets' groups alone)
        elif k.startswith(("m:", "v:")):
            moved = v[src].clone()
            moved[kind != 0] = 0.0
            out[k] = moved
        else:
            moved = v[src].clone()
            if k == "_scaling":
                moved[kind == 2] = pl["new_scaling"][child[kind == 2]]
            out[k] = moved
    return out
