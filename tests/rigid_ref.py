"""Float64 restatement of the reference's find_knn / rigidity_loss / isometry_loss (utils/loss_utils.py:35-72), for
tests/test_rigid.py and tests/golden/make_golden_rigid.py.  numpy only; the gradients are written out by hand (autograd's are
in tests/golden/rigid.npz, from the reference's own functions, and test_rigid.py holds these against them).

With j = idx[i, k], w = w_i_j[i, k], d0 = initial_xyz_to_knn_dist[i, k]:
  rigidity = mean w * sqrt(|(prev_i - prev_j) - (curr_i - curr_j)|^2 + 1e-16)
  isometry = mean |w * (sqrt(d0 + 1e-16) - sqrt(|curr_i - curr_j|^2 + 1e-16))|
"""
import numpy as np

EPS = 1e-16


def clouds(P, kind, seed=5):
    """tests/test_knn.py's clouds, and `centred`: its clustered cloud without the offset of 20, its mean at the origin."""
    import test_knn
    if kind != "centred":
        return test_knn.cloud(P, seed, kind)
    rng = np.random.default_rng(seed)
    c = rng.normal(0, 3, (8, 3))
    pts = c[rng.integers(0, 8, P)] + rng.normal(0, 0.05, (P, 3))
    pts[: P // 10] = rng.uniform(-10, 10, (P // 10, 3))
    return (pts - pts.mean(axis=0)).astype(np.float32)


def dist2_f32(a, b):
    """dx * dx + dy * dy + dz * dz in float32, every operation rounded on its own (oracle/knn_ref.py's expression)"""
    d = (b.astype(np.float32) - a.astype(np.float32)).astype(np.float32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float32) + d[..., 2] * d[..., 2]).astype(np.float32)


def knn_bruteforce(points, K, rows=None, chunk=512):
    """(idx, dist2) of the K nearest other points of `rows` (all by default), a row ordered by (float32 distance, index)"""
    p = np.asarray(points, np.float32)
    rows = np.arange(p.shape[0]) if rows is None else np.asarray(rows)
    idx = np.empty((rows.size, K), np.int64)
    for s in range(0, rows.size, chunk):
        r = rows[s:s + chunk]
        d = dist2_f32(p[r][:, None, :], p[None, :, :]).astype(np.float64)
        d[np.arange(r.size), r] = np.inf                       # self excluded by index
        # stable argsort: equal distances stay in index order
        idx[s:s + chunk] = np.argsort(d, axis=1, kind="stable")[:, :K]
    return idx, dist2_f32(p[rows][:, None, :], p[idx])


def exact_knn(points, K, spare=8):
    """As knn_bruteforce for every row, through scipy's cKDTree: K + `spare` candidates, the point itself removed by index,
    ordered by (float32 distance, index).  A row whose last candidate is no farther than its K-th neighbour (a run of equal
    distances may go on beyond the candidates) is redone by brute force."""
    from scipy.spatial import cKDTree
    p = np.asarray(points, np.float32)
    P = p.shape[0]
    assert P > K
    n = K + spare + 1
    if P <= n:
        return knn_bruteforce(p, K)
    p64 = p.astype(np.float64)
    _, cand = cKDTree(p64).query(p64, k=n)
    rows = np.arange(P)[:, None]
    d = dist2_f32(p[:, None, :], p[cand]).astype(np.float64)
    d[cand == rows] = np.inf
    missing = ~(cand == rows).any(axis=1)                      # many duplicates: the point itself fell out of its candidates
    order = np.lexsort((cand, d), axis=1)                      # by distance, then by index
    cand, d = np.take_along_axis(cand, order, 1), np.take_along_axis(d, order, 1)
    idx = cand[:, :K].copy()
    last = np.where(missing, d[:, n - 1], d[:, n - 2])         # the farthest real candidate
    redo = np.nonzero(missing | (last <= d[:, K - 1]))[0]
    if redo.size:
        idx[redo] = knn_bruteforce(p, K, redo)[0]
    return idx, dist2_f32(p[:, None, :], p[idx])


def table_weights(prev, idx):
    """(w_i_j, initial_xyz_to_knn_dist) of a case, float32 [P, K]: d0 the float32 squared distances of `prev` along the
    table, w = 1 / (1 + d0 / median(d0)).  Correctly rounded float32 operations only, so every platform gets the bits the
    golden values were computed with (an exp would not promise that)."""
    p = np.asarray(prev, np.float32)
    d0 = dist2_f32(p[:, None, :], p[idx])
    lam = np.float32(1.0) / np.float32(np.median(d0) + np.float32(1e-12))
    w = (np.float32(1.0) / (np.float32(1.0) + (lam * d0).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return w, d0


def losses(prev, curr, idx, w, d0):
    """dict of float64: rig, iso (the two means), rig_g_curr, rig_g_prev, iso_g_curr [P, 3] (the gradients of each mean)"""
    prev, curr, w, d0 = (np.asarray(a, np.float64) for a in (prev, curr, w, d0))
    idx = np.asarray(idx, np.int64)
    P, K = idx.shape
    n = float(P * K)
    u = curr[:, None, :] - curr[idx]                           # [P, K, 3]
    v = (prev[:, None, :] - prev[idx]) - u
    rv = np.sqrt((v ** 2).sum(-1) + EPS)
    ru = np.sqrt((u ** 2).sum(-1) + EPS)
    t = w * (np.sqrt(d0 + EPS) - ru)
    out = dict(rig=(w * rv).mean(), iso=np.abs(t).mean())

    def scatter(own):                                          # + to the row's point, - to the neighbour
        g = own.sum(axis=1)
        np.subtract.at(g, idx.reshape(-1), own.reshape(-1, 3))
        return g

    d_rig = (w / rv)[..., None] * v / n                        # d rigidity / d v
    out["rig_g_prev"] = scatter(d_rig)
    out["rig_g_curr"] = -out["rig_g_prev"]
    out["iso_g_curr"] = scatter((-np.sign(t) * w / ru)[..., None] * u / n)
    return out


def max_in_degree(idx):
    idx = np.asarray(idx)
    return int(np.bincount(idx.reshape(-1), minlength=idx.shape[0]).max())
