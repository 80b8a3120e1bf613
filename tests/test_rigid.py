"""gftorf_amd.rigid: exact K nearest neighbours, and the reference's rigidity_loss / isometry_loss (utils/loss_utils.py:35-72)
as one autograd node.  Yardsticks: tests/rigid_ref.py (float64, numpy; exact neighbours through scipy's cKDTree) and
tests/golden/rigid.npz (the reference's own functions in float32 and float64, tests/golden/make_golden_rigid.py).

Tolerances:
  neighbours   a row's squared distances equal the oracle's K smallest, and each the float32 distance of its index, to
               rtol 2e-6 (the kernel's FMA against numpy's separately rounded products, as test_knn.py allows); order, self
               exclusion, distinctness and determinism are exact
  values       4 * e_ref of the float64 value, e_ref the reference's own float32 error on the case (rigid.npz); on the
               two-point case, which has no golden data, e_ref is that of `statements` below run by torch on the CPU, and
               the bound is not taken below 8 * 2^-24: a term is ~8 rounded float32 operations
  gradients    max(4 * e_ref, n * 2^-23) of the float64 gradient's max-norm, n = K + the table's largest in-degree, the
               number of terms a component sums: each term carries a few roundings of 2^-24, adding linearly at worst
Measured on the MI355X (error / bound, the worst over the cases): see the table in DESIGN.md section 6.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import rigid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_rigid.h")
GOLDEN_CASES = {"u21": (21, 20), "u1025": (1025, 20), "c3000": (3000, 20)}
E_REF = ("rig", "iso", "rig_g_curr", "rig_g_prev", "iso_g_curr")
EPS23 = 2.0 ** -23


# ---- the statements, for torch in any dtype on any device -----------------------------------------------------------------

def statements(prev, curr, idx, w, d0):
    """loss_utils.py:55-60 and :70-72, to be read against those lines: (rigidity, isometry)"""
    K = idx.shape[1]
    curr_knn_pos, prev_knn_pos = curr[idx], prev[idx]
    curr_rep, prev_rep = curr.unsqueeze(1).expand(-1, K, -1), prev.unsqueeze(1).expand(-1, K, -1)
    rig = (w * torch.sqrt((((prev_rep - prev_knn_pos) - (curr_rep - curr_knn_pos)) ** 2).sum(dim=-1) + 1e-16)).mean()
    iso = (w * (torch.sqrt(d0 + 1e-16) - torch.sqrt(((curr_rep - curr_knn_pos) ** 2).sum(dim=-1) + 1e-16))).abs().mean()
    return rig, iso


def run_statements(c, dtype, dev):
    """dict as rigid_ref.losses, by torch autograd"""
    t = {k: torch.tensor(c[k], dtype=dtype, device=dev) for k in ("prev", "curr", "w", "d0")}
    idx = torch.tensor(c["idx"], device=dev)
    out = {}
    p, q = t["prev"].clone().requires_grad_(), t["curr"].clone().requires_grad_()
    rig, _ = statements(p, q, idx, t["w"], t["d0"])
    rig.backward()
    out.update(rig=rig.item(), rig_g_curr=q.grad.cpu().numpy(), rig_g_prev=p.grad.cpu().numpy())
    q = t["curr"].clone().requires_grad_()
    _, iso = statements(t["prev"], q, idx, t["w"], t["d0"])
    iso.backward()
    out.update(iso=iso.item(), iso_g_curr=q.grad.cpu().numpy())
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "rigid.npz")))


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs, the float64 results (`ref`), e_ref per tensor and n = K + the largest in-degree; computed once and shared"""
    if name == "two":                        # (P, K) = (2, 1): each point the other's neighbour
        rng = np.random.default_rng(3)
        prev = rng.uniform(-1, 1, (2, 3)).astype(np.float32)
        curr = (prev + rng.normal(0, 0.01, (2, 3))).astype(np.float32)
        idx = np.array([[1], [0]], np.int64)
        w, d0 = R.table_weights(prev, idx)
        c = dict(prev=prev, curr=curr, idx=idx, w=w, d0=d0)
        c["ref"] = R.losses(prev, curr, idx, w, d0)
        r32 = run_statements(c, torch.float32, "cpu")
        rel = lambda k: float(np.abs(np.asarray(r32[k], np.float64) - c["ref"][k]).max() / np.abs(c["ref"][k]).max())
        c["e_ref"] = {k: max(rel(k), 2.0 * 2.0 ** -24) if k in ("rig", "iso") else rel(k) for k in E_REF}
    else:
        g = golden()
        prev, curr, idx = g[name + "_prev"], g[name + "_curr"], g[name + "_idx"].astype(np.int64)
        w, d0 = R.table_weights(prev, idx)
        c = dict(prev=prev, curr=curr, idx=idx, w=w, d0=d0)
        c["ref"] = dict(rig=g[name + "_rig"][1], iso=g[name + "_iso"][1], rig_g_curr=g[name + "_rig_g_curr"],
                        rig_g_prev=-g[name + "_rig_g_curr"], iso_g_curr=g[name + "_iso_g_curr"])
        c["e_ref"] = dict(zip(E_REF, g[name + "_e_ref"]))
    c["n"] = idx.shape[1] + R.max_in_degree(idx)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def grad_bound(c, k):
    return max(4.0 * c["e_ref"][k], c["n"] * EPS23) * np.abs(c["ref"][k]).max()


def on_device(c, dev, grad=True):
    t = types.SimpleNamespace(**{k: torch.tensor(c[k], device=dev) for k in ("prev", "curr", "w", "d0")})
    t.idx = torch.tensor(c["idx"], device=dev)
    if grad:
        t.prev.requires_grad_(), t.curr.requires_grad_()
    return t


# ---- CPU: the yardsticks themselves, the header, the argument checks ------------------------------------------------------

@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_restatement_equals_the_reference(name):
    """rigid_ref.losses against the reference's functions in float64 (values and autograd's gradients), and torch's
    restatement in this file against both"""
    c = case(name)
    assert c["idx"].shape == GOLDEN_CASES[name]
    own = R.losses(c["prev"], c["curr"], c["idx"], c["w"], c["d0"])
    tor = run_statements(c, torch.float64, "cpu")
    for k in E_REF:
        scale = np.abs(c["ref"][k]).max()
        assert np.abs(own[k] - c["ref"][k]).max() <= 1e-12 * scale, k
        assert np.abs(tor[k] - c["ref"][k]).max() <= 1e-12 * scale, k
    g = golden()
    assert abs(g[name + "_rig"][0] - g[name + "_rig"][1]) == pytest.approx(c["e_ref"]["rig"] * g[name + "_rig"][1], rel=1e-6)
    assert max(c["e_ref"]["rig"], c["e_ref"]["iso"], c["e_ref"]["rig_g_curr"], c["e_ref"]["rig_g_prev"]) <= 1.6e-6


def test_the_isometry_gradient_has_a_kink_the_float32_reference_can_sit_on():
    """What the reference's float32 isometry gradient being percents off float64 on some clouds comes from: the term is
    |w (sqrt(d0) - r)|, and on an edge where sqrt(d0) - r is below float32's rounding its sign -- the whole term of the
    gradient -- is decided by rounding.  u1025 has one such edge: float64 gives +1.8e-9, float32 exactly 0, so torch's
    abs passes no gradient; e_ref of that tensor is 1.9e-2, on every other tensor of every case it is below 1e-6."""
    c = case("u1025")
    u = c["curr"].astype(np.float64)[:, None, :] - c["curr"].astype(np.float64)[c["idx"]]
    t64 = np.sqrt(c["d0"].astype(np.float64) + 1e-16) - np.sqrt((u ** 2).sum(-1) + 1e-16)
    u32 = c["curr"][:, None, :] - c["curr"][c["idx"]]
    t32 = np.sqrt(c["d0"] + np.float32(1e-16)) - np.sqrt((u32 ** 2).sum(-1, dtype=np.float32) + np.float32(1e-16))
    flips = np.argwhere(np.sign(t32) != np.sign(t64))
    assert len(flips) == 1 and abs(t64[tuple(flips[0])]) < 1e-8
    assert 1e-2 < c["e_ref"]["iso_g_curr"] < 3e-2
    for name in GOLDEN_CASES:
        assert all(v <= 1.6e-6 for k, v in case(name)["e_ref"].items() if (name, k) != ("u1025", "iso_g_curr"))


@pytest.mark.parametrize("P,K,kind", [(9, 8, "uniform"), (300, 20, "duplicates"), (700, 5, "clustered"), (257, 32, "plane")])
def test_oracle_knn_equals_bruteforce(P, K, kind):
    p = R.clouds(P, kind)
    a, b = R.exact_knn(p, K), R.knn_bruteforce(p, K)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not (a[0] == np.arange(P)[:, None]).any()
    assert (np.diff(a[1].astype(np.float64), axis=1) >= 0).all()


def test_golden_find_knn_is_the_exact_table():
    g = golden()
    for name in ("u21", "u1025"):
        assert np.array_equal(g[name + "_find_knn"], g[name + "_idx"])
        assert np.array_equal(g[name + "_idx"], R.knn_bruteforce(g[name + "_prev"], GOLDEN_CASES[name][1])[0])


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
    assert set(names) == set(_lib.RIGID_EXPORTS), names
    assert all(n.startswith("gft_rigid_") for n in names)
    others = [t for t in dir(_lib) if t.endswith("EXPORTS") and t != "RIGID_EXPORTS"]
    assert len(others) >= 16 and "EXPORTS" in others and "REG_EXPORTS" in others
    for t in others:
        assert not set(names) & set(getattr(_lib, t)), t
    for n in names:
        assert hasattr(lib, n), n
    assert "struct" not in re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    prog = tmp_path / "rigid_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_rigid.h"', '#include "gftorf_knn.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "rigid_abi.o")])
    out = subprocess.check_output(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-include", "gftorf_rigid.h",
                                   "-x", "c", "-"], input="WORDS_ARE GFT_RIGID_MAX_K GFT_RIGID_PARTIAL_WORDS GFT_RIGID_MEANS GFT_RIGID_TOTAL\n",
                                  text=True)
    consts = [int(v) for v in out.split("WORDS_ARE", 1)[1].split()]
    assert consts == [_lib.RIGID_MAX_K, _lib.RIGID_PARTIAL_WORDS, _lib.RIGID_MEANS, _lib.RIGID_TOTAL]
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16
    assert lib.gft_rigid_result_words() > _lib.RIGID_TOTAL


def test_size_queries_and_argument_errors(lib):
    from gftorf_amd import _lib
    assert lib.gft_rigid_blocks(0, 20) == 0 and lib.gft_rigid_blocks(5, 0) == 0 and lib.gft_rigid_blocks(-1, 3) == 0
    assert lib.gft_rigid_blocks(2, 1) == 1 and lib.gft_rigid_blocks(1024, 1) == 1 and lib.gft_rigid_blocks(1025, 1) == 2
    assert lib.gft_rigid_blocks(1025, 20) == 21 and lib.gft_rigid_blocks(100_000, 20) == 1024       # then grid-stride
    assert lib.gft_rigid_knn_scratch_bytes(1000) == lib.gft_knn_scratch_bytes(1000)
    x = C.c_void_p(16)                                         # never dereferenced: the calls fail before any launch
    for P, K, word in ((100, 0, "outside"), (100, 33, "outside"), (20, 20, "other points"), (1 << 30, 4, "too large")):
        assert lib.gft_rigid_knn(None, P, K, x, x, x, x) != 0 and word in _lib.last_error(), (P, K)
    assert lib.gft_rigid_knn(None, 100, 3, None, x, x, x) != 0 and "NULL" in _lib.last_error()
    fwd = lambda P, K, idx, w, prev, curr, d0, part=x, res=x: lib.gft_rigid_forward(None, P, K, idx, w, prev, curr, d0, None, 1.0, 1.0, part, res)
    assert fwd(0, 3, x, x, x, x, x) != 0 and "bad sizes" in _lib.last_error()
    assert fwd(10, 3, None, x, x, x, x) != 0 and "NULL" in _lib.last_error()
    assert fwd(10, 3, x, x, None, x, None) != 0 and "no term" in _lib.last_error()
    assert fwd(10, 3, x, x, x, x, x, None) != 0 and "NULL" in _lib.last_error()
    bwd = lambda P, K, off, prev, g, gc, gp: lib.gft_rigid_backward(None, P, K, x, off, x, x, prev, x, x, None, 1.0, 1.0, g, gc, gp)
    assert bwd(10, 3, None, x, x, x, x) != 0 and "NULL" in _lib.last_error()
    assert bwd(10, 3, x, x, None, x, x) != 0 and "NULL" in _lib.last_error()
    assert bwd(10, 3, x, None, x, x, x) != 0 and "g_prev without prev" in _lib.last_error()
    assert bwd(10, 3, x, x, x, None, None) == 0                # nothing asked for: nothing launched


def test_wrapper_rejects_what_the_kernels_cannot_take():
    import gftorf_amd
    from gftorf_amd import rigid
    assert gftorf_amd.find_knn is rigid.find_knn and gftorf_amd.Neighbours is rigid.Neighbours
    assert gftorf_amd.rigidity_loss is rigid.rigidity_loss and gftorf_amd.isometry_loss is rigid.isometry_loss
    xyz, idx = torch.zeros(40, 3), torch.zeros(40, 3, dtype=torch.int64)
    w = torch.ones(40, 3)
    with pytest.raises(RuntimeError, match="HIP device only"):
        rigid.find_knn(xyz, 3)
    with pytest.raises(RuntimeError, match="HIP device only"):
        rigid.Neighbours.build(xyz, 3)
    with pytest.raises(RuntimeError, match="HIP device only"):
        rigid.Neighbours.from_indices(idx)
    with pytest.raises(RuntimeError, match="HIP device only"):
        rigid.rigidity_loss(w, xyz, xyz, idx)
    with pytest.raises(RuntimeError, match="HIP device only"):
        rigid.isometry_loss(types.SimpleNamespace(w_i_j=w, initial_xyz_to_knn_dist=w), xyz, idx)
    for P, k in ((3, 3), (20, 20), (2, 5)):                    # the reference's topk(k + 1) raises there too
        with pytest.raises(ValueError, match="other points"):
            rigid.find_knn(torch.zeros(P, 3), k)
    for k in (0, 33, 34, 1000):
        with pytest.raises(ValueError, match="outside 1..32"):
            rigid.find_knn(torch.zeros(2000, 3), k)
    for bad in (dict(w=w.clone().requires_grad_()), dict(d0=w.clone().requires_grad_())):
        with pytest.raises(NotImplementedError, match="requires grad"):
            rigid.rigid_terms(xyz, xyz, idx, bad.get("w", w), bad.get("d0", w))
    with pytest.raises(NotImplementedError, match="requires grad"):
        rigid.rigidity_loss(types.SimpleNamespace(w_i_j=w.clone().requires_grad_()), xyz, xyz, idx)
    with pytest.raises(RuntimeError, match=r"\[P, 3\]"):
        rigid.find_knn(torch.zeros(40, 2), 3)
    with pytest.raises(TypeError, match="float32"):
        rigid.find_knn(torch.zeros(40, 3, dtype=torch.float64), 3)
    with pytest.raises(TypeError, match="int32 or torch.int64"):
        rigid.Neighbours.from_indices(idx.float())
    with pytest.raises(ValueError, match="no term"):
        rigid.rigid_terms(None, xyz, idx, w, None)


# ---- GPU: the neighbours ---------------------------------------------------------------------------------------------------

KNN_CASES = [(2, 1, "uniform"), (9, 8, "uniform"), (21, 20, "uniform"), (1024, 8, "uniform"), (1025, 20, "plane"),
             (2049, 32, "uniform"), (5000, 16, "duplicates"), (20000, 20, "clustered")]


@pytest.mark.gpu
@pytest.mark.parametrize("P,K,kind", KNN_CASES)
def test_hip_knn_vs_oracle(P, K, kind, gpu):
    from gftorf_amd import rigid
    p = R.clouds(P, kind)
    nb = rigid.Neighbours.build(torch.tensor(p, device=gpu), K)
    assert nb.idx.dtype == torch.int32 and nb.dist2.dtype == torch.float32
    assert tuple(nb.idx.shape) == tuple(nb.dist2.shape) == (P, K) and (nb.P, nb.K) == (P, K)
    idx, d = nb.idx.cpu().numpy().astype(np.int64), nb.dist2.cpu().numpy()
    assert idx.min() >= 0 and idx.max() < P
    assert not (idx == np.arange(P)[:, None]).any()                            # no self index
    assert (np.diff(np.sort(idx, axis=1), axis=1) > 0).all()                   # distinct along a row
    step = np.diff(d.astype(np.float64), axis=1)
    assert (step >= 0).all()                                                   # non-decreasing
    assert (np.diff(idx, axis=1)[step == 0] > 0).all()                         # equal distances: increasing index
    np.testing.assert_allclose(d, R.dist2_f32(p[:, None, :], p[idx]), rtol=2e-6, atol=1e-30)
    ref_idx, ref_d = R.exact_knn(p, K)
    np.testing.assert_allclose(d, ref_d, rtol=2e-6, atol=1e-30)
    # the transpose: every edge once, under the point it names, ascending
    off, edges = nb.offsets.cpu().numpy().astype(np.int64), nb.edges.cpu().numpy().astype(np.int64)
    assert off[0] == 0 and off[-1] == P * K and np.array_equal(np.diff(off), np.bincount(idx.reshape(-1), minlength=P))
    assert np.array_equal(idx.reshape(-1)[edges], np.repeat(np.arange(P), np.diff(off)))
    assert np.array_equal(np.sort(edges), np.arange(P * K))
    inner = np.ones(P * K, bool)
    inner[off[:-1][np.diff(off) > 0]] = False
    assert (np.diff(edges)[inner[1:]] > 0).all()
    if K >= 3:                                                                 # distCUDA2's value to the bit
        from gftorf_amd import distCUDA2
        mean = distCUDA2(torch.tensor(p, device=gpu)).cpu().numpy()
        assert np.array_equal(((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0), mean)


@pytest.mark.gpu
def test_hip_knn_is_deterministic_and_follows_a_permutation(gpu):
    from gftorf_amd import rigid
    p = torch.tensor(R.clouds(20000, "clustered"), device=gpu)
    a = rigid.Neighbours.build(p, 20)
    for _ in range(3):
        b = rigid.Neighbours.build(p, 20)
        assert torch.equal(a.idx, b.idx) and torch.equal(a.dist2, b.dist2)
    # a cloud without equal distances: the table of the permuted cloud is the permuted table, whatever the placement did
    q = R.clouds(3001, "uniform", seed=11)
    base = rigid.Neighbours.build(torch.tensor(q, device=gpu), 16)
    d = base.dist2.cpu().numpy()
    assert (np.diff(d.astype(np.float64), axis=1) > 0).all()
    perm = np.random.default_rng(2).permutation(3001)
    moved = rigid.Neighbours.build(torch.tensor(q[perm], device=gpu), 16)
    assert np.array_equal(perm[moved.idx.cpu().numpy()], base.idx.cpu().numpy()[perm])
    assert np.array_equal(moved.dist2.cpu().numpy(), d[perm])


@pytest.mark.gpu
def test_find_knn_equals_the_reference_on_its_good_clouds(gpu):
    from gftorf_amd import find_knn
    g = golden()
    for name in ("u21", "u1025"):
        got = find_knn(torch.tensor(g[name + "_prev"], device=gpu), GOLDEN_CASES[name][1])
        assert got.dtype == torch.int64 and got.device == gpu
        assert np.array_equal(got.cpu().numpy(), g[name + "_find_knn"].astype(np.int64))


# ---- GPU: the losses -------------------------------------------------------------------------------------------------------

LOSS_CASES = ["two", "u21", "u1025", "c3000"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", LOSS_CASES)
def test_losses_vs_float64(name, gpu):
    """each drop-in alone, its value and its gradients"""
    from gftorf_amd import rigid
    c = case(name)
    t = on_device(c, gpu)
    nb = rigid.Neighbours.from_indices(t.idx)
    model = types.SimpleNamespace(w_i_j=t.w, initial_xyz_to_knn_dist=t.d0)
    rig = rigid.rigidity_loss(model, t.prev, t.curr, nb)
    rig.backward()
    got = dict(rig=rig.item(), rig_g_curr=t.curr.grad.cpu().numpy(), rig_g_prev=t.prev.grad.cpu().numpy())
    t.curr.grad = None
    iso = rigid.isometry_loss(model, t.curr, nb)
    iso.backward()
    got.update(iso=iso.item(), iso_g_curr=t.curr.grad.cpu().numpy())
    report, fails = [], []
    for k in E_REF:
        err = float(np.abs(np.asarray(got[k], np.float64) - c["ref"][k]).max())
        bound = 4.0 * c["e_ref"][k] * abs(c["ref"][k]) if k in ("rig", "iso") else grad_bound(c, k)
        report.append("%s %.3g / %.3g" % (k, err, bound))
        if not err <= bound:
            fails.append(k)
    print("rigid %s (n = %d): error / bound: %s" % (name, c["n"], "; ".join(report)))
    assert not fails, report
    assert rig.dtype == torch.float32 and rig.dim() == 0 and got["rig_g_prev"].shape == c["prev"].shape


@pytest.mark.gpu
def test_fused_node_terms_weights_and_runs(gpu):
    """rigid_terms: each term alone is the fused node's mean for it bit for bit, device weights equal the same floats, a
    second run repeats every bit, and the index-tensor form equals the Neighbours form"""
    from gftorf_amd import rigid
    c = case("u1025")
    nb = rigid.Neighbours.from_indices(torch.tensor(c["idx"], device=gpu))

    def run(w_rigid, w_iso, weights=None, neighbours=nb, up=1.0):
        t = on_device(c, gpu)
        total, terms = rigid.rigid_terms(t.prev, t.curr, neighbours, t.w, t.d0, w_rigid, w_iso, weights=weights)
        assert not terms.means.requires_grad and not terms.total.requires_grad
        (up * total).backward()
        return total.detach(), terms.means.clone(), t.curr.grad, t.prev.grad

    a = run(4.0, 2.0)
    for other in (run(4.0, 2.0), run(0.0, 0.0, weights=torch.tensor([4.0, 2.0], device=gpu)),
                  run(4.0, 2.0, neighbours=torch.tensor(c["idx"].astype(np.int32), device=gpu))):
        assert all(torch.equal(x, y) for x, y in zip(a, other))
    t = on_device(c, gpu, grad=False)
    assert torch.equal(rigid.rigidity_loss(t.w, t.prev, t.curr, nb), a[1][0])
    assert torch.equal(rigid.isometry_loss(t.w, t.curr, nb, t.d0), a[1][1])
    assert float(a[0]) == pytest.approx(4.0 * float(a[1][0]) + 2.0 * float(a[1][1]), rel=1e-6)
    ref = c["ref"]
    for got, k in ((a[2], 4.0 * ref["rig_g_curr"] + 2.0 * ref["iso_g_curr"]), (a[3], 4.0 * ref["rig_g_prev"])):
        bound = 4.0 * grad_bound(c, "rig_g_curr") + 2.0 * grad_bound(c, "iso_g_curr")
        assert np.abs(got.cpu().numpy() - k).max() <= bound
    # the upstream gradient is read on the device and scales both
    half = run(4.0, 2.0, up=0.5)
    assert torch.equal(half[2], 0.5 * a[2]) and torch.equal(half[3], 0.5 * a[3])
    # a term whose every weight is zero is zero, and so are its gradients
    z = on_device(c, gpu)
    total, terms = rigid.rigid_terms(z.prev, z.curr, nb, torch.zeros_like(z.w), z.d0)
    total.backward()
    assert float(total.detach()) == 0.0 and not bool(terms.means.any()) and not bool(z.curr.grad.any()) and not bool(z.prev.grad.any())


@pytest.mark.gpu
def test_coincident_points_are_finite_with_zero_gradients(gpu):
    """curr_i == curr_j and prev_i == prev_j on every edge (a table over duplicates): sqrt(0 + 1e-16) keeps both terms
    finite, and every gradient term is 0 / 1e-8 = 0"""
    from gftorf_amd import rigid
    P, K = 600, 3
    base = R.clouds(P // 4, "uniform", seed=4)
    prev = np.concatenate([base] * 4)
    curr = np.concatenate([base + np.float32(0.25)] * 4)
    nb = rigid.Neighbours.build(torch.tensor(prev, device=gpu), K)
    assert not bool(nb.dist2.any())                            # the three duplicates, at distance 0
    p, q = (torch.tensor(a, device=gpu, requires_grad=True) for a in (prev, curr))
    w = torch.full((P, K), 0.7, device=gpu)
    total, terms = rigid.rigid_terms(p, q, nb, w, nb.dist2)
    total.backward()
    assert bool(torch.isfinite(terms.means).all()) and float(terms.means[0]) == pytest.approx(0.7e-8, rel=1e-5)
    assert float(terms.means[1]) == 0.0
    assert not bool(p.grad.any()) and not bool(q.grad.any())


@pytest.mark.gpu
def test_captured_step_follows_positions_moved_in_place(gpu):
    """forward and backward in one graph; curr and prev are rewritten in place between replays, and every replay equals an
    eager call on the same contents bit for bit"""
    from gftorf_amd import rigid
    c = case("u1025")
    t = on_device(c, gpu)
    nb = rigid.Neighbours.from_indices(t.idx)
    wt = torch.tensor([4.0, 2.0], device=gpu)

    def step(t, wt):
        total, terms = rigid.rigid_terms(t.prev, t.curr, nb, t.w, t.d0, weights=wt)
        (0.5 * total).backward()
        return torch.cat([total.detach().reshape(1), terms.means])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            t.prev.grad = t.curr.grad = None
            step(t, wt)
    torch.cuda.current_stream().wait_stream(side)
    t.prev.grad = t.curr.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(t, wt)
    rng = np.random.default_rng(8)
    for move in (None, 0.01, 0.3):
        if move is not None:
            with torch.no_grad():
                t.curr.add_(torch.tensor(rng.normal(0, move, c["curr"].shape).astype(np.float32), device=gpu))
                t.prev.mul_(1.0 + move)
                wt.mul_(1.5)
        graph.replay()
        torch.cuda.synchronize()
        e = on_device(c, gpu)
        with torch.no_grad():
            e.prev.copy_(t.prev), e.curr.copy_(t.curr)
        eager = step(e, wt.clone())
        assert torch.equal(out, eager), move
        assert torch.equal(t.curr.grad, e.curr.grad) and torch.equal(t.prev.grad, e.prev.grad), move
        assert float(out[0]) > 0


@pytest.mark.gpu
def test_chain_through_torch_vs_eager_statements(gpu):
    """curr = xyz[mask] + d_xyz, the two losses, backward to d_xyz: against the reference's statements run by torch on the
    device, at the gradient bound (the statements' own float32 error is inside 4 * e_ref)"""
    from gftorf_amd import rigid
    c = case("c3000")
    P = c["prev"].shape[0]
    rng = np.random.default_rng(12)
    mask = np.zeros(2 * P, bool)
    mask[rng.permutation(2 * P)[:P]] = True
    xyz = np.zeros((2 * P, 3), np.float32)
    xyz[mask] = c["prev"]
    t = on_device(c, gpu, grad=False)
    nb = rigid.Neighbours.from_indices(t.idx)
    grads = []
    for fused in (True, False):
        d_xyz = torch.tensor(c["curr"] - c["prev"], device=gpu, requires_grad=True)
        curr = torch.tensor(xyz, device=gpu)[torch.tensor(mask, device=gpu)] + d_xyz
        if fused:
            loss = rigid.rigid_terms(t.prev, curr, nb, t.w, t.d0, 4.0, 2.0)[0]
        else:
            rig, iso = statements(t.prev, curr, t.idx, t.w, t.d0)
            loss = 4.0 * rig + 2.0 * iso
        loss.backward()
        grads.append((loss.item(), d_xyz.grad.cpu().numpy().astype(np.float64)))
    # (curr here is xyz + (curr - prev) rounded once more: not the golden curr to the bit, so the yardstick is the eager
    # device result, held to both terms' bounds)
    bound = 4.0 * grad_bound(c, "rig_g_curr") + 2.0 * grad_bound(c, "iso_g_curr")
    err = np.abs(grads[0][1] - grads[1][1]).max()
    print("rigid chain: |fused - eager| %.3g / %.3g; loss %.9g vs %.9g" % (err, bound, grads[0][0], grads[1][0]))
    assert err <= bound
    assert grads[0][0] == pytest.approx(grads[1][0], rel=4 * (c["e_ref"]["rig"] + c["e_ref"]["iso"]) + 2.0 ** -22)


@pytest.mark.gpu
def test_a_table_out_of_range_raises_before_any_launch(gpu):
    from gftorf_amd import _lib, rigid
    c = case("u21")
    t = on_device(c, gpu)
    lib = _lib.load()
    for bad in (-1, 21):
        for dtype in (torch.int32, torch.int64):
            idx = t.idx.to(dtype).clone()
            idx[7, 3] = bad
            calls = []
            real = lib.gft_rigid_forward
            lib.gft_rigid_forward = lambda *a: calls.append(a) or real(*a)
            try:
                with pytest.raises(ValueError, match=r"outside \[0, 21\)"):
                    rigid.Neighbours.from_indices(idx)
                with pytest.raises(ValueError, match=r"outside \[0, 21\)"):
                    rigid.rigidity_loss(t.w, t.prev, t.curr, idx)
            finally:
                lib.gft_rigid_forward = real
            assert not calls
    assert t.curr.grad is None and t.prev.grad is None
