"""gftorf_amd.query: the deformation queries of an iteration as one call -- scene/gaussian_model.py:170-174 with what
train.py:164-177, 248, 255 (and training_report, :520-532) do around it.

Yardsticks:
  inputs        eager torch on the device: `(xyz / extent)[mask]`, bit for bit
  combinations  the reference's statements run by torch (train.py:176, 249, 256), bit for bit; the backward against the
                ordered float32 expression (bit for bit) and against the float64 sum within 3 * 2^-24 * sum_m |C[m,k] g_m|,
                the bound of a sum of up to three rounded products
  the network   K separate DeformNetwork calls (bit for bit: a point's result does not depend on its batch), the
                reference's own module through tests/golden/query.npz (make_golden_query.py) and oracle/deform_ref in
                float64, under FWD_TOL / BWD_TOL of tests/test_deform.py: the same kernels and the same kind of sums
"""
import ctypes as C
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from helpers import DEFORM_BLOCKING, deform_modes
from oracle import deform_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_query.h")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "query.npz")
FWD_TOL = 3e-6      # tests/test_deform.py:161
BWD_TOL = 2e-5      # tests/test_deform.py:162
EPS24 = 2.0 ** -24

FLOW = [[1.0, 0.0, 0.0], [-1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]]            # d_xyz, d_xyz_next - d_xyz, d_xyz_prev - d_xyz
LERPS = {r: [[0.25 * (4 - r), 0.25 * r]] for r in (1, 2, 3)}            # frame curr + r between curr and curr + 4
MATRICES = {"lerp1": LERPS[1], "lerp2": LERPS[2], "lerp3": LERPS[3], "flow": FLOW}


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / max(np.abs(b).max(), 1e-30))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


# ---- the restatements ------------------------------------------------------------------------------------------------------

def reference_statements(query_dmlp, frame_id, total_num_views, sync, forward_flow, backward_flow):
    """train.py:169-176, 248-249, 255-256 word for word (`sync`: iteration <= opt.optimize_sync_iters; the flags:
    viewpoint_cam.forward_flow / backward_flow is not None, inside the window of :243)."""
    out = {}
    curr_int_fid = (frame_id // 4) * 4
    next_int_fid = (frame_id // 4 + 1) * 4
    d_xyz_curr = query_dmlp(curr_int_fid / (total_num_views - 1))
    if frame_id % 4 == 0 or sync:
        d_xyz = d_xyz_curr
    else:
        d_xyz_next = query_dmlp(next_int_fid / (total_num_views - 1))
        d_xyz = 0.25 * ((frame_id - curr_int_fid) * d_xyz_next + (next_int_fid - frame_id) * d_xyz_curr)
    out["d_xyz"] = d_xyz
    if frame_id % 4 == 0:
        if forward_flow:
            d_xyz_next = query_dmlp((frame_id + 4) / (total_num_views - 1))
            out["flow_next"] = d_xyz_next - d_xyz
        if backward_flow:
            d_xyz_prev = query_dmlp((frame_id - 4) / (total_num_views - 1))
            out["flow_prev"] = d_xyz_prev - d_xyz
    return out


def apply_rows(matrix, blocks, transpose=False):
    """The documented rule with torch: every product rounded, the terms added in increasing index, a coefficient that is
    exactly 0 skipped (its block may be None), nothing left: zeros.  `transpose`: sum over the rows (the backward)."""
    M, K = len(matrix), len(matrix[0])
    like = next(b for b in blocks if b is not None)
    outs = []
    for r in range(K if transpose else M):
        acc = None
        for s in range(M if transpose else K):
            c = matrix[s][r] if transpose else matrix[r][s]
            if c == 0.0 or blocks[s] is None:
                continue
            p = c * blocks[s]
            acc = p if acc is None else acc + p
        outs.append(acc if acc is not None else torch.zeros_like(like))
    return outs


# ---- not GPU ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from gftorf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from gftorf_amd import build
        build.build()
    return _lib.load()


def test_header_is_plain_c_and_every_symbol_is_exported(tmp_path, lib):
    from gftorf_amd import _lib, build
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gft_[a-z_0-9]+)\s*\(", src)))
    assert names and all(n.startswith("gft_query_") for n in names)
    assert set(names) == set(_lib.QUERY_EXPORTS), names
    assert not set(names) & (set(_lib.EXPORTS) | set(_lib.FLOW_EXPORTS) | set(_lib.FEATURE_EXPORTS) | set(_lib.REG_EXPORTS)
                             | set(_lib.TOF_EXPORTS))
    for n in names:
        assert hasattr(lib, n), n
    assert "k_query.hip" in build.SOURCES
    prog = tmp_path / "query_abi.c"
    prog.write_text("\n".join(['#include <stdio.h>', '#include "gftorf_query.h"', 'int main(void){',
                               'void* f[] = {%s};' % ", ".join("(void*)%s" % n for n in names),
                               'printf("%d\\n", (int)(sizeof(f) / sizeof(f[0]))); return 0;}']))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(prog), "-o", str(tmp_path / "query_abi.o")])
    out = subprocess.check_output(["gcc", "-std=c99", "-E", "-P", "-I", os.path.join(ROOT, "include"), "-include", "gftorf_query.h",
                                   "-x", "c", "-"], input="QUERY_LIMITS_ARE GFT_QUERY_MAX_TIMES GFT_QUERY_MAX_OUTPUTS\n", text=True)
    assert [int(v) for v in out.split("QUERY_LIMITS_ARE", 1)[1].split()] == [_lib.QUERY_MAX_TIMES, _lib.QUERY_MAX_OUTPUTS] == [4, 4]
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16               # no struct in the header: the version stays


def test_argument_errors_of_the_c_entry_points(lib):
    from gftorf_amd import _lib
    x = C.c_void_p(16)                        # never dereferenced: the calls fail before any launch
    host = (C.c_float * 16)()
    inputs = lambda P=8, xyz=x, mask=x, rank=x, count=x, n=4, K=2, tdev=None, thost=host, ox=x, ot=x: lib.gft_query_inputs(
        None, P, xyz, mask, rank, count, n, K, 0.5, tdev, thost, ox, ot)
    for K in (0, -1, 5):
        assert inputs(K=K) != 0
        assert "K=%d is not in 1..4" % K in _lib.last_error()
    for kw in (dict(n=-1), dict(P=-1), dict(n=1 << 31), dict(P=1 << 31)):
        assert inputs(**kw) != 0
        assert "bad row counts" in _lib.last_error(), kw
    for kw in (dict(mask=None), dict(rank=None), dict(count=None), dict(mask=None, rank=None)):
        assert inputs(**kw) != 0
        assert "come together or not at all" in _lib.last_error(), kw
    assert inputs(thost=None) != 0
    assert "times_dev and times_host are both NULL" in _lib.last_error()
    for kw in (dict(ox=None), dict(ot=None), dict(xyz=None)):
        assert inputs(**kw) != 0
        assert "NULL argument" in _lib.last_error(), kw
    assert inputs(n=0) == 0 and inputs(n=0, ox=None, ot=None, xyz=None) == 0             # nothing to launch
    table = lambda *p: (C.c_void_p * len(p))(*p)
    fwd = lambda n=4, K=2, M=3, d=x, cdev=None, chost=host, out=table(16, 16, 16, 16): lib.gft_query_combine(None, n, K, M, d, cdev, chost, out)
    bwd = lambda n=4, K=2, M=3, g=table(16, None, 16, 16), cdev=None, chost=host, gd=x: lib.gft_query_combine_backward(
        None, n, K, M, g, cdev, chost, gd)
    for call, who in ((fwd, "gft_query_combine"), (bwd, "gft_query_combine_backward")):
        for K in (0, 5):
            assert call(K=K) != 0
            assert "%s: K=%d is not in 1..4" % (who, K) in _lib.last_error()
        for M in (0, 5):
            assert call(M=M) != 0
            assert "%s: M=%d is not in 1..4" % (who, M) in _lib.last_error()
        assert call(n=-1) != 0
        assert "%s: bad row count" % who in _lib.last_error()
        assert call(chost=None) != 0
        assert "coeffs_dev and coeffs_host are both NULL" in _lib.last_error()
        assert call(n=0) == 0
    assert fwd(d=None) != 0 and "NULL argument" in _lib.last_error()
    assert fwd(out=None) != 0 and "NULL argument" in _lib.last_error()
    assert fwd(out=table(16, None, 16)) != 0 and "out[1] is NULL" in _lib.last_error()
    assert bwd(g=None) != 0 and "NULL argument" in _lib.last_error()
    assert bwd(gd=None) != 0 and "NULL argument" in _lib.last_error()


def test_wrapper_rejects_cpu_tensors_shapes_dtypes_and_gradients():
    from gftorf_amd import DeformNetwork, DeformQuery, query
    net = DeformNetwork()
    xyz = torch.zeros(6, 3)
    with pytest.raises(RuntimeError, match="motion_mask is on cpu; the query kernels run on a HIP device only, there is no CPU path"):
        DeformQuery(torch.zeros(6, dtype=torch.bool))
    with pytest.raises(TypeError, match="motion_mask must be torch.bool"):
        DeformQuery(torch.zeros(6))
    with pytest.raises(RuntimeError, match=r"motion_mask must be a contiguous \[P\] tensor"):
        DeformQuery(torch.zeros(6, 1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match=r"motion_mask must be a contiguous \[P\] tensor"):
        DeformQuery(torch.zeros(12, dtype=torch.bool)[::2])
    q = DeformQuery(None)
    for call in (lambda: q.plan(net, xyz, 2.0, [0.5]), lambda: q.plan(net, xyz, 2.0, [0.0, 0.5], LERPS[1]),
                 lambda: q.inputs(xyz, 2.0, [0.5, 0.25, 0.0]),
                 lambda: query.query_dmlp(_Pc(net, xyz, torch.ones(6, dtype=torch.bool)), 0.5, plan=q)):
        with pytest.raises(RuntimeError, match="xyz is on cpu; the query kernels run on a HIP device only, there is no CPU path"):
            call()
    shapes = [(lambda: q.plan(net, torch.zeros(6, 2), 2.0, [0.5]), r"xyz must be \[P, 3\]"),
              (lambda: q.plan(net, torch.zeros(18), 2.0, [0.5]), r"xyz must be \[P, 3\]"),
              (lambda: q.plan(net, xyz, 2.0, []), r"times must be \[K\] with 1 <= K <= 4, got \[0\]"),
              (lambda: q.plan(net, xyz, 2.0, [0.1] * 5), r"times must be \[K\] with 1 <= K <= 4, got \[5\]"),
              (lambda: q.plan(net, xyz, 2.0, torch.zeros(2, 1)), r"times must be \[K\]"),
              (lambda: q.inputs(xyz, 2.0, torch.zeros(5)), r"times must be \[K\]"),
              (lambda: q.plan(net, xyz, 2.0, [0.1, 0.2], FLOW), r"combine must be \[M, 2\] with 1 <= M <= 4, got \[3, 3\]"),
              (lambda: q.plan(net, xyz, 2.0, [0.1, 0.2], [[1.0, 0.0]] * 5), r"combine must be \[M, 2\]"),
              (lambda: q.plan(net, xyz, 2.0, [0.1, 0.2], torch.zeros(2)), r"combine must be \[M, 2\]"),
              (lambda: q.plan(net, xyz, 2.0, [0.1, 0.2], [[1.0, 0.0], [1.0]]), r"rows of combine differ in length")]
    for call, msg in shapes:
        with pytest.raises(RuntimeError, match=msg):
            call()
    dtypes = [(lambda: q.plan(net, xyz.double(), 2.0, [0.5]), "xyz must be torch.float32"),
              (lambda: q.plan(net, xyz, 2.0, torch.zeros(2, dtype=torch.float64)), "times must be torch.float32"),
              (lambda: q.plan(net, xyz, 2.0, [0.1, 0.2], torch.zeros(1, 2, dtype=torch.float16)), "combine must be torch.float32"),
              (lambda: q.plan(net, xyz, 2.0, 0.5), "times must be a float32 device tensor or a list of numbers"),
              (lambda: q.plan(net, xyz, 2.0, [0.1, 0.2], [1.0, 0.0]), "combine must be a float32 device tensor or a nested list"),
              (lambda: q.plan(torch.nn.Linear(3, 3), xyz, 2.0, [0.5]), "net must be a gftorf_amd.DeformNetwork"),
              (lambda: q.plan(net, [[0.0, 0.0, 0.0]], 2.0, [0.5]), "xyz must be a tensor")]
    for call, msg in dtypes:
        with pytest.raises(TypeError, match=msg):
            call()
    with pytest.raises(ValueError, match="sh_of must be None or an index into the 2 times"):
        q.plan(net, xyz, 2.0, [0.1, 0.2], sh_of=2)
    with pytest.raises(NotImplementedError, match="gradients flow to the network's parameters only; times requires grad"):
        q.plan(net, xyz, 2.0, torch.zeros(2, requires_grad=True))
    with pytest.raises(NotImplementedError, match="combine requires grad"):
        q.plan(net, xyz, 2.0, [0.1, 0.2], torch.zeros(1, 2, requires_grad=True))
    with pytest.raises(NotImplementedError, match="times requires grad"):
        q.inputs(xyz, 2.0, torch.zeros(2, requires_grad=True))


class _Pc:
    """What query_dmlp reads of a GaussianModel."""

    def __init__(self, net, xyz, mask, extent=2.0):
        import types
        self._xyz, self.get_motion_mask, self.scene_extent = xyz, mask, extent
        self.deform_model = types.SimpleNamespace(deform=net)


@pytest.mark.parametrize("frame_id", range(12))
def test_ftorf_schedule_reproduces_the_training_statements(frame_id):
    """Every frame of 12 views and every flag combination: the schedule's rows applied to random tensors by the documented
    rule against the literal statements, bit for bit -- and the times in the order the statements query them."""
    from gftorf_amd import ftorf_schedule
    for sync, ff, bf in itertools.product((False, True), repeat=3):
        gen = torch.Generator().manual_seed(100 * frame_id + 4 * sync + 2 * ff + bf)
        asked, blocks = [], []

        def query_dmlp(fid):
            asked.append(fid)
            blocks.append(torch.randn((257, 3), generator=gen) * 10.0 ** float(torch.randint(-4, 5, (1,), generator=gen)))
            return blocks[-1]

        ref = reference_statements(query_dmlp, frame_id, 12, sync, ff, bf)
        times, combine, names = ftorf_schedule(frame_id, 12, sync=sync, forward_flow=ff, backward_flow=bf)
        what = (frame_id, sync, ff, bf)
        assert times == asked, what
        assert names == tuple(ref) and names[0] == "d_xyz", what
        assert len(combine) == len(names) and all(len(r) == len(times) for r in combine), what
        assert 1 <= len(times) <= 4 and len(names) <= 4
        outs = apply_rows(combine, blocks)
        for name, o in zip(names, outs):
            assert _same_bits(o, ref[name]), (what, name)
        if frame_id % 4 == 0 or sync:
            assert outs[0] is blocks[0] or _same_bits(outs[0], blocks[0])        # d_xyz = d_xyz_curr
            assert combine[0] == [1.0] + [0.0] * (len(times) - 1)
    # training_report (train.py:525-532) is the unsynchronised schedule without flows
    times, combine, names = ftorf_schedule(frame_id, 12)
    assert names == ("d_xyz",) and len(times) == (1 if frame_id % 4 == 0 else 2)


def _case(g, case):
    names = [str(n) for n in g[case + ":names"]]
    return dict(frame_id=int(g[case + ":frame_id"]), times=[float(t) for t in g[case + ":times"]], names=names,
                outs=[g["%s:out:%s" % (case, n)] for n in names], gs=[g["%s:g:%s" % (case, n)] for n in names],
                grad_none=sorted(g[case + ":grad_none"].tolist()),
                grads={k.split(":", 2)[2]: (k.split(":")[1], g[k]) for k in g.files if k.startswith(case + ":grad")
                       and not k.endswith("grad_none")})


def _case_schedule(c):
    from gftorf_amd import ftorf_schedule
    if c["names"] == ["d_xyz", "d_sh"]:
        return c["times"], None
    times, combine, names = ftorf_schedule(c["frame_id"], 12, forward_flow=True, backward_flow=True)
    assert times == c["times"] and list(names) == c["names"]
    return times, combine


@pytest.mark.parametrize("case", ["lerp", "flow", "torf"])
def test_fixture_agrees_with_the_float64_oracle(case):
    """query.npz (the reference's module and statements, float32) against oracle/deform_ref in float64 over the batched rows
    plus the combination: the fixture and the oracle say the same."""
    g = np.load(GOLDEN)
    c = _case(g, case)
    params = deform_ref.random_params(int(g["seed"]))
    assert float(g["scene_extent"]) == 4.0 and g["xyz"].shape == (48, 3)
    x = g["xyz"] / np.float32(g["scene_extent"])
    np.testing.assert_array_equal(x, g["x"])
    times, combine = _case_schedule(c)
    K, n = len(times), x.shape[0]
    X = np.concatenate([x] * K)
    T = np.concatenate([np.full((n, 1), np.float32(t), np.float32) for t in times])
    assert min(deform_ref.relu_margin(params, X, T)) > 1e-6
    d_xyz, _, d_sh, _ = deform_ref.forward(params, X, T, dtype=np.float64)
    g_dxyz, g_dsh = np.zeros((K * n, 3)), np.zeros((K * n, 16, 3))
    if combine is None:
        outs = [d_xyz, d_sh]
        g_dxyz, g_dsh = c["gs"][0].astype(np.float64), c["gs"][1].astype(np.float64)
    else:
        outs = [sum(combine[m][k] * d_xyz[k * n:(k + 1) * n] for k in range(K)) for m in range(len(combine))]
        for k in range(K):
            g_dxyz[k * n:(k + 1) * n] = sum(combine[m][k] * c["gs"][m].astype(np.float64) for m in range(len(combine)))
    for name, o, ref in zip(c["names"], outs, c["outs"]):
        assert _rel(ref, o) < FWD_TOL, (name, _rel(ref, o))
    grads = deform_ref.backward(params, X, T, g_dxyz, g_dsh, dtype=np.float64)
    heads_unused = [] if combine is None else [h + s for h in ("r", "g", "b") for s in (".weight", ".bias")]
    assert c["grad_none"] == sorted([k for k, v in grads.items() if v is None] + heads_unused)
    assert len(c["grads"]) == 24 - len(heads_unused)
    for name, (kind, ref) in c["grads"].items():
        got = grads[name] if kind == "grad" else grads[name][::8, ::4]
        assert _rel(ref, got) < BWD_TOL, (name, _rel(ref, got))


# ---- GPU -------------------------------------------------------------------------------------------------------------------

def _net(seed, dev):
    from gftorf_amd.deform import DeformNetwork
    params = deform_ref.random_params(seed)
    net = DeformNetwork(D=8, W=256, xyz_multires=10, t_multires=10, sh_degree=3)
    net.load_state_dict({k: torch.tensor(v) for k, v in params.items()})
    return net.to(dev), params


def _mask(kind, P, seed=0):
    if kind == "none":
        return torch.zeros(P, dtype=torch.bool)
    if kind == "all":
        return torch.ones(P, dtype=torch.bool)
    if kind == "alternating":
        return torch.arange(P) % 2 == 0
    if kind == "last":
        return torch.arange(P) == P - 1
    return torch.rand(P, generator=torch.Generator().manual_seed(seed)) < 0.3


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["none", "all", "alternating", "last", "random"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 5000])
def test_inputs_equal_eager_torch_bit_for_bit(P, kind, gpu):
    from gftorf_amd import DeformQuery
    extent = 3.7                                                   # its fp32 reciprocal is inexact: multiply and divide differ
    gen = torch.Generator().manual_seed(P)
    xyz = (torch.randn((P, 3), generator=gen) * 10.0 ** torch.randint(-3, 3, (P, 1), generator=gen).float()).to(gpu)
    mask = _mask(kind, P, seed=P).to(gpu)
    q = DeformQuery(mask)
    want = (xyz / extent)[mask]                                    # get_xyz_normalized[get_motion_mask]
    n = want.shape[0]
    assert q.n == n == int(mask.sum()) and int(q.count.item()) == n
    for K in (1, 3, 4):
        times = [0.0, 4 / 11, 8 / 11, 1.0909090909090908][:K]
        x, t = q.inputs(xyz, extent, times)
        assert x.shape == (K * n, 3) and t.shape == (K * n,) and x.dtype == t.dtype == torch.float32
        x_dev, t_dev = q.inputs(xyz, extent, torch.tensor(times, dtype=torch.float32, device=gpu))
        assert _same_bits(x, x_dev) and _same_bits(t, t_dev), K
        if n == 0:
            assert x.numel() == 0 and t.numel() == 0
            continue
        assert _same_bits(x, want.repeat(K, 1)), K
        assert _same_bits(t, torch.tensor(times, dtype=torch.float32, device=gpu).repeat_interleave(n)), K
    if kind == "all":                                              # None: every Gaussian is dynamic
        x, t = DeformQuery(None).inputs(xyz, extent, [0.25, 0.5])
        assert _same_bits(x, (xyz / extent).repeat(2, 1)) and _same_bits(t, torch.tensor([0.25, 0.5], device=gpu).repeat_interleave(P))
    if n == 0 or n == P:
        return
    # an in-place edit that keeps the count: refresh() follows it
    mask.copy_(mask.roll(1))
    assert q.refresh() is q and q.n == n
    x, t = q.inputs(xyz, extent, [0.5, 0.75])
    assert _same_bits(x, (xyz / extent)[mask].repeat(2, 1))
    # an edit that lowers the count: the surplus rows are the point 0, their times the times
    first = int(torch.nonzero(mask)[0, 0])
    mask[first] = False
    x, t = q.refresh().inputs(xyz, extent, [0.5, 0.75])
    left = (xyz / extent)[mask]
    assert left.shape[0] == n - 1 and q.n == n
    x = x.view(2, n, 3)
    for k in range(2):
        assert _same_bits(x[k, :n - 1], left) and not x[k, n - 1].any()
    assert _same_bits(t, torch.tensor([0.5, 0.75], device=gpu).repeat_interleave(n))
    # one that raises it: the rows beyond n are left out
    mask.fill_(True)
    x, _ = q.refresh().inputs(xyz, extent, [0.5])
    assert _same_bits(x, (xyz / extent)[:n])


def _combine(d, matrix, n, on_device):
    from gftorf_amd import query
    K, M = len(matrix[0]), len(matrix)
    host = [float(v) for r in matrix for v in r]
    if on_device:
        return query._Combine.apply(d, torch.tensor(matrix, dtype=torch.float32, device=d.device), None, n, K, M)
    return query._Combine.apply(d, None, host, n, K, M)


def _torch_statements(name, blocks):
    """train.py:176 / :173, 249, 256 on the device"""
    if name == "flow":
        d_xyz_curr, d_xyz_next, d_xyz_prev = blocks
        d_xyz = d_xyz_curr
        return [d_xyz, d_xyz_next - d_xyz, d_xyz_prev - d_xyz]
    frame_id, curr_int_fid, next_int_fid = 4 + int(name[-1]), 4, 8
    d_xyz_curr, d_xyz_next = blocks
    return [0.25 * ((frame_id - curr_int_fid) * d_xyz_next + (next_int_fid - frame_id) * d_xyz_curr)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_combinations_equal_the_torch_statements_bit_for_bit(n, name, gpu):
    matrix = MATRICES[name]
    M, K = len(matrix), len(matrix[0])
    gen = torch.Generator().manual_seed(7 * n + K)
    scale = 10.0 ** torch.randint(-4, 5, (K * n, 1), generator=gen).float()
    d = (torch.randn((K * n, 3), generator=gen) * scale).to(gpu).requires_grad_()
    blocks = [d.detach()[k * n:(k + 1) * n] for k in range(K)]
    want = _torch_statements(name, blocks)
    g_out = [torch.randn((n, 3), generator=gen).to(gpu) * 10.0 ** (m - 1) for m in range(M)]
    for on_device in (False, True):
        outs = _combine(d, matrix, n, on_device)
        assert len(outs) == M
        for m in range(M):
            assert _same_bits(outs[m].detach(), want[m]), (m, on_device)
        # backward: the ordered float32 expression, bit for bit; the float64 sum within the bound of a three-term sum
        d.grad = None
        torch.autograd.backward(list(outs), g_out)
        ordered = torch.cat(apply_rows(matrix, g_out, transpose=True))
        assert _same_bits(d.grad, ordered), on_device
        exact = torch.cat([sum(matrix[m][k] * g_out[m].double() for m in range(M)) for k in range(K)])
        bound = torch.cat([sum(abs(matrix[m][k]) * g_out[m].double().abs() for m in range(M)) for k in range(K)]) * 3 * EPS24
        assert bool(((d.grad.double() - exact).abs() <= bound).all())
    # outputs without a gradient count as zeros; a block nothing reaches is written as zeros
    if M > 1:
        d.grad = None
        outs = _combine(d, matrix, n, True)
        (outs[1] * g_out[1]).sum().backward()
        ordered = torch.cat(apply_rows(matrix, [None, g_out[1], None], transpose=True))
        assert _same_bits(d.grad, ordered) and not d.grad[2 * n:].any() and bool(d.grad[:2 * n].any())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_a_zero_coefficient_does_not_read_its_block(n, gpu):
    gen = torch.Generator().manual_seed(n)
    d = torch.randn((3 * n, 3), generator=gen).to(gpu)
    d[2 * n:] = float("nan")
    for on_device in (False, True):
        (lerp,) = _combine(d, [[0.75, 0.25, 0.0]], n, on_device)
        assert _same_bits(lerp, 0.25 * (1 * d[n:2 * n] + 3 * d[:n]))
        d_xyz, flow_next, zero = _combine(d, [[1.0, 0.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 0.0]], n, on_device)
        assert _same_bits(d_xyz, d[:n]) and _same_bits(flow_next, d[n:2 * n] - d[:n])             # (a single 1: a bit copy)
        assert bool(torch.isfinite(lerp).all()) and not zero.any()
        (poisoned,) = _combine(d, [[0.5, 0.0, 0.5]], n, on_device)
        assert bool(torch.isnan(poisoned).all())
    # the backward: an upstream NaN under a zero coefficient stays out as well
    dd = d.clone().requires_grad_()
    outs = _combine(dd, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], n, True)
    torch.autograd.backward(list(outs), [torch.ones((n, 3), device=gpu), torch.full((n, 3), float("nan"), device=gpu)])
    assert bool((dd.grad[:n] == 1).all()) and bool(torch.isnan(dd.grad[n:2 * n]).all()) and not dd.grad[2 * n:].any()


def _points(n, seed, dev, extent=2.5):
    rng = np.random.default_rng(seed)
    xyz = (rng.random((n, 3)).astype(np.float32) * 2 - 0.5) * np.float32(extent)
    return torch.tensor(xyz, device=dev), extent


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("n", [1, 65, 333])
def test_batched_blocks_equal_separate_calls_bit_for_bit(n, K, gpu):
    """A point's result does not depend on its batch (gftorf_deform.h): the K blocks of d_xyz and d_sh against K separate
    DeformNetwork.forward(x, t_k) calls with a per-row t."""
    from gftorf_amd import DeformQuery
    net, _ = _net(21, gpu)
    xyz, extent = _points(n, 300 + n, gpu)
    times = [4 / 11, 8 / 11, 0.0][:K]
    q = DeformQuery(None)
    with torch.no_grad():
        x, _ = q.inputs(xyz, extent, times[:1])
        for k in range(K):
            outs, d_sh = q.plan(net, xyz, extent, times, sh_of=k)
            assert len(outs) == K and d_sh.shape == (n, 16, 3)
            t_k = torch.full((n, 1), float(np.float32(times[k])), device=gpu)                   # one value per row
            d_xyz_k, _, d_sh_k, _ = net(x, t_k)
            assert _same_bits(outs[k], d_xyz_k) and _same_bits(d_sh, d_sh_k), k
        outs_dev, _ = q.plan(net, xyz, extent, torch.tensor(times, dtype=torch.float32, device=gpu))
        assert all(_same_bits(a, b) for a, b in zip(outs, outs_dev))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["lerp", "flow", "torf"])
def test_reference_fixture(case, gpu):
    """The reference's own module and statements (query.npz): outputs, parameter gradients and the parameters without one."""
    from gftorf_amd import DeformQuery, query
    g = np.load(GOLDEN)
    c = _case(g, case)
    net, _ = _net(int(g["seed"]), gpu)
    xyz = torch.tensor(g["xyz"], device=gpu)
    times, combine = _case_schedule(c)
    if case == "torf":
        d_xyz, d_rot, d_sh, d_sh_p = query.query_dmlp(_Pc(net, xyz, torch.ones(48, dtype=torch.bool, device=gpu), float(g["scene_extent"])),
                                                      times[0])
        assert d_rot.shape == (48, 4) and d_sh_p.shape == (48, 16, 2) and not d_rot.any() and not d_sh_p.any()
        outs = [d_xyz, d_sh]
    else:
        outs, none = DeformQuery(None).plan(net, xyz, float(g["scene_extent"]), times, combine)
        assert none is None
    for name, o, ref in zip(c["names"], outs, c["outs"]):
        err = _rel(o.detach().cpu().numpy(), ref)
        print("%s %s: %.3g of the max-norm" % (case, name, err))
        assert err < FWD_TOL, (name, err)
    sum((o * torch.tensor(gi, device=gpu)).sum() for o, gi in zip(outs, c["gs"])).backward()
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert sorted(k for k, v in grads.items() if v is None) == c["grad_none"]
    for name, (kind, ref) in c["grads"].items():
        got = grads[name].cpu().numpy()
        err = _rel(got if kind == "grad" else got[::8, ::4], ref)
        assert err < BWD_TOL, (name, err)


@functools.lru_cache(maxsize=None)
def _oracle_points(n, seed, times):
    """n points away from every ReLU edge at all the times (tests/test_deform.py:221-224), and the parameters"""
    params = deform_ref.random_params(seed)
    rng = np.random.default_rng(seed + n)
    cand = rng.random((n + n // 8, 3)).astype(np.float32)
    margin = np.min([deform_ref.relu_margin(params, cand, np.full((len(cand), 1), np.float32(t), np.float32)) for t in times], axis=0)
    keep = np.sort(np.argsort(-margin)[:n])
    assert margin[keep].min() > 1e-6
    return cand[keep]


@pytest.mark.gpu
def test_flow_iteration_against_the_float64_oracle(gpu):
    from gftorf_amd import DeformQuery, deform as D
    n, K = 333, 3
    times = (4 / 11, 8 / 11, 0.0)
    x = _oracle_points(n, 12, times)
    net, params = _net(12, gpu)
    rng = np.random.default_rng(5)
    gs = [rng.normal(size=(n, 3)).astype(np.float32) for _ in range(3)]
    outs, _ = DeformQuery(None).plan(net, torch.tensor(x, device=gpu), 1.0, list(times), FLOW)
    torch.autograd.backward(list(outs), [torch.tensor(gi, device=gpu) for gi in gs])
    assert D.last_backward_stats["points"] == K * n
    X = np.concatenate([x] * K)
    T = np.concatenate([np.full((n, 1), np.float32(t), np.float32) for t in times])
    d64 = deform_ref.forward(params, X, T, dtype=np.float64)[0]
    for m in range(3):
        want = sum(FLOW[m][k] * d64[k * n:(k + 1) * n] for k in range(K))
        assert _rel(outs[m].detach().cpu().numpy(), want) < FWD_TOL, m
    g_dxyz = np.concatenate([sum(FLOW[m][k] * gs[m].astype(np.float64) for m in range(3)) for k in range(K)])
    ref = deform_ref.backward(params, X, T, g_dxyz, np.zeros((K * n, 16, 3)), dtype=np.float64)
    for name, p in net.named_parameters():
        if ref[name] is None or name.split(".")[0] in ("r", "g", "b"):
            assert p.grad is None, name
        else:
            err = _rel(p.grad.cpu().numpy(), ref[name])
            assert err < BWD_TOL, (name, err)


@pytest.mark.gpu
def test_one_backward_and_one_gradient_bucket(gpu):
    from gftorf_amd import DeformQuery, deform as D
    n, K = 200, 3
    net, _ = _net(13, gpu)
    xyz, extent = _points(n, 9, gpu)
    times = [4 / 11, 8 / 11, 0.0]
    gen = torch.Generator().manual_seed(2)
    gs = [torch.randn((n, 3), generator=gen).to(gpu) for _ in range(3)]
    q = DeformQuery(None)
    outs, _ = q.plan(net, xyz, extent, times, FLOW)
    torch.autograd.backward(list(outs), gs)
    assert D.last_backward_stats["points"] == D.last_backward_stats["points_processed"] == K * n
    with_grad = [p for p in D._param_list(net) if p.grad is not None]
    assert len(with_grad) == 18
    bucket, scatter_back = D.flat_grad_bucket(net)
    store = with_grad[0].grad.untyped_storage().data_ptr()
    assert bucket.untyped_storage().data_ptr() == store and bucket.data_ptr() == with_grad[0].grad.data_ptr()
    assert all(p.grad.untyped_storage().data_ptr() == store for p in with_grad)
    assert bucket.numel() >= sum(p.numel() for p in with_grad)
    fused = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    # the unfused route: K calls, K backwards, autograd's sums -- no buffer of its own left to reduce in place
    net.zero_grad(set_to_none=True)
    x, _ = q.inputs(xyz, extent, times[:1])
    d = [net(x, torch.full((n, 1), float(np.float32(t)), device=gpu), zeros_as_scalars=True)[0] for t in times]
    torch.autograd.backward([d[0], d[1] - d[0], d[2] - d[0]], gs)
    assert D.last_backward_stats["points"] == n
    bucket2, _ = D.flat_grad_bucket(net)
    grads = [p.grad for p in D._param_list(net) if p.grad is not None]
    assert len({g_.untyped_storage().data_ptr() for g_ in grads}) > 1
    assert bucket2.untyped_storage().data_ptr() not in {g_.untyped_storage().data_ptr() for g_ in grads}
    for k, v in fused.items():                                     # the same gradients up to the order of the sums
        assert _rel(v.cpu().numpy(), dict(net.named_parameters())[k].grad.cpu().numpy()) < BWD_TOL, k


def _sparse_upstream(n, dev, seed=5):
    """Upstream gradients that are non-zero on 10 % of the rows of d_xyz and of flow_next; flow_prev gets none."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        keep = (torch.rand((n,), generator=g) < 0.1).to(dev)
        out.append(torch.randn((n, 3), generator=g).to(dev) * keep[:, None])
    return out


@pytest.mark.gpu
def test_rows_counted_on_the_device_give_the_blocking_selections_gradients(gpu):
    """n = 2731, K = 3: 8193 rows, the first count above the row selection's threshold.  As tests/test_deform.py holds it
    for single calls: the blocking selection on exactly the rows with a gradient against the rows counted on the device."""
    from gftorf_amd import DeformQuery, deform as D
    n, K = 2731, 3
    assert K * n == D._SPARSE_MIN_POINTS + 1
    xyz, extent = _points(n, 17, gpu)
    gs = _sparse_upstream(n, gpu)
    rows = int(((gs[0] != 0).any(1) | (gs[1] != 0).any(1)).sum() + (gs[1] != 0).any(1).sum())     # blocks curr, next; prev: none

    def step(net):
        outs, _ = DeformQuery(None).plan(net, xyz, extent, [4 / 11, 8 / 11, 0.0], FLOW)
        torch.autograd.backward([outs[0], outs[1]], gs)
        return {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}, dict(D.last_backward_stats)

    with deform_modes(**DEFORM_BLOCKING):
        ref_net, _ = _net(12, gpu)
        ref_net._save_state = {"fraction": 0.0}
        ref, st = step(ref_net)
        assert st["points"] == K * n and st["recomputed"] and st["points_processed"] == rows
    with deform_modes(**dict(DEFORM_BLOCKING, device_row_count=True)):
        net, _ = _net(12, gpu)
        got, st = step(net)
        assert st["points"] == K * n and st["recomputed"] and int(st["rows_on_device"].item()) == rows
        assert len(got) == len(ref) == 18
        for k in ref:
            assert torch.equal(got[k], ref[k]) and bool(got[k].any()), k


def _flow_step(q, net, xyz, extent, times, combine, gs):
    net.zero_grad(set_to_none=True)
    outs, _ = q.plan(net, xyz, extent, times, combine)
    torch.autograd.backward(list(outs[:len(gs)]), gs)
    return [o.detach().clone() for o in outs], {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [333, 2731])
def test_no_host_sync_and_reproducible(n, gpu):
    """K * n below and above the row selection's 8192: a second call and its backward read nothing on the host, and two runs
    give the same bits (the times and the matrix by value or from the device alike).  Above 8192 the first backward of a
    network runs dense and counts its rows, the later ones recompute the rows that count (deform.device_row_count "auto"):
    the two runs compared are later ones."""
    from gftorf_amd import DeformQuery
    net, _ = _net(14, gpu)
    P = 3 * n
    xyz, extent = _points(P, 23, gpu)
    mask = (torch.arange(P) % 3 == 1).to(gpu)
    q = DeformQuery(mask)
    assert q.n == n
    times = torch.tensor([4 / 11, 8 / 11, 0.0], device=gpu)
    combine = torch.tensor(FLOW, device=gpu)
    gs = _sparse_upstream(n, gpu)
    first = _flow_step(q, net, xyz, extent, times, combine, gs)     # warm-up: the library's first load is not the question
    _flow_step(q, net, xyz, extent, [4 / 11, 8 / 11, 0.0], FLOW, gs)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        q.refresh()
        second = _flow_step(q, net, xyz, extent, times, combine, gs)
        by_value = _flow_step(q, net, xyz, extent, [4 / 11, 8 / 11, 0.0], FLOW, gs)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert all(_same_bits(a, b) for a, b in zip(first[0], second[0])) and all(_same_bits(a, b) for a, b in zip(first[0], by_value[0]))
    assert sorted(first[1]) == sorted(second[1]) == sorted(by_value[1]) and len(second[1]) == 18
    for k in second[1]:
        assert _same_bits(second[1][k], by_value[1][k]) and bool(second[1][k].any()), k
        assert _rel(first[1][k].cpu().numpy(), second[1][k].cpu().numpy()) < BWD_TOL, k


def _capture_case(n, gpu, device_rows):
    """The query, a loss and backward captured on static tensors with `times` and `combine` on the device; between replays the
    times, the weights, xyz and the parameters are rewritten in place: every replay against the eager call on those values."""
    from gftorf_amd import DeformQuery
    net, _ = _net(15, gpu)
    others = [deform_ref.random_params(30 + k) for k in range(2)]
    P = 2 * n
    mask = (torch.arange(P) % 2 == 0).to(gpu)
    q = DeformQuery(mask)
    K = 2 if not device_rows else 3
    contents = []
    for k in range(3):
        xyz, extent = _points(P, 40 + k, gpu)
        if K == 2:
            times, comb = [4 * k / 11, (4 * k + 4) / 11], LERPS[k + 1]
        else:
            times, comb = [4 * k / 11, (4 * k + 4) / 11, (4 * k - 4) / 11], FLOW
        contents.append(dict(xyz=xyz, times=torch.tensor(times, dtype=torch.float32, device=gpu),
                             combine=torch.tensor(comb, dtype=torch.float32, device=gpu),
                             params=None if k == 0 else others[k - 1]))
    gs = _sparse_upstream(n, gpu)[:len(contents[0]["combine"])]
    static = {k: contents[0][k].clone() for k in ("xyz", "times", "combine")}

    def step(net_, c):
        net_.zero_grad(set_to_none=True)
        outs, _ = q.plan(net_, c["xyz"], extent, c["times"], c["combine"])
        loss = sum((o * g_).sum() for o, g_ in zip(outs, gs))
        loss.backward()
        return [o.detach() for o in outs] + [loss.detach()], {k: p.grad for k, p in net_.named_parameters() if p.grad is not None}

    with deform_modes(**(dict(device_row_count=True) if device_rows else {})):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step(net, static)
        torch.cuda.current_stream().wait_stream(side)
        net.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs, grads = step(net, static)
        for k, c in enumerate(contents):
            with torch.no_grad():
                for key in static:
                    static[key].copy_(c[key])
                if c["params"] is not None:
                    net.load_state_dict({name: torch.tensor(v) for name, v in c["params"].items()})
            graph.replay()
            torch.cuda.synchronize()
            eager_net, _ = _net(15, gpu)
            eager_net.load_state_dict(net.state_dict())
            want_outs, want_grads = step(eager_net, c)
            torch.cuda.synchronize()
            assert all(_same_bits(a, b) for a, b in zip(outs, want_outs)), k
            assert sorted(grads) == sorted(want_grads) and len(grads) == 18
            for name in grads:
                assert _same_bits(grads[name], want_grads[name]) and bool(grads[name].any()), (k, name)


@pytest.mark.gpu
def test_captured_query_follows_times_weights_positions_and_parameters(gpu):
    _capture_case(333, gpu, device_rows=False)


@pytest.mark.gpu
def test_captured_query_above_the_row_threshold_counts_its_rows_on_the_device(gpu):
    _capture_case(2731, gpu, device_rows=True)


# ---- a composed F-ToRF flow iteration ---------------------------------------------------------------------------------------

def _model(scene, dev, dyn_share=0.4):
    """What GaussianModel keeps (scene/gaussian_model.py:180-236) for a synthetic scene, with the getters render_flow reads."""
    import types
    g = scene["gaussians"]
    P = g["means3D"].shape[0]
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    leaf = lambda a: a.contiguous().clone().requires_grad_()
    shs, shs_p, op = t(g["shs"]), t(g["shs_p"]), t(g["opacities"]).reshape(P, 1)
    normalize = lambda r: torch.nn.functional.normalize(r, dim=-1)
    pc = types.SimpleNamespace(
        _xyz=leaf(t(g["means3D"])), _opacity=leaf(torch.log(op / (1 - op))), _scaling=leaf(torch.log(t(g["scales"]))),
        _rotation=leaf(t(g["rotations"]) * 1.7), _features_dc_color=leaf(shs[:, :1]), _features_rest_color=leaf(shs[:, 1:]),
        _features_dc_phase=leaf(shs_p[:, :1, :1]), _features_rest_phase=leaf(shs_p[:, 1:, :1]),
        _features_dc_amp=leaf(shs_p[:, :1, 1:]), _features_rest_amp=leaf(shs_p[:, 1:, 1:]),
        get_motion_mask=(torch.rand(P, generator=torch.Generator().manual_seed(1)) < dyn_share).to(dev),
        rotation_activation=normalize, active_sh_degree=3, use_view_dependent_phase=True, scene_extent=3.7)
    pc.get_xyz, pc.get_opacity, pc.get_scaling = pc._xyz.detach(), torch.sigmoid(pc._opacity.detach()), torch.exp(pc._scaling.detach())
    pc.get_rotation = normalize(pc._rotation.detach())
    pc.leaves = [v for k, v in vars(pc).items() if isinstance(v, torch.Tensor) and v.requires_grad]
    return pc


def _tof_camera(scene, dev, gt):
    import math
    import types
    cam = scene["cam"]
    W, H = scene["cfg"]["W"], scene["cfg"]["H"]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32, device=dev)
    fx = W / (2 * cam["tanfovx"])
    K = t([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]])
    return types.SimpleNamespace(tof_image_height=H, tof_image_width=W, FoVx_tof=2 * math.atan(cam["tanfovx"]),
                                 FoVy_tof=2 * math.atan(cam["tanfovy"]), world_view_transform_tof=t(cam["viewmatrix"]),
                                 full_proj_transform_tof=t(cam["projmatrix"]), camera_center_tof=t(cam["campos"]),
                                 znear=cam["znear"], zfar=cam["zfar"], depth_range=float(scene["depth_range"]),
                                 K=K, K_tof=K, world_view_transform=t(cam["viewmatrix"]), forward_flow=gt[0], backward_flow=gt[1])


@pytest.mark.gpu
def test_composed_ftorf_flow_iteration(gpu):
    """train.py:164-178, 237-261 on a flow frame from this package's pieces: plan -> assemble_parameters -> GaussianRasterizer
    on the ToF camera -> render_flow_pair -> flow_loss -> reg.motion_reg, then backward -- against the same iteration built
    from K separate network calls on `(xyz / extent)[mask]` and torch's statements.  The deformations are the same bits, so
    the images and the loss are; the network's gradients pass through the rasterizer's float atomics
    (tests/test_frames.py:56: 2e-3 of the max-norm)."""
    import helpers
    from gftorf_amd import DeformQuery, GaussianRasterizer, assemble_parameters, flow, ftorf_schedule, reg
    W, H, P = 64, 48, 3000
    scene = helpers.small_scene(P=P, W=W, H=H, seed=29)
    pc = _model(scene, gpu)
    mask = pc.get_motion_mask
    share = float(mask.float().mean())
    assert 0.35 < share < 0.45
    gen = torch.Generator().manual_seed(8)
    cam = _tof_camera(scene, gpu, [torch.randn((2, H, W), generator=gen).to(gpu) for _ in range(2)])
    targets = [torch.rand((3, H, W), generator=gen).to(gpu), torch.rand((7, H, W), generator=gen).to(gpu)]
    rast = GaussianRasterizer(raster_settings=helpers.gpu_settings(scene, gpu))
    bg_flow = torch.zeros((7, H, W), device=gpu)
    params = deform_ref.random_params(31, head_std=0.005)
    frame_id, total = 4, 12
    times, combine, names = ftorf_schedule(frame_id, total, forward_flow=True, backward_flow=True)
    assert names == ("d_xyz", "flow_next", "flow_prev")
    q = DeformQuery(mask)

    def iteration(fused):
        from gftorf_amd.deform import DeformNetwork
        net = DeformNetwork(D=8, W=256, xyz_multires=10, t_multires=10, sh_degree=3)
        net.load_state_dict({k: torch.tensor(v) for k, v in params.items()})
        net = net.to(gpu)
        for v in pc.leaves:
            v.grad = None
        if fused:
            (d_xyz, flow_next, flow_prev), _ = q.plan(net, pc._xyz, pc.scene_extent, times, combine)
        else:
            def query_dmlp(fid):                                   # gaussian_model.py:170-174
                t = torch.tensor(np.array([fid])).float().to(gpu).unsqueeze(0).expand(pc._xyz[mask].shape[0], -1)
                xyz = (pc._xyz / pc.scene_extent)[mask].detach()
                return net(xyz, t, zeros_as_scalars=True)[0]
            st = reference_statements(query_dmlp, frame_id, total, False, True, True)
            d_xyz, flow_next, flow_prev = st["d_xyz"], st["flow_next"], st["flow_prev"]
        ssp = torch.zeros((P, 3), device=gpu, requires_grad=True)
        m3, m2, op, sc, ro, shs, shp = assemble_parameters(
            pc._xyz, ssp, pc._opacity, pc._scaling, pc._rotation, pc._features_dc_color, pc._features_rest_color,
            pc._features_dc_phase, pc._features_rest_phase, pc._features_dc_amp, pc._features_rest_amp, mask, d_xyz, 0.0, 0.0, 0.0)
        out = rast(means3D=m3, means2D=m2, opacities=op, shs=shs, shs_p=shp, scales=sc, rotations=ro,
                   phase_offset=scene["phase_offset"], dc_offset=scene["dc_offset"])
        color, phasor, depth = out[0], out[1], out[2]
        imf, imb = flow.render_flow_pair(cam, pc, d_xyz.detach(), 0.0, flow_next, flow_prev, bg_flow)
        lf, lb = flow.flow_loss(depth.detach(), cam, imf, imb)
        loss = ((color - targets[0]).abs().mean() + 0.5 * (phasor - targets[1]).abs().mean() + 0.01 * (lf + lb)
                + 0.1 * reg.motion_reg(d_xyz))
        loss.backward()
        images = [t_.detach().clone() for t_ in (color, phasor, depth, imf, imb, d_xyz, flow_next, flow_prev)]
        return images, loss.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    iteration(True)                                                # (the first frame of a shape sizes its buffers)
    fused = iteration(True)
    ref = iteration(False)
    torch.cuda.synchronize()
    for name, a, b in zip(("color", "phasor", "depth", "flow image forward", "flow image backward") + names, fused[0], ref[0]):
        assert _same_bits(a, b), name
        assert bool(torch.isfinite(a).all()) and bool(a.any()), name
    assert _same_bits(fused[1], ref[1]) and np.isfinite(float(fused[1]))
    assert len(fused[2]) == 18 and set(fused[2]) <= set(ref[2])
    for k, v in fused[2].items():
        err = _rel(v.cpu().numpy(), ref[2][k].cpu().numpy())
        assert float(ref[2][k].abs().max()) > 0 and err < 2e-3, (k, err)
