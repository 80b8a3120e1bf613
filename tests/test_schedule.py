"""gftorf_amd.schedule: the run's schedule on the device (include/gftorf_schedule.h, csrc/k_schedule.hip).

A tick copies numbers and draws a background whose every bit torch defines, so there is no tolerance in this file but one: the
parameters of the composed training step, whose backward sums with float atomics (the bound tests/test_loop_graph.py uses
for graph against eager).  The background is compared with torch itself -- ``torch.manual_seed(it); torch.rand(...) * 2 - 1``
-- at the smallest sizes that reach every part of the mapping: fewer elements than one block of the fill, several blocks
with a ragged last one, the training frame, and the first size at which a thread of torch's fill draws a second time.
The learning rates are compared with the reference's own statements, recorded in tests/golden/schedule.npz
(tests/golden/make_schedule_golden.py).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gftorf_schedule.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "schedule.npz")


# ---- CPU-runnable checks ------------------------------------------------------------------------------------------------

def test_header_declares_the_exports():
    from gftorf_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"\b(gft_schedule_\w+)\s*\(", src)
    assert sorted(names) == sorted(_lib.SCHEDULE_EXPORTS) == ["gft_schedule_tick"], names
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    others = [getattr(_lib, t) for t in dir(_lib) if t.endswith("EXPORTS") and t != "SCHEDULE_EXPORTS"]
    assert not set(names) & {n for o in others for n in o}
    defines = {k: int(v) for k, v in re.findall(r"#define (GFT_SCHEDULE_\w+) (\d+)", src)}
    assert defines["GFT_SCHEDULE_MAX_DESTS"] == _lib.SCHEDULE_MAX_DESTS == 1024
    assert defines["GFT_SCHEDULE_STATE_WORDS"] == _lib.SCHEDULE_STATE_WORDS
    assert [defines["GFT_SCHEDULE_" + k.upper()] for k in _lib.SCHEDULE_KINDS] == [0, 1]
    for word in ("COUNTER", "ITERATION", "TICKET", "OVERRUN", "OVERRUNS"):
        assert defines["GFT_SCHEDULE_" + word] == getattr(_lib, "SCHEDULE_" + word) < _lib.SCHEDULE_STATE_WORDS
    assert lib.gft_abi_version() == _lib.ABI_VERSION == 16               # no struct that existed has changed


def test_header_is_plain_c_and_matches_ctypes(tmp_path):
    from gftorf_amd import _lib
    mirrors = {"gft_schedule_dest": _lib.ScheduleDest, "gft_schedule": _lib.Schedule}
    body = ['#include <stdio.h>', '#include <stddef.h>', '#include "gftorf_schedule.h"', 'int main(void){']
    for s, cls in mirrors.items():
        body.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f, _t in cls._fields_:
            body.append('printf("%s.%s %%zu\\n", offsetof(%s,%s));' % (s, f, s, f))
    body.append('return 0;}')
    prog, exe = tmp_path / "abi.c", tmp_path / "abi"
    prog.write_text("\n".join(body))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for s, cls in mirrors.items():
        assert int(out[s]) == C.sizeof(cls), s
        for f, _t in cls._fields_:
            assert int(out["%s.%s" % (s, f)]) == getattr(cls, f).offset, (s, f)
    assert C.sizeof(_lib.ScheduleDest) == 16                              # the kernel reads a destination as one 16-byte word


PHILOX_KNOWN = (
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


@pytest.mark.parametrize("counter,key,want", PHILOX_KNOWN)
def test_philox_known_answers(counter, key, want):
    from gftorf_amd import schedule
    assert " ".join("%08x" % w for w in schedule.philox4x32_10(counter, key)) == want


def test_background_restatement_shape_and_range():
    """The host restatement: every element in [-1, 1), element e of thread idx, draw j at idx + T (4 j + k)"""
    from gftorf_amd import schedule
    T = 8
    b = schedule.background(5, 4 * T + 3, T)                             # one whole draw of every thread and a ragged second
    assert b.dtype == np.float32 and b.shape == (35,) and (b >= -1).all() and (b < 1).all()
    for e, (idx, j, k) in ((0, (0, 0, 0)), (T + 2, (2, 0, 1)), (4 * T + 1, (1, 1, 0))):
        v = schedule.philox4x32_10((j, 0, idx, 0), (5, 0))[k]
        assert b[e] == np.float32(2.0 ** -32 + np.float32(v) * np.float32(2.0 ** -32)) * 2 - 1
    assert not np.array_equal(b, schedule.background(6, 4 * T + 3, T))


def expon_lr(lr_init, lr_final, lr_delay_mult, max_steps):
    """The published schedule the reference uses (Plenoxels / 3D Gaussian Splatting ``get_expon_lr_func`` with no delay
    steps), restated: numpy double arithmetic"""
    def helper(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        t = np.clip(step / (max_steps if max_steps != 0 else 1), 0, 1)
        return 1.0 * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)
    return helper


def golden_updates(z, gaussians, deform):
    """``update_learning_rate`` of both models restated over two optimizers with the fixture's groups"""
    s = dict(zip(z["settings"].tolist(), z["values"].tolist()))
    extent = float(z["scene_extent"])
    steps = s["position_lr_max_steps"]
    xyz = expon_lr(s["position_lr_init"] * extent, s["position_lr_final"] * extent, s["position_lr_delay_mult"], steps)
    phase = expon_lr(s["feature_phase_lr_init"] * extent, s["feature_phase_lr_final"] * extent, s["position_lr_delay_mult"], steps)
    amp = expon_lr(s["feature_amp_lr_init"] * extent ** 2, s["feature_amp_lr_final"], s["position_lr_delay_mult"], steps)
    net = expon_lr(s["deform_lr_init"], s["deform_lr_final"], s["position_lr_delay_mult"], steps - s["warm_up"])

    def update(it):
        for g in gaussians.param_groups:
            lr = g["lr"]
            if g["name"] == "xyz":
                lr = xyz(it)
            if g["name"] in ("phase_f_dc", "phase_f_rest"):
                lr = phase(it)
            if g["name"] in ("amp_f_dc", "amp_f_rest"):
                lr = amp(it)
            if it > s["optimize_offset_start"]:
                if g["name"] == "phase_offset":
                    lr = s["phase_offset_lr"]
                if g["name"] == "dc_offset":
                    lr = s["dc_offset_lr"]
            g["lr"] = lr

    def update_net(it):
        deform.param_groups[0]["lr"] = net(it - s["warm_up"])

    return update, update_net, s


def test_record_lrs_against_the_reference():
    from gftorf_amd import schedule
    z = np.load(GOLDEN)
    names, rates, first = z["names"].tolist(), z["rates"], int(z["first_iter"])
    assert rates.dtype == np.float64 and rates.shape == (7000, len(names)) and z["deform"].shape == (7000,)
    gaussians = torch.optim.Adam([{"params": [torch.zeros(1, requires_grad=True)], "lr": float(lr), "name": n}
                                  for n, lr in zip(names, z["initial"])], lr=0.0, eps=1e-15)
    deform = torch.optim.Adam([{"params": [torch.zeros(1, requires_grad=True)], "lr": float(z["deform_initial"]), "name": "deform"}],
                              lr=0.0, eps=1e-15)
    update, update_net, s = golden_updates(z, gaussians, deform)
    # the fixture has what the issue asks for: both sides of the offsets' window and of the warm-up
    off, start, warm = names.index("phase_offset"), int(s["optimize_offset_start"]), int(s["warm_up"])
    assert rates[start - first, off] == 0.0 and rates[start + 1 - first, off] == s["phase_offset_lr"] > 0
    assert z["deform"][warm - 1 - first] == 0.0 and abs(z["deform"][warm - first] / s["deform_lr_init"] - 1) < 1e-12
    run = schedule.RunSchedule("cuda", first, first + 6999, bg_shape=(7, 4, 4))
    kept = [dict(g) for g in gaussians.param_groups], [dict(g) for g in deform.param_groups]
    got = run.record_lrs(gaussians, update)
    got_net = run.record_lrs(deform, update_net)
    assert got.dtype == np.float64 and got.shape == rates.shape
    assert np.array_equal(got.view(np.uint64), rates.view(np.uint64))                 # every float64, every bit
    assert np.array_equal(got_net[:, 0].view(np.uint64), z["deform"].view(np.uint64))
    for before, opt in zip(kept, (gaussians, deform)):
        assert len(before) == len(opt.param_groups)
        for a, b in zip(before, opt.param_groups):
            assert a.keys() == b.keys() and all(a[k] is b[k] or a[k] == b[k] for k in a if k != "params")
            assert all(p is q for p, q in zip(a["params"], b["params"])) and type(a["lr"]) is type(b["lr"])
    assert run.names[:2] == ["lr:0:xyz", "lr:0:f_dc_color"] and run.names[-1] == "lr:1:deform" and len(run.names) == len(names) + 1


def test_refusals_and_no_cpu_path():
    from gftorf_amd import _lib, schedule, FusedAdam
    with pytest.raises(RuntimeError, match="no CPU path"):
        schedule.RunSchedule("cpu", 1, 10)
    with pytest.raises(ValueError, match="lies before first_iter"):
        schedule.RunSchedule("cuda", 5, 4)
    with pytest.raises(ValueError, match="bg_shape"):
        schedule.RunSchedule("cuda", 1, 4, bg_shape=(7, 0, 3))
    run = schedule.RunSchedule("cuda", 1, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        run.column("w", lambda it: 1.0, into=torch.zeros(1))
    with pytest.raises(TypeError, match="into must be a tensor"):
        run.column("w", lambda it: 1.0, into=[0.0])
    with pytest.raises(TypeError, match="into must be torch.float32"):
        run.column("w", lambda it: 1.0, into=torch.zeros(1, dtype=torch.float64))
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=0.5)
    with pytest.raises(TypeError, match="update must be callable"):
        run.record_lrs(opt, None)
    for what in ("tick", "rebind", "status"):
        with pytest.raises(RuntimeError, match="before commit"):
            getattr(run, what)()
    with pytest.raises(RuntimeError, match="before commit"):
        run.seek(3)
    with pytest.raises(RuntimeError, match="before commit"):
        run.bg
    # an update() that fails leaves the rates as they were
    def bad(it):
        opt.param_groups[0]["lr"] = 0.25
        raise KeyError("boom")
    with pytest.raises(KeyError):
        run.record_lrs(opt, bad)
    assert opt.param_groups[0]["lr"] == 0.5 and run.names == []
    # FusedAdam: the mode belongs to the capturable optimizer
    eager = FusedAdam([torch.zeros(4, requires_grad=True)], lr=0.1)
    with pytest.raises(RuntimeError, match="capturable=True"):
        eager.lr_on_device(True)
    with pytest.raises(RuntimeError, match="capturable=True"):
        eager.lr_slots()
    cap = FusedAdam([torch.zeros(4, requires_grad=True)], lr=0.1, capturable=True)
    with pytest.raises(RuntimeError, match="eager step"):
        cap.lr_slots()
    assert cap.lr_on_device(True) is cap
    with pytest.raises(RuntimeError, match="RunSchedule"):
        cap.refresh_lr()
    cap.lr_on_device(False).refresh_lr()
    # the C ABI: every refusal is made before anything is launched
    lib = _lib.load()
    assert lib.gft_schedule_tick(None, None) != 0 and "NULL" in _lib.last_error()
    words = (C.c_int64 * 18)()
    base = (C.addressof(words) + 15) // 16 * 16

    def call(**over):
        s = _lib.Schedule()
        s.state, s.table, s.N, s.C, s.D, s.first_iter, s.dests, s.bg, s.n, s.T = base, base + 64, 1, 1, 0, 1, None, None, 0, 0
        for k, v in over.items():
            setattr(s, k, v)
        assert lib.gft_schedule_tick(None, C.byref(s)) != 0, over
        return _lib.last_error()

    assert "NULL state or table" in call(state=None) and "NULL state or table" in call(table=None)
    assert "8-byte aligned" in call(state=base + 4) and "8-byte aligned" in call(table=base + 68)
    assert "N=0 rows" in call(N=0) and "C=0 columns" in call(C=0) and "rows" in call(N=1 << 39, C=4)
    assert "D=1025 destinations" in call(D=1025) and "D=-1" in call(D=-1) and "NULL array" in call(D=3)
    assert "16-byte aligned" in call(D=1, dests=base + 72)
    assert "n=0 elements" in call(bg=base, n=0, T=256) and "T=0 threads" in call(bg=base, n=7, T=0)
    assert "4-byte aligned" in call(bg=base + 2, n=7, T=256) and "n=" in call(bg=base, n=(1 << 40) + 1, T=256)


# ---- GPU ------------------------------------------------------------------------------------------------------------------

def torch_background(it, shape, dev):
    """train.py:120-129, the generator's state kept"""
    rs, crs = torch.random.get_rng_state(), torch.cuda.get_rng_state(dev)
    torch.manual_seed(it)
    bg = torch.rand(*shape, dtype=torch.float32, device=dev) * 2 - 1
    torch.random.set_rng_state(rs)
    torch.cuda.set_rng_state(crs, dev)
    return bg


def fill_capacity(dev):
    p = torch.cuda.get_device_properties(dev)
    return 256 * p.multi_processor_count * (p.max_threads_per_multi_processor // 256)


ITS = (1, 7000, 2 ** 31 + 5, 2 ** 33 + 7)           # the last two reach bit 31 of the low key word and the high key word
BG_SHAPES = ("7x1x1", "7x13x17", "7x240x320", "second_draw")


@pytest.mark.gpu
@pytest.mark.parametrize("name", BG_SHAPES)
def test_background_is_torch_rand(gpu, name):
    from gftorf_amd import schedule
    if name == "second_draw":
        # the smallest n at which a thread of torch's grid-stride fill draws a second time (7 x 480 x 640 on a 256-CU part)
        shape = (fill_capacity(gpu) * 4 + 3,)
        assert (shape[0] - 1) // (4 * schedule.fill_threads(shape[0], gpu)) + 1 == 2
    else:
        shape = tuple(int(x) for x in name.split("x"))
    run = schedule.RunSchedule(gpu, 1, 8, bg_shape=shape).commit()
    assert run.bg.shape == shape and run.bg.dtype == torch.float32 and not run.bg.any()
    address = run.bg.data_ptr()
    n = run.bg.numel()
    for it in ITS:
        want = torch_background(it, shape, gpu)
        before = torch.cuda.get_rng_state(gpu), torch.random.get_rng_state()
        run.seek(it).tick()
        torch.cuda.synchronize()
        assert torch.equal(torch.cuda.get_rng_state(gpu), before[0]) and torch.equal(torch.random.get_rng_state(), before[1])
        differ = int((run.bg != want).sum())
        print("background", name, "it", it, "elements that differ from torch:", differ, "of", n)
        assert torch.equal(run.bg, want), (name, it, differ)
        assert int(run.iteration.item()) == it and run.status()[0] == it + 1 and run.bg.data_ptr() == address
    if n <= 7 * 13 * 17:
        host = schedule.background(7000, n, schedule.fill_threads(n, gpu))
        assert np.array_equal(host, torch_background(7000, shape, gpu).reshape(-1).cpu().numpy())
    assert float(run.bg.min()) >= -1.0 and float(run.bg.max()) < 1.0


FIRST, ROWS = 11, 6


def _value(it, column):
    return it * 100.0 + column + 0.5 + 1e-9 * (column + 1)              # (not a float32: the f32 kind has to round)


def _scatter_setup(gpu, bg_shape=(7, 13, 17)):
    """A FusedAdam of two groups (two and one parameters: f64 destinations, two of them for one column) and two float32
    tensors (three elements and one): D = 7"""
    from gftorf_amd import schedule, FusedAdam
    ps = [torch.zeros(n, device=gpu, requires_grad=True) for n in (8, 12, 4)]
    opt = FusedAdam([{"params": ps[:2], "lr": 0.5, "name": "a"}, {"params": ps[2:], "lr": 0.25, "name": "b"}], lr=0.0, capturable=True)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    opt.lr_on_device(True)
    weights = torch.full((5,), -1.0, device=gpu)
    single = torch.full((1,), -1.0, device=gpu)
    run = schedule.RunSchedule(gpu, FIRST, FIRST + ROWS - 1, bg_shape=bg_shape)

    def update(it):
        for k, g in enumerate(opt.param_groups):
            g["lr"] = _value(it, k)
    run.record_lrs(opt, update)
    run.column("w", lambda it: _value(it, 2), into=weights[1:4])
    run.column("s", lambda it: _value(it, 3), into=single)
    run.commit()
    assert run.D == 7 and [g["lr"] for g in opt.param_groups] == [0.5, 0.25]
    return run, opt, weights, single


def _slot_values(opt, gpu):
    b = opt._buffers(gpu)
    return [[float(b["lr"][(a - b["lr"].data_ptr()) // 8].item()) for a in group] for group in opt.lr_slots()]


def _check_row(it_row, opt, weights, single, gpu):
    assert _slot_values(opt, gpu) == [[_value(it_row, 0)] * 2, [_value(it_row, 1)]]
    w = weights.cpu().numpy()
    assert (w[[0, 4]] == -1).all() and (w[1:4] == np.float32(_value(it_row, 2))).all()
    assert single.cpu().numpy()[0] == np.float32(_value(it_row, 3)) and float(np.float32(_value(it_row, 3))) != _value(it_row, 3)


@pytest.mark.gpu
def test_row_scatter_counter_and_overrun(gpu):
    run, opt, weights, single = _scatter_setup(gpu)
    assert run.status() == (FIRST, False, 0) and int(run.iteration.item()) == FIRST - 1
    assert torch.equal(run.table.cpu(), torch.tensor([[_value(FIRST + r, c) for c in range(4)] for r in range(ROWS)], dtype=torch.float64))
    for r in range(ROWS):
        run.tick()
        _check_row(FIRST + r, opt, weights, single, gpu)
        assert int(run.iteration.item()) == FIRST + r and run.status() == (FIRST + r + 1, False, 0)
        assert torch.equal(run.bg, torch_background(FIRST + r, run.bg_shape, gpu))
    run.tick()                                                           # one past the end: the last row, and it is said
    _check_row(FIRST + ROWS - 1, opt, weights, single, gpu)
    assert int(run.iteration.item()) == FIRST + ROWS and run.status() == (FIRST + ROWS + 1, True, 1)
    assert torch.equal(run.bg, torch_background(FIRST + ROWS, run.bg_shape, gpu))         # the background follows the counter
    run.seek(FIRST - 3).tick()                                           # in front of the table: the first row
    _check_row(FIRST, opt, weights, single, gpu)
    assert int(run.iteration.item()) == FIRST - 3 and run.status() == (FIRST - 2, True, 2)
    run.seek(FIRST + 2).tick()                                           # back inside: the flag and the count stay
    _check_row(FIRST + 2, opt, weights, single, gpu)
    assert run.status() == (FIRST + 3, True, 2)
    with pytest.raises(RuntimeError, match="after commit"):
        run.column("late", lambda it: 0.0, into=single)


def _capture(region, after_warm_up=None):
    """The recipe of tests/test_gpu_graph.py: warm-up on a side stream, then one capture"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        region()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if after_warm_up is not None:
        after_warm_up()
        torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = region()
    return graph, static


@pytest.mark.gpu
def test_captured_tick_follows_the_counter(gpu):
    run, opt, weights, single = _scatter_setup(gpu)
    n_log = 5
    log_bg = torch.zeros((n_log,) + run.bg_shape, device=gpu)
    log_it = torch.zeros((n_log,), device=gpu, dtype=torch.int64)
    log_w = torch.zeros((n_log, 3), device=gpu)
    log_lr = torch.zeros((n_log,), device=gpu, dtype=torch.float64)
    b = opt._buffers(gpu)
    slot = b["lr"][(opt.lr_slots()[1][0] - b["lr"].data_ptr()) // 8:][:1]           # group b's rate, as the step reads it

    def region():
        run.tick()
        row = run.iteration - FIRST                                      # the log's row, chosen on the device
        log_bg.index_copy_(0, row, run.bg.unsqueeze(0))
        log_it.index_copy_(0, row, run.iteration)
        log_w.index_copy_(0, row, weights[1:4].unsqueeze(0))
        log_lr.index_copy_(0, row, slot)

    graph, _ = _capture(region, after_warm_up=lambda: run.seek(FIRST))
    assert run.status()[0] == FIRST                                      # the capture ran nothing
    for t in (log_bg, log_it, log_w, log_lr):
        t.copy_(torch.zeros_like(t))
    for _ in range(n_log):
        graph.replay()                                                   # no host statement in between
    torch.cuda.synchronize()
    assert log_it.tolist() == list(range(FIRST, FIRST + n_log)) and run.status() == (FIRST + n_log, False, 0)
    for r in range(n_log):
        assert torch.equal(log_bg[r], torch_background(FIRST + r, run.bg_shape, gpu)), r
        assert (log_w[r].cpu().numpy() == np.float32(_value(FIRST + r, 2))).all() and float(log_lr[r]) == _value(FIRST + r, 1)
    assert not torch.equal(log_bg[0], log_bg[1])


@pytest.mark.gpu
def test_no_host_sync(gpu):
    run, opt, weights, single = _scatter_setup(gpu)
    graph, _ = _capture(run.tick, after_warm_up=lambda: run.seek(FIRST))
    run.tick()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run.tick()
        graph.replay()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert run.status() == (FIRST + 3, False, 0)
    _check_row(FIRST + 2, opt, weights, single, gpu)


# ---- FusedAdam ------------------------------------------------------------------------------------------------------------

ADAM_FIRST = 3


def _adam_lrs(it):
    """group a: a decaying rate; group b: zero until a window opens at iteration 6 (as the offsets' rates do)"""
    return 1e-2 * float(np.exp(-0.37 * it)) + 1e-4, (2e-3 if it > 5 else 0.0)


class _AdamSide:
    """Three parameters in two groups with fixed gradients, a capturable FusedAdam that has taken its first eager step"""

    def __init__(self, gpu, on_device):
        from gftorf_amd import FusedAdam
        gen = torch.Generator().manual_seed(20261020)
        self.gpu = gpu
        self.p = [torch.nn.Parameter(torch.randn(s, generator=gen).to(gpu)) for s in ((5, 3), (7,), (4, 2))]
        self.g = [torch.randn(s, generator=gen).to(gpu) for s in ((5, 3), (7,), (4, 2))]
        self.grad_of = {id(p): g for p, g in zip(self.p, self.g)}
        self.opt = FusedAdam([{"params": self.p[:2], "lr": 1e-3, "name": "a"}, {"params": self.p[2:], "lr": 0.0, "name": "b"}], lr=0.0,
                             eps=1e-15, capturable=True)
        self.set_grads()
        self.opt.step()
        self.opt.lr_on_device(True)
        if not on_device:
            self.opt.lr_on_device(False)                                 # off again: the route through pinned memory, as before

    def set_grads(self):
        for g in self.opt.param_groups:
            for p in g["params"]:
                p.grad = self.grad_of[id(p)]

    def update(self, it):
        for g, lr in zip(self.opt.param_groups, _adam_lrs(it)):
            g["lr"] = lr

    def tensors(self):
        out = []
        for g in self.opt.param_groups:
            for p in g["params"]:
                st = self.opt.state[p]
                out += [p.data, st["exp_avg"], st["exp_avg_sq"], st["step"]]
        return out

    def snapshot(self):
        return [t.clone() for t in self.tensors()]

    def restore(self, snap):
        with torch.no_grad():
            for t, s in zip(self.tensors(), snap):
                t.copy_(s)

    def extend_first(self):
        """The first parameter gains two rows the way cat_tensors_to_optimizer does (scene/gaussian_model.py:497-518): the
        state dict is kept and handed to the new nn.Parameter"""
        group = self.opt.param_groups[0]
        old = group["params"][0]
        extension = torch.full((2, 3), 0.125, device=self.gpu)
        stored_state = self.opt.state.get(old, None)
        stored_state["exp_avg"] = torch.cat((stored_state["exp_avg"], torch.zeros_like(extension)), dim=0)
        stored_state["exp_avg_sq"] = torch.cat((stored_state["exp_avg_sq"], torch.zeros_like(extension)), dim=0)
        del self.opt.state[old]
        group["params"][0] = torch.nn.Parameter(torch.cat((old.data, extension), dim=0).requires_grad_(True))
        self.opt.state[group["params"][0]] = stored_state
        self.grad_of[id(group["params"][0])] = torch.cat((self.grad_of.pop(id(old)), torch.full((2, 3), -0.75, device=self.gpu)), dim=0)
        self.set_grads()


def _equal_sides(a, b, what):
    for k, (x, y) in enumerate(zip(a.tensors(), b.tensors())):
        assert x.shape == y.shape and torch.equal(x, y), (what, k)


@pytest.mark.gpu
def test_adam_reads_the_ticked_rates(gpu):
    from gftorf_amd import schedule
    A, B = _AdamSide(gpu, True), _AdamSide(gpu, False)
    _equal_sides(A, B, "after the eager step")
    with pytest.raises(RuntimeError, match="RunSchedule"):
        A.opt.refresh_lr()
    run = schedule.RunSchedule(gpu, ADAM_FIRST, ADAM_FIRST + 19)
    kept = [g["lr"] for g in A.opt.param_groups]
    run.record_lrs(A.opt, A.update)
    assert [g["lr"] for g in A.opt.param_groups] == kept
    run.commit()
    assert run.bg is None and run.D == 3
    slots = A.opt.lr_slots()
    assert [len(s) for s in slots] == [2, 1] and len({a for s in slots for a in s}) == 3

    def region():
        run.tick()
        A.opt.step()

    def rounds(first_it, what):
        start = A.snapshot()
        graph, _ = _capture(region, after_warm_up=lambda: (A.restore(start), run.seek(first_it)))
        for _ in range(6):
            graph.replay()                                               # back to back
        for it in range(first_it, first_it + 6):                         # the existing route, eagerly
            B.update(it)
            B.opt.refresh_lr()
            B.opt.step()
            # (the step's copy of the rates reads the pinned buffer when the device reaches it, not when it was queued: the
            # host must not write the next iteration's rates before -- the hazard a ticked schedule does not have)
            torch.cuda.synchronize()
        _equal_sides(A, B, what)
        assert run.status() == (first_it + 6, False, 0)
        assert float(A.opt.state[A.opt.param_groups[0]["params"][0]]["step"]) == 1 + (first_it - ADAM_FIRST) + 6

    rounds(ADAM_FIRST, "six replays")                                    # the window of group b opens inside these
    assert not torch.equal(A.p[2].data, _AdamSide(gpu, False).p[2].data)                # ... and its parameter has moved
    # a densification re-keys a parameter; the state dict, hence the slot, is kept
    A.extend_first()
    B.extend_first()
    assert A.opt.lr_slots() == slots
    address = run._dests.data_ptr()
    run.rebind()
    assert run._dests.data_ptr() == address and run.D == 3
    rounds(ADAM_FIRST + 6, "six replays after the re-keyed parameter")
    assert A.opt.param_groups[0]["params"][0].shape == (7, 3)
    # the host's rates are not read in the mode: whatever param_groups say, a step takes the ticked row
    for g in A.opt.param_groups:
        g["lr"] = 123.0
    run.seek(ADAM_FIRST + 12).tick()
    A.opt.step()
    B.update(ADAM_FIRST + 12)
    B.opt.refresh_lr()
    B.opt.step()
    _equal_sides(A, B, "an eager tick and step")


# ---- composition ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_captured_iteration_with_the_rasterizer(gpu):
    """{tick; rasterizer(bg=run.bg); loss; backward; step} in one graph, replayed three times back to back"""
    import helpers as Hh
    from gftorf_amd import api, schedule, synth, FusedAdam, GaussianRasterizer
    P, W, H = 300, 32, 24
    first = 41
    sc = Hh.small_scene(P=P, W=W, H=H, seed=47, w2c=synth.look_at_w2c(0.05, -0.02, 0.0, (0.05, 0.0, 0.1)))
    names = ("means3D", "opacities", "shs", "shs_p", "scales", "rotations")
    start = {k: torch.tensor(sc["gaussians"][k], dtype=torch.float32, device=gpu) for k in names}
    rates = dict(means3D=2e-4, opacities=5e-3, shs=2.5e-3, shs_p=2.5e-3, scales=1e-3, rotations=1e-3)

    def lr_of(name, it):
        return rates[name] * (0.5 if name == "means3D" and it >= first + 2 else 1.0) * (1.0 + 0.01 * (it - first))

    class Side:
        def __init__(self):
            self.par = {k: torch.nn.Parameter(v.clone()) for k, v in start.items()}
            self.opt = FusedAdam([{"params": [self.par[k]], "lr": rates[k], "name": k} for k in names], lr=0.0, eps=1e-15, capturable=True)
            self.m2 = torch.zeros((P, 3), device=gpu, requires_grad=True)
            self.log = torch.zeros((3, 2, 3, H, W), device=gpu)

        def update(self, it):
            for g in self.opt.param_groups:
                g["lr"] = lr_of(g["name"], it)

        def forward(self, settings):
            p = self.par
            return GaussianRasterizer(raster_settings=settings)(
                means3D=p["means3D"], means2D=self.m2, opacities=p["opacities"], shs=p["shs"], shs_p=p["shs_p"], scales=p["scales"],
                rotations=p["rotations"], phase_offset=0.1, dc_offset=0.05)

        def iteration(self, settings, row=None):
            self.m2.grad = None
            out = self.forward(settings)
            if row is not None:
                self.log.index_copy_(0, row, torch.stack((out[0][:3], out[1][:3])).detach().unsqueeze(0))
            loss = (out[0] ** 2).mean() + (out[1][:3] ** 2).mean()
            loss.backward()
            self.opt.step()
            self.opt.zero_grad(set_to_none=True)

        def values(self):
            return {k: v.detach().clone() for k, v in self.par.items()}

        def restore(self, values):
            with torch.no_grad():
                for k, v in values.items():
                    self.par[k].copy_(v)
                for p in self.par.values():
                    st = self.opt.state[p]
                    st["exp_avg"].copy_(torch.zeros_like(p))
                    st["exp_avg_sq"].copy_(torch.zeros_like(p))
                    st["step"].copy_(torch.zeros_like(st["step"]))

    def eager_settings(it):
        return Hh.gpu_settings(sc, gpu, bg=torch_background(it, (7, H, W), gpu))

    api._instance_hint.clear()
    try:
        A, B = Side(), Side()
        for s in (A, B):                                                 # the eager iterations in front of a capture (section K)
            for _ in range(2):
                s.iteration(eager_settings(first))
        A.opt.lr_on_device(True)
        run = schedule.RunSchedule(gpu, first, first + 9, bg_shape=(7, H, W))
        run.record_lrs(A.opt, A.update)
        run.commit()

        static_settings = Hh.gpu_settings(sc, gpu, bg=run.bg)             # built once: its tensors are copied from the host

        def region():
            run.tick()
            A.iteration(static_settings, row=run.iteration - first)

        graph, _ = _capture(region, after_warm_up=lambda: (A.restore(start), run.seek(first)))
        B.restore(start)
        torch.cuda.synchronize()
        with torch.no_grad():                                            # replay 1's forward, eagerly: same parameters, torch's background
            want = B.forward(eager_settings(first))
            want = torch.stack((want[0][:3], want[1][:3])).clone()
        for _ in range(3):
            graph.replay()                                               # back to back
        for it in range(first, first + 3):                               # the eager loop: the statements the tick replaces
            B.update(it)
            B.opt.refresh_lr()
            B.iteration(eager_settings(it))
            torch.cuda.synchronize()                                     # (the pinned rates are read when the device reaches the copy)
        assert run.status() == (first + 3, False, 0)
        assert torch.equal(A.log[0], want)                               # bit for bit
        assert not torch.equal(A.log[0], A.log[1]) and not torch.equal(A.log[1], A.log[2])
        report = {}
        for k in names:
            ref, got = B.par[k].detach(), A.par[k].detach()
            moved = float((ref - start[k]).abs().max())
            err = (got - ref).abs()
            if moved == 0.0:
                assert float(err.max()) == 0.0, k
                continue
            # the bound of tests/test_loop_graph.py for graph against eager: the mean error and the share of elements that
            # differ visibly, in units of the largest move (the backward's float atomics have no fixed order)
            report[k] = (float(err.mean()) / moved, float((err > 0.05 * moved).float().mean()), float(err.max()) / moved)
            print("composition", k, "mean error / move %.3g, share above 5 %% %.3g, worst / move %.3g" % report[k])
        for k, r in report.items():
            assert r[0] <= 5e-3 and r[1] <= 2e-2, (k, r)
        assert set(report) >= {"means3D", "opacities", "scales"}
        st = [x for x in api.enqueue_status() if x["key"][1:4] == (P, W, H)]
        assert st and all(not x["overflow"] for x in st)
    finally:
        api._instance_hint.clear()
