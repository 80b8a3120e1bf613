"""The run's schedule on the device (``csrc/k_schedule.hip``, ``include/gftorf_schedule.h``): the statement in front of an
iteration, "make iteration ``it`` current", as one launch that a captured graph can hold.

The reference seeds the global generator with the iteration and draws the background (``train.py:120-129``), then walks both
optimizers' groups to set their learning rates (``train.py:146-147``, ``scene/gaussian_model.py:294-313``,
``scene/deform_model.py:42-47``).  Neither can be captured: ``torch.manual_seed`` is host state, a captured ``uniform_`` takes
its seed from the generator and not from the iteration, and the rates reach a captured ``FusedAdam`` step through pinned
memory the host rewrites first.  Here all of it is a function of a device counter that the launch itself advances, as
``views.ViewStore.draw()`` does for the view:

``RunSchedule(device, first_iter, iterations, bg_shape=)``  the table of the run: one float64 row per iteration
    ``first_iter .. iterations``.  ``record_lrs(optimizer, update)`` fills one column per parameter group by calling the
    caller's own ``update(it)`` for every iteration, on the host, once -- the table is the reference's statements
    themselves, nothing is re-derived on the device --, ``column(name, fn, into=)`` one column of ``fn(it)`` bound to a
    float32 device tensor, ``commit()`` uploads it.  ``tick()`` is the launch: the background of the iteration into ``bg``
    (``torch.manual_seed(it); torch.rand(bg_shape, device=...) * 2 - 1`` bit for bit, the torch generator untouched), the
    iteration's row to its destinations, the iteration into ``iteration``, and the counter one further.
``philox4x32_10(counter, key)``, ``background(it, n, T)``  the generator and the fill restated in pure Python and numpy.

Not covered: the gating of the steps (``train.py:469-472``), the SH-degree schedule and the ``tof_iters`` switch of
``lambda_color`` change which kernels run, not a number they read; they stay one captured graph per phase.

There is no CPU path for ``commit()`` and ``tick()``; recording the table and the restatements run anywhere.
"""
import ctypes as C

import numpy as np
import torch

from . import _args, _lib

_TAG = "gftorf_amd.schedule"
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): the four 32-bit
    words of the block ``counter`` (four words) under ``key`` (two words)"""
    c0, c1, c2, c3 = (int(x) & _MASK for x in counter)
    k0, k1 = (int(x) & _MASK for x in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def fill_threads(n, device=None, properties=None):
    """T of ``gft_schedule_tick``: the threads of torch's own fill of ``n`` elements (``calc_execution_policy`` of
    ATen/native/cuda/DistributionTemplates.h: blocks of 256, as many as fit the device at once and no more than cover n)"""
    p = torch.cuda.get_device_properties(device) if properties is None else properties
    return 256 * min(int(p.multi_processor_count) * (int(p.max_threads_per_multi_processor) // 256), (int(n) + 255) // 256)


def background(it, n, T):
    """The tick's background restated on the host: float32 ``[n]``.  Slow (a Python loop per block): for tests and small n."""
    out = np.empty((n,), np.float32)
    key = (it & _MASK, (it >> 32) & _MASK)
    scale = np.float32(2.0 ** -32)
    for j in range((n - 1) // (4 * T) + 1):
        for idx in range(min(T, n - 4 * j * T)):
            words = philox4x32_10((j & _MASK, j >> 32, idx & _MASK, idx >> 32), key)
            for k in range(4):
                e = idx + T * (4 * j + k)
                if e < n:
                    u = scale + np.float32(words[k]) * scale
                    out[e] = (np.float32(0.0) if u == np.float32(1.0) else u) * np.float32(2.0) - np.float32(1.0)
    return out


class RunSchedule:
    """The per-iteration numbers of a run, on the device.

    ``first_iter``, ``iterations``: the run is ``range(first_iter, iterations + 1)`` (``train.py:118``).  ``bg_shape``: the
    shape of the random background (``(7, H, W)``), or None for a run without one (``dataset.random_bg_color`` off).  Record
    the columns, ``commit()``, then ``tick()`` once per iteration -- eagerly or as the first node of a captured graph.
    ``bg`` and ``iteration`` (int64 ``[1]``) keep their addresses for the life of the object."""

    def __init__(self, device, first_iter, iterations, bg_shape=None):
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError("%s: a RunSchedule lives on a HIP device, got %s; there is no CPU path" % (_TAG, device))
        self._device_arg = device
        self.device = None                      # with its index, from commit() on
        self.first_iter, self.iterations = int(first_iter), int(iterations)
        if self.iterations < self.first_iter:
            raise ValueError("%s: iterations=%d lies before first_iter=%d" % (_TAG, self.iterations, self.first_iter))
        self.N = self.iterations - self.first_iter + 1
        if bg_shape is not None:
            bg_shape = tuple(int(s) for s in bg_shape)
            if not bg_shape or min(bg_shape) < 1:
                raise ValueError("%s: bg_shape must be a non-empty shape of positive sizes, got %s" % (_TAG, list(bg_shape)))
        self.bg_shape = bg_shape
        self.names = []                         # one per column
        self._columns = []                      # float64 [N] each
        self._bindings = []                     # ("lrs", optimizer, first column, groups) | ("f32", tensor, column)
        self._committed = False

    # ---- recording ----------------------------------------------------------------------------------------------------------

    def _open(self, what):
        if self._committed:
            raise RuntimeError("%s: %s after commit(); the table of a RunSchedule is fixed once uploaded" % (_TAG, what))

    def _name(self, name):
        if name in self.names:
            raise ValueError("%s: a column named %r exists already" % (_TAG, name))
        self.names.append(name)

    def record_lrs(self, optimizer, update):
        """One column per group of ``optimizer.param_groups``: ``update(it)`` is called for every iteration of the run, in
        order, and ``[g["lr"] for g in param_groups]`` is recorded after each call, in float64; the groups' rates are put
        back afterwards.  ``update`` is the caller's own statement (``lambda it: gaussians.update_learning_rate(it, opt)``),
        state it keeps between calls included.  Returns the ``[N, groups]`` array.  A ``tick()`` writes the row into every
        ``lr_slots()`` of the group, so by ``commit()`` the optimizer is a ``FusedAdam(capturable=True)`` that has taken a
        step and is in the ``lr_on_device(True)`` mode."""
        self._open("record_lrs()")
        groups = optimizer.param_groups
        if not groups:
            raise ValueError("%s: record_lrs(): the optimizer has no parameter groups" % _TAG)
        if not callable(update):
            raise TypeError("%s: record_lrs(): update must be callable with the iteration, got %s" % (_TAG, type(update).__name__))
        kept = [g["lr"] for g in groups]
        rows = np.empty((self.N, len(groups)), np.float64)
        try:
            for r in range(self.N):
                update(self.first_iter + r)
                if len(optimizer.param_groups) != len(kept):
                    raise RuntimeError("%s: record_lrs(): update() changed the number of parameter groups" % _TAG)
                rows[r] = [float(g["lr"]) for g in optimizer.param_groups]
        finally:
            for g, lr in zip(groups, kept):
                g["lr"] = lr
        at = len(self._columns)
        for k, g in enumerate(groups):
            self._name("lr:%d:%s" % (sum(1 for b in self._bindings if b[0] == "lrs"), g.get("name", k)))
            self._columns.append(rows[:, k].copy())
        self._bindings.append(("lrs", optimizer, at, len(groups)))
        return rows

    def column(self, name, fn, into):
        """One column of ``float(fn(it))``, bound to ``into``: a float32 device tensor (contiguous; ``weights[1:2]`` serves)
        whose every element a ``tick()`` sets to the iteration's value, rounded once from the double.  Returns the ``[N]``
        array."""
        self._open("column()")
        into_d = _args.tensor(_TAG, into, "into")
        if into_d.numel() < 1 or not into_d.is_contiguous():
            raise RuntimeError("%s: into must be a contiguous tensor with at least one element, got %s" % (_TAG, list(into_d.shape)))
        _args.devices(_TAG, "schedule", [(into_d, "into")])
        if not callable(fn):
            raise TypeError("%s: column(): fn must be callable with the iteration, got %s" % (_TAG, type(fn).__name__))
        values = np.array([float(fn(self.first_iter + r)) for r in range(self.N)], np.float64)
        self._name(str(name))
        self._columns.append(values)
        self._bindings.append(("f32", into_d, len(self._columns) - 1))
        return values

    # ---- the device side ------------------------------------------------------------------------------------------------------

    def _destinations(self):
        """(address, column, kind) of every destination, in the order of the bindings"""
        out = []
        for b in self._bindings:
            if b[0] == "lrs":
                _kind, optimizer, at, count = b
                if not hasattr(optimizer, "lr_slots"):
                    raise TypeError("%s: the learning rates are written into the device slots of a "
                                    "gftorf_amd.FusedAdam(capturable=True); got %s" % (_TAG, type(optimizer).__name__))
                slots = optimizer.lr_slots()
                if len(slots) != count:
                    raise RuntimeError("%s: the optimizer has %d parameter groups, %d were recorded" % (_TAG, len(slots), count))
                if not optimizer._gft_lr_on_device:
                    raise RuntimeError("%s: the optimizer still copies its rates from the host in every step(), over what a "
                                       "tick() writes; call optimizer.lr_on_device(True)" % _TAG)
                for k, group in enumerate(slots):
                    out += [(address, at + k, 0) for address in group]
            else:
                _kind, t, col = b
                if t.device != self.device:
                    raise RuntimeError("%s: into of column %r is on %s, the schedule on %s" % (_TAG, self.names[col], t.device, self.device))
                out += [(t.data_ptr() + 4 * i, col, 1) for i in range(t.numel())]
        if len(out) > _lib.SCHEDULE_MAX_DESTS:
            raise ValueError("%s: %d destinations; a tick takes at most %d" % (_TAG, len(out), _lib.SCHEDULE_MAX_DESTS))
        return out

    def _dest_bytes(self, dests):
        arr = (_lib.ScheduleDest * max(len(dests), 1))()
        for e, (address, column, kind) in zip(arr, dests):
            e.address, e.column, e.kind = address, column, kind
        return torch.from_numpy(np.frombuffer(arr, np.uint8, 16 * max(len(dests), 1)).copy())

    def commit(self):
        """Uploads the table and binds the destinations; the counter stands at ``first_iter``.  Once."""
        self._open("commit()")
        self.device = dev = _args.indexed_device(_TAG, "a RunSchedule", self._device_arg)
        dests = self._destinations()
        table = np.stack(self._columns, axis=1) if self._columns else np.zeros((self.N, 1), np.float64)
        with _lib.on_device(dev):
            self._table = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
            self._dests = self._dest_bytes(dests).to(dev)
            state = np.zeros((_lib.SCHEDULE_STATE_WORDS,), np.int64)
            state[_lib.SCHEDULE_COUNTER] = self.first_iter
            state[_lib.SCHEDULE_ITERATION] = self.first_iter - 1
            self._state = torch.from_numpy(state).to(dev)
            self._bg = None if self.bg_shape is None else torch.from_numpy(np.zeros(self.bg_shape, np.float32)).to(dev)
        self.D = len(dests)
        n = 0 if self._bg is None else self._bg.numel()
        s = self._struct = _lib.Schedule()
        s.state, s.table, s.N, s.C, s.D, s.first_iter = self._state.data_ptr(), self._table.data_ptr(), self.N, table.shape[1], self.D, self.first_iter
        s.dests, s.bg, s.n, s.T = self._dests.data_ptr(), _args.ptr(self._bg), n, fill_threads(n, dev) if n else 0
        self._ref = C.byref(s)
        self._tick = _lib.load().gft_schedule_tick
        self._committed = True
        return self

    def _live(self, what):
        if not self._committed:
            raise RuntimeError("%s: %s before commit()" % (_TAG, what))

    def tick(self):
        """Makes the counter's iteration current and moves the counter on: one launch on the current stream, nothing read on
        the host.  Can be captured; ticks of one schedule belong on one stream."""
        self._live("tick()")
        dev = self.device
        with _lib.on_device(dev):
            _lib.check(self._tick(_lib.raw_stream(dev), self._ref))
        return self

    def rebind(self):
        """After a densification: the optimizers' parameters were re-keyed and their state dicts kept, so the slots are the
        same ones -- but this rewrites the destination array from the optimizers and tensors as they are now, in place, at
        the same address; the number of destinations must not change.  Forces no new capture by itself."""
        self._live("rebind()")
        dests = self._destinations()
        if len(dests) != self.D:
            raise RuntimeError("%s: rebind(): %d destinations, %d at commit(); a schedule of another size is a new RunSchedule" % (_TAG, len(dests), self.D))
        with _lib.on_device(self.device):
            self._dests.copy_(self._dest_bytes(dests))
        return self

    def seek(self, it):
        """Sets the counter: the next ``tick()`` makes iteration ``it`` current.  A copy, never a memset."""
        self._live("seek()")
        with _lib.on_device(self.device):
            self._state[_lib.SCHEDULE_COUNTER:_lib.SCHEDULE_COUNTER + 1].copy_(torch.from_numpy(np.array([int(it)], np.int64)))
        return self

    def status(self):
        """``(next iteration, overrun flag, overrun count)``: the one blocking read.  The flag is set, and the count goes up,
        whenever a tick finds the counter outside ``first_iter .. iterations`` (it then draws the nearest row); nothing here
        clears them."""
        self._live("status()")
        s = self._state.cpu()
        return int(s[_lib.SCHEDULE_COUNTER]), bool(s[_lib.SCHEDULE_OVERRUN]), int(s[_lib.SCHEDULE_OVERRUNS])

    @property
    def bg(self):
        """float32 ``bg_shape``: the background of the iteration made current last (None without ``bg_shape``)"""
        self._live("bg")
        return self._bg

    @property
    def iteration(self):
        """int64 ``[1]``: the iteration made current last (``first_iter - 1`` before the first tick)"""
        self._live("iteration")
        return self._state[_lib.SCHEDULE_ITERATION:_lib.SCHEDULE_ITERATION + 1]

    @property
    def table(self):
        """float64 ``[N, C]`` on the device: row ``it - first_iter``, columns in the order of ``names``"""
        self._live("table")
        return self._table
