"""Fused Adam for the Gaussian parameters (optimizer part).

``FusedAdam`` is a ``torch.optim.Adam`` whose ``step()`` runs one hand-written gfx950 kernel per
call -- all tensors of all groups that share betas / eps / weight decay in one launch, each with its own learning
rate and step count (``csrc/k_adam.hip``, ``include/gftorf_optim.h``) --
instead of torch's multi-tensor path (one kernel per arithmetic operation); constructor, ``param_groups``, ``state`` (``step`` / ``exp_avg`` / ``exp_avg_sq``),
``state_dict`` and ``zero_grad`` are torch's own, so the reference's densification code, which
edits the optimizer state in place (``scene/gaussian_model.py:456-540``), works unchanged.
Use: replace ``torch.optim.Adam(l, lr=0.0, eps=1e-15)`` at ``scene/gaussian_model.py:274`` by
``gftorf_amd.FusedAdam(l, lr=0.0, eps=1e-15)``.

Opt-in, not the reference's behaviour: ``step(visibility=mask)`` ("sparse Adam on visible
Gaussians") updates only the rows ``mask`` selects in every parameter whose first dimension is ``mask.numel()`` -- with
``visibility_filter`` of the iteration's render (``train.py:181``) that is the 10-20 % of the Gaussians that received a
gradient at all.  The other rows keep parameter AND moments (a dense Adam lets their moments decay and still moves
them by the decaying first moment); parameters of other shapes (the deformation network) take the dense step.

``FusedAdam(..., capturable=True)``: the step inside a captured iteration (``torch.cuda.graph``).  Nothing the update
depends on is baked into the launch: ``state["step"]`` is a 0-dim fp32 DEVICE tensor (as torch's capturable Adam keeps it),
the learning rates are read on the device from a small buffer that every ``step()`` refreshes from ``param_groups`` through
pinned host memory -- a copy node when captured, so a replay sees whatever ``refresh_lr()`` (or any eager bookkeeping
that ends in it: the reference's ``update_learning_rate``, scene/gaussian_model.py:294-310, then ``refresh_lr()``) wrote
there since.  ``lr_on_device(True)`` drops that copy: the device buffer is then written by ``schedule.RunSchedule.tick()``,
itself a node of the graph, and ``lr_slots()`` names its destinations.  Bias corrections are formed in double precision on the device: N replays leave the parameters N eager
non-capturable steps would (to the rounding of one double ``pow``).  ``step(visibility=mask)`` works in this mode too: the
mask is read when the kernel runs, so a replay follows the mask's contents of that replay.

Gradient-norm clipping (``train.py:468``: ``torch.nn.utils.clip_grad_norm_(deform.parameters(), max_norm=1.0)``) has two
forms.  ``clip_grad_norm_`` is the drop-in: one norm launch per 40 tensors, a one-workgroup sum, one scaling launch per 40
tensors, no host read, so it can be captured.  ``FusedAdam.step(max_grad_norm=1.0)`` folds the scaling into the update: the
norm over every gradient of this optimizer is left on the device with torch's coefficient ``min(1, max_norm / (norm + 1e-6))``,
and every Adam launch multiplies the gradients by it as it reads them -- the update is the one ``clip_grad_norm_`` followed by
``step()`` gives, bit for bit, but ``.grad`` is NOT written (the reference drops the gradients two lines later,
``train.py:473-474``).  ``optimizer.last_grad_norm`` is the norm, a 0-dim device tensor.  Eager, capturable and
``visibility`` steps all take it.  Under data parallelism the clip comes after ``allreduce_gradients``.
"""
import ctypes as C

import torch

from . import _lib

_NORM_SCRATCH = {}          # (device index, stream) -> the norm's partial sums (bytes), kept from call to call


def _span_tables(grads):
    n = len(grads)
    return (C.c_void_p * n)(*[g.data_ptr() for g in grads]), (C.c_int64 * n)(*[g.numel() for g in grads])


def _grad_norm(lib, dev, grads, max_norm, ptrs=None, ns=None):
    """(norm, coefficient) of gft_grad_norm over ``grads`` (contiguous fp32 tensors on ``dev``) as a fresh 2-element device
    tensor.  The partial sums go through a buffer kept per device and stream -- except while a graph is captured: a buffer
    baked into a graph comes from the graph's pool (a kept one may be replaced by a larger one, which would free it under
    the graph), the rule of ``api.py``."""
    if ptrs is None:
        ptrs, ns = _span_tables(grads)
    n = len(grads)
    need = lib.gft_grad_norm_scratch_bytes(sum(ns), n)
    stream = _lib.raw_stream(dev)
    if torch.cuda.is_current_stream_capturing():
        scratch = torch.empty((need,), device=dev, dtype=torch.uint8)
    else:
        key = (dev.index, stream)
        scratch = _NORM_SCRATCH.get(key)
        if scratch is None or scratch.numel() < need:
            if len(_NORM_SCRATCH) > 16:
                _NORM_SCRATCH.clear()
            scratch = _NORM_SCRATCH[key] = torch.empty((max(need, 4096),), device=dev, dtype=torch.uint8)
    out = torch.empty((2,), device=dev, dtype=torch.float32)
    with _lib.on_device(dev):
        _lib.check(lib.gft_grad_norm(stream, n, ptrs, ns, float(max_norm), scratch.data_ptr(), scratch.numel(), out.data_ptr()))
    return out


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` for fp32 gradients on a HIP device, L2 norm (``train.py:468``): the gradients are
    scaled in place by ``min(1, max_norm / (norm + 1e-6))``; returns the norm, a 0-dim fp32 device tensor.  Nothing is read
    on the host and nothing is cleared: the call can be captured in a graph (``error_if_nonfinite=True`` reads the norm, so
    it cannot).  ``foreach`` is accepted and ignored."""
    if float(norm_type) != 2.0:
        raise NotImplementedError("gftorf_amd.clip_grad_norm_: norm_type=%r is not supported (the L2 norm only)" % (norm_type,))
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    dev = grads[0].device
    for g in grads:
        if g.device.type != "cuda":
            raise RuntimeError("gftorf_amd.clip_grad_norm_ runs on a HIP device only (gradient on %s); there is no CPU path" % (g.device,))
        if g.device != dev:
            raise RuntimeError("gftorf_amd.clip_grad_norm_: gradients on %s and %s (one device per call)" % (dev, g.device))
        if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous():
            raise RuntimeError("gftorf_amd.clip_grad_norm_: gradients must be dense contiguous float32 tensors")
    if error_if_nonfinite and torch.cuda.is_current_stream_capturing():
        raise NotImplementedError("gftorf_amd.clip_grad_norm_: error_if_nonfinite=True reads the norm on the host, which a "
                                  "captured call cannot")
    lib = _lib.load()
    ptrs, ns = _span_tables(grads)
    out = _grad_norm(lib, dev, grads, max_norm, ptrs, ns)
    if error_if_nonfinite and not bool(torch.isfinite(out[0])):
        raise RuntimeError("The total norm of order %s for gradients from `parameters` is non-finite, so it cannot be clipped. "
                           "To disable this error and scale the gradients by the non-finite norm anyway, set "
                           "`error_if_nonfinite=False`" % (float(norm_type),))
    with _lib.on_device(dev):
        _lib.check(lib.gft_grad_scale(_lib.raw_stream(dev), len(grads), ptrs, ns, out.data_ptr() + 4))
    return out[0]


class FusedAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **kw):
        if amsgrad or kw.get("maximize") or kw.get("differentiable"):
            raise NotImplementedError("gftorf_amd.FusedAdam: amsgrad / maximize / differentiable are not supported")
        kw.pop("foreach", None)
        kw.pop("fused", None)
        self._gft_capturable = bool(kw.pop("capturable", False))
        self._gft_dev = {}              # device -> dict(step, lr, lr_host, factors, used): the buffers of the capturable mode
        self._gft_lr_on_device = False  # lr_on_device(True): the device slots of the rates belong to a schedule.RunSchedule
        self.last_grad_norm = None      # step(max_grad_norm=...): the gradients' global L2 norm, a 0-dim device tensor
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, **kw)

    # ---- capturable mode ------------------------------------------------------------------------------------------
    _SLOTS = 512

    def _buffers(self, dev):
        b = self._gft_dev.get(dev)
        if b is None:
            b = self._gft_dev[dev] = dict(
                step=torch.zeros((self._SLOTS,), device=dev, dtype=torch.float32),
                lr=torch.zeros((self._SLOTS,), device=dev, dtype=torch.float64),
                lr_host=torch.zeros((self._SLOTS,), dtype=torch.float64).pin_memory(),
                factors=torch.zeros((2 * self._SLOTS,), device=dev, dtype=torch.float32), used=0)
            b["lr_np"] = b["lr_host"].numpy()
        return b

    def _slot_of(self, b, st):
        """The slot whose count ``st`` (a ``state["step"]``) views, or None.  The state itself is the record: the reference's
        densification code replaces a parameter and hands the SAME state dict to the new tensor
        (scene/gaussian_model.py:456-540), so nothing keyed by the parameter object survives it."""
        base = b["step"].data_ptr()
        if (isinstance(st, torch.Tensor) and st.device == b["step"].device and st.dtype == torch.float32
                and base <= st.data_ptr() < base + 4 * self._SLOTS):
            return (st.data_ptr() - base) // 4
        return None

    def _slot(self, p, state):
        """The parameter's slot in the device buffers; its ``state["step"]`` becomes (or stays) the 0-dim view of the slot's
        count.  A count that came from elsewhere -- a state_dict, steps taken before the mode was switched on -- is copied in."""
        b = self._buffers(p.device)
        st = state.get("step")
        slot = self._slot_of(b, st)
        if slot is not None:
            return slot, b
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("gftorf_amd.FusedAdam(capturable=True): take one eager step() before capturing (the optimizer "
                               "state of a parameter is created, or adopted, outside the graph)")
        if b["used"] >= self._SLOTS:
            # (slots of parameters that no longer exist are reclaimed: a slot is taken while the state of a parameter of
            # some group views it)
            taken = set()
            for g in self.param_groups:
                for q in g["params"]:
                    if q.device == p.device and q in self.state:
                        taken.add(self._slot_of(b, self.state[q].get("step")))
            free = sorted(set(range(self._SLOTS)) - taken)
            if not free:
                raise RuntimeError("gftorf_amd.FusedAdam(capturable=True): more than %d parameter tensors" % self._SLOTS)
            slot = free[0]
        else:
            slot = b["used"]
            b["used"] += 1
        view = b["step"][slot]
        view.fill_(float(st) if st is not None else 0.0)
        state["step"] = view
        return slot, b

    def lr_on_device(self, on=True):
        """``lr_on_device(True)``: the learning rates a step reads are whatever the device slots hold -- what the last
        ``schedule.RunSchedule.tick()`` wrote there (``lr_slots()`` are its destinations).  ``step()`` no longer copies the
        rates of ``param_groups`` to the device and ``refresh_lr()`` raises: a captured ``{tick; step}`` is the whole
        statement, and two replays can follow one another with no host work in between.  ``lr_on_device(False)``, the
        default, is the route through pinned memory described above.  Capturable mode only.  Returns the optimizer."""
        if on and not self._gft_capturable:
            raise RuntimeError("gftorf_amd.FusedAdam: lr_on_device(True) needs FusedAdam(capturable=True)")
        self._gft_lr_on_device = bool(on)
        return self

    def lr_slots(self):
        """For every group of ``param_groups``, in order, the device addresses of the float64 learning-rate slots of its
        parameters (one per parameter tensor that has taken a step; a slot stays with the parameter's state dict, so a
        re-keyed parameter keeps its slot).  RuntimeError for a parameter without a slot: take one eager ``step()`` first."""
        if not self._gft_capturable:
            raise RuntimeError("gftorf_amd.FusedAdam: lr_slots() needs FusedAdam(capturable=True)")
        out = []
        for group in self.param_groups:
            slots = []
            for p in group["params"]:
                b = self._gft_dev.get(p.device)
                slot = self._slot_of(b, self.state[p].get("step")) if b is not None and p in self.state else None
                if slot is None:
                    raise RuntimeError("gftorf_amd.FusedAdam: lr_slots(): a parameter of group %r has no slot yet; take one eager "
                                       "step() first" % (group.get("name", len(out)),))
                slots.append(b["lr"].data_ptr() + 8 * slot)
            out.append(slots)
        return out

    def refresh_lr(self):
        """Writes the groups' current learning rates where a captured step reads them (pinned host memory: no device work,
        no synchronisation).  Call it after the scheduler has set ``param_groups[...]["lr"]`` and before the replay."""
        if self._gft_lr_on_device:
            raise RuntimeError("gftorf_amd.FusedAdam: refresh_lr() in the lr_on_device(True) mode: the rates are written on the "
                               "device by schedule.RunSchedule.tick(); change them there (or lr_on_device(False))")
        for group in self.param_groups:
            lr = float(group["lr"])
            for p in group["params"]:
                b = self._gft_dev.get(p.device)
                if b is not None and p in self.state:
                    slot = self._slot_of(b, self.state[p].get("step"))
                    if slot is not None:
                        b["lr_np"][slot] = lr

    def _clip_coef(self, lib, grads, max_grad_norm):
        """The device address of the clip coefficient for this step's launches (None: no clipping).  The norm runs over every
        gradient of the step -- all groups, all launch buckets, in the order of ``param_groups`` -- as ``clip_grad_norm_`` over
        the optimizer's parameters would; ``grads`` are the tensors the launches read (a gradient that was copied for
        alignment is not copied again)."""
        if max_grad_norm is None:
            return None
        if not grads:
            self.last_grad_norm = torch.tensor(0.0)
            return None
        devs = {g.device for g in grads}
        if len(devs) != 1:
            raise RuntimeError("gftorf_amd.FusedAdam: step(max_grad_norm=...) needs all gradients on one device, got %s" % sorted(map(str, devs)))
        out = _grad_norm(lib, grads[0].device, grads, max_grad_norm)
        self._gft_clip = out            # (alive until the launches that read it are on the stream and the next step replaces it)
        self.last_grad_norm = out[0]
        return out.data_ptr() + 4

    def _collect(self, visibility, rows, row_params):
        """Every tensor that takes a step, in the order of ``param_groups``: ``buckets`` maps the settings one launch shares,
        (device, betas, eps, weight decay, by rows), to its tensors as (parameter, gradient, both moments, lr, ``state["step"]``,
        slot); ``grads`` are the gradients the launches read.  Capturable: ``slot`` is the tensor's place in the device buffers,
        whose learning rate is written here (eager: None)."""
        cap = self._gft_capturable
        buckets, grads = {}, []
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            lr, eps, wd = float(group["lr"]), group["eps"], group["weight_decay"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.device.type != "cuda":
                    raise RuntimeError("gftorf_amd.FusedAdam runs on a HIP device only (parameter on %s); there is no CPU path" % (p.device,))
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("gftorf_amd.FusedAdam: parameters must be contiguous float32 tensors")
                state = self.state[p]
                if cap:
                    # (the count is created, or adopted, with its slot)
                    if "exp_avg" not in state:
                        state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    slot, b = self._slot(p, state)
                    if not self._gft_lr_on_device:
                        b["lr_np"][slot] = lr
                else:
                    if len(state) == 0:
                        # same state as torch.optim.Adam._init_group
                        state["step"] = torch.tensor(0.0, dtype=torch.float32)
                        state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    slot = None
                m, v = state["exp_avg"], state["exp_avg_sq"]
                grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                # the kernels move 16-byte pieces: a gradient that is a view at an odd offset (e.g. the rasterizer's
                # dc_offset gradient, element 1 of a two-float tensor) is copied once; parameter and moments are the
                # caller's own allocations and must be aligned as torch allocates them
                if grad.data_ptr() % 16:
                    grad = grad.clone()
                contiguous = m.is_contiguous() and v.is_contiguous()
                aligned = not (p.data_ptr() % 16 or m.data_ptr() % 16 or v.data_ptr() % 16)
                if cap and not (contiguous and aligned):
                    raise RuntimeError("gftorf_amd.FusedAdam: parameters and optimizer state must be contiguous and 16-byte aligned")
                if not contiguous:
                    raise RuntimeError("gftorf_amd.FusedAdam: optimizer state must be contiguous")
                if not aligned:
                    raise RuntimeError("gftorf_amd.FusedAdam: parameters and optimizer state must be 16-byte aligned")
                by_rows = rows is not None and p.dim() >= 1 and p.shape[0] == rows and rows > 0 and (
                    row_params is None or id(p) in row_params)
                if by_rows and visibility.device != p.device:
                    raise RuntimeError("gftorf_amd.FusedAdam: visibility is on %s, the parameter on %s" % (visibility.device, p.device))
                buckets.setdefault((p.device, float(beta1), float(beta2), float(eps), float(wd), by_rows), []).append((p, grad, m, v, lr, state["step"], slot))
                grads.append(grad)
        return buckets, grads

    @torch.no_grad()
    def step(self, closure=None, visibility=None, row_params=None, max_grad_norm=None):
        """``visibility``: opt-in row mask (see the module docstring).  ``row_params``: the parameters the mask applies to
        (an iterable of tensors; default: every parameter whose first dimension equals ``visibility.numel()`` -- name
        them when another parameter, e.g. a network weight, could have that many rows by coincidence).  A row that is
        skipped keeps its moments, and the bias correction uses the tensor's one step count: a row that was skipped
        k times is corrected as if it had taken those k steps (dense Adam differs there as well as in the decay).
        ``max_grad_norm``: the update of ``clip_grad_norm_(all parameters of this optimizer, max_grad_norm)`` followed by
        ``step()``, with ``.grad`` left unscaled and the norm in ``self.last_grad_norm`` (see the module docstring)."""
        loss = None
        rows = mask_u8 = None
        if row_params is not None:
            row_params = {id(t) for t in row_params}
        if visibility is not None:
            if visibility.dim() != 1 or visibility.dtype not in (torch.bool, torch.uint8):
                raise RuntimeError("gftorf_amd.FusedAdam: visibility must be a 1-D bool / uint8 tensor (one entry per Gaussian)")
            rows = visibility.numel()
            visibility = visibility.contiguous()
            mask_u8 = visibility.view(torch.uint8) if visibility.dtype == torch.bool else visibility
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        cap = self._gft_capturable
        buckets, grads = self._collect(visibility, rows, row_params)
        coef = self._clip_coef(lib, grads, max_grad_norm)
        copied = set()
        for (dev, beta1, beta2, eps, wd, by_rows), items in buckets.items():
            n = len(items)
            tab = (_lib.AdamTensor * n)()
            lrs = steps = factors = None
            if cap:
                b = self._buffers(dev)
                # the learning rates of this step: host values -> device, a copy node under capture (a replay re-reads the pinned
                # buffer: refresh_lr); once per device
                # (lr_on_device: the slots hold what the schedule's tick wrote)
                if dev not in copied and not self._gft_lr_on_device:
                    b["lr"].copy_(b["lr_host"], non_blocking=True)
                    copied.add(dev)
                lrs, steps, factors = (C.c_void_p * n)(), (C.c_void_p * n)(), b["factors"].data_ptr()
                lr0, st0 = b["lr"].data_ptr(), b["step"].data_ptr()
            for i, (e, (p, g, m, v, lr, st, slot)) in enumerate(zip(tab, items)):
                e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
                if cap:
                    lrs[i], steps[i] = lr0 + 8 * slot, st0 + 4 * slot
                else:
                    e.lr, e.step = lr, int(st) + 1
            with _lib.on_device(dev):
                _lib.check(lib.gft_adam_step(_lib.raw_stream(dev), n, tab, rows if by_rows else 0, mask_u8.data_ptr() if by_rows else None,
                                             lrs, steps, factors, beta1, beta2, eps, wd, coef))
            if not cap:
                # the step counters advance only once the launch was accepted (a rejected table leaves every tensor of the
                # bucket and its counter as they were)
                torch._foreach_add_([it[5] for it in items], 1)
        return loss
