"""The argument checks the fused scalar modules share (``tof``, ``metrics``, ``present``; ``reg`` and ``flow`` use
``devices`` and ``ptr``).  Every helper takes the module's tag (``"gftorf_amd.tof"``), which opens its messages; ``devices``
also the noun of the module's kernels (``"ToF"``: "the ToF kernels run on a HIP device only")."""
import torch


def tensor(tag, t, name, dtypes=(torch.float32,)):
    """`t` detached, after its type and dtype are checked"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: %s must be a tensor, got %s" % (tag, name, type(t).__name__))
    if t.dtype not in dtypes:
        raise TypeError("%s: %s must be %s, got %s" % (tag, name, " or ".join(str(d) for d in dtypes), t.dtype))
    return t.detach()


def devices(tag, noun, named):
    """`named`: tuples that begin (tensor, name).  Shapes and dtypes are checked first, then the devices: every tensor on the
    first one's HIP device, which is returned."""
    dev = named[0][0].device
    for t, name, *_ in named:
        if t.device.type != "cuda":
            raise RuntimeError("%s: %s is on %s; the %s kernels run on a HIP device only, there is no CPU path" % (tag, name, t.device, noun))
        if t.device != dev:
            raise RuntimeError("%s: %s is on %s, %s on %s" % (tag, name, t.device, named[0][1], dev))
    return dev


def planes(tag, t, name, least=1, most=1 << 30, want=None, keep=None):
    """A [C, H, W] float32 image (`least` <= C <= `most`; `want` words the C of the message otherwise) as (tensor, plane
    stride): taken in place when every plane is contiguous -- ``phasor[:3]`` of the 7-plane tensor, whole rows cut from every
    plane --, else copied (its first `keep` planes when only those are read)."""
    t = tensor(tag, t, name)
    if t.dim() != 3 or not least <= t.shape[0] <= most or t.shape[1] < 1 or t.shape[2] < 1:
        want = want or ("%d..%d" % (least, most) if most < 1 << 30 else ">=%d" % least)
        raise RuntimeError("%s: %s must be [%s, H, W], got %s" % (tag, name, want, list(t.shape)))
    H, W = int(t.shape[1]), int(t.shape[2])
    if not ((W == 1 or t.stride(2) == 1) and (H == 1 or t.stride(1) == W) and (t.shape[0] == 1 or t.stride(0) >= 0)):
        t = t[:keep].contiguous()
    return t, (int(t.stride(0)) if t.shape[0] > 1 else 0)


def scalar(tag, v, name, named):
    """(tensor or None, float): a one-element float32 device tensor is passed by address (and joins `named`), a number by
    value"""
    if isinstance(v, torch.Tensor):
        v = tensor(tag, v, name)
        if v.numel() != 1:
            raise RuntimeError("%s: %s must be a number or a one-element tensor, got %s" % (tag, name, list(v.shape)))
        named.append((v, name))
        return v, 0.0
    return None, float(v)


def ptr(t):
    return None if t is None else t.data_ptr()


def ptr_nonempty(t):
    """as ``ptr``, and NULL for a tensor without elements"""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def indexed_device(tag, what, device):
    """The HIP device `what` ("a TrainLog") lives on, with its index: "cuda" alone does not compare equal to the cuda:0 of the
    tensors it meets."""
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError("%s: %s lives on a HIP device, got %s; there is no CPU path" % (tag, what, device))
    return torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)
