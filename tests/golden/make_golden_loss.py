"""Generate tests/golden/loss.npz from the reference's loss helpers (utils/loss_utils.py).

Usage: python tests/golden/make_golden_loss.py <checkout of the reference project>.  The reference
files themselves never travel; only the input/output vectors written here do.

  loss.npz : l1_loss, l2_loss, weighted_l1_loss, weighted_l1_loss_quad, weighted_l2_loss_quad (loss_utils.py:17-33, 51-53)
             and ssim (:76-123) on float64 copies of float32 image pairs -- the value of each and its autograd gradient with
             respect to the first image.  Pairs:
               rgb   3 x 37 x 53 (ragged tiles), weighted_l1 also with n = 2 (fn "weighted_l1_n2")
               quad  1 x 24 x 32, a signed quad measurement plane
               tof   2 x 24 x 36, a phasor pair
               equal 3 x 20 x 28, a block of exactly equal pixels
             keys: <pair>_a, <pair>_b (float32), <pair>_e (the weighted terms' offset), <pair>_<fn>, <pair>_<fn>_grad
"""
import os
import sys

import numpy as np
import torch


HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261016


def pair(rng, shape, signed):
    """a smooth image with structure plus noise, and a perturbed copy (float32)"""
    C, H, W = shape
    yy, xx = np.meshgrid(np.linspace(0, 3, H), np.linspace(0, 4, W), indexing="ij")
    base = np.stack([np.sin(yy * (c + 1) + c) * np.cos(xx * (c + 2)) for c in range(C)])
    a = 0.5 * base + 0.1 * rng.normal(size=shape)
    if not signed:
        a = 0.5 + 0.5 * a
    b = a + 0.08 * rng.normal(size=shape) + 0.02
    return a.astype(np.float32), b.astype(np.float32)


def main():
    sys.path.insert(0, sys.argv[1])
    from utils.loss_utils import (l1_loss, l2_loss, ssim, weighted_l1_loss,
                                  weighted_l1_loss_quad, weighted_l2_loss_quad)
    rng = np.random.default_rng(SEED)
    pairs = {"rgb": pair(rng, (3, 37, 53), False), "quad": pair(rng, (1, 24, 32), True),
             "tof": pair(rng, (2, 24, 36), True)}
    a, b = pair(rng, (3, 20, 28), False)
    b[:, 6:14, 9:21] = a[:, 6:14, 9:21]
    pairs["equal"] = (a, b)
    es = {"rgb": 0.01, "quad": 0.1, "tof": 0.1, "equal": 0.05}
    out = {}
    for name, (a, b) in pairs.items():
        e = es[name]
        C = a.shape[0]
        fns = {"l1": lambda x, y: l1_loss(x, y), "l2": lambda x, y: l2_loss(x, y),
               "weighted_l1": lambda x, y: weighted_l1_loss(x, y, e, C),
               "weighted_l1_quad": lambda x, y: weighted_l1_loss_quad(x, y, e),
               "weighted_l2_quad": lambda x, y: weighted_l2_loss_quad(x, y, e),
               "ssim": lambda x, y: ssim(x, y)}
        if name == "rgb":
            fns["weighted_l1_n2"] = lambda x, y: weighted_l1_loss(x, y, e, 2)
        out[name + "_a"], out[name + "_b"], out[name + "_e"] = a, b, np.float64(e)
        for fn, f in fns.items():
            x = torch.tensor(a, dtype=torch.float64, requires_grad=True)
            v = f(x, torch.tensor(b, dtype=torch.float64))
            v.backward()
            out["%s_%s" % (name, fn)] = np.float64(v.item())
            out["%s_%s_grad" % (name, fn)] = x.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "loss.npz"), **out)
    print("wrote loss.npz", os.path.getsize(os.path.join(HERE, "loss.npz")), "bytes")


if __name__ == "__main__":
    main()
