"""A numpy model of the host side of tile-pull binning and of the rule by which k_tile_pull chooses a tile's sorted head,
restated from gftorf_amd/csrc/k_pull.hip and gft_internal.h (lines as of this file's writing):

  * super_shape: gft_super_shape (k_pull.hip:1221-1253) and the `copies` / `stage_cap` rules of gft_launch_super_bin
    (k_pull.hip:1281-1295);
  * depth_bins: near_bits / bin_shift of gft_super_shape (k_pull.hip:1242-1251) and gft_depth_bin (gft_internal.h:289-294);
  * head_model: pass A of k_tile_pull and its choice of the head (k_pull.hip:673-749, 775-777, 888-891) for a frame without
    tile hints.

head_model's inputs are the ORACLE's sorted lists: it says what the device must leave in tile_cnt / front_len / tile_cut for
those lists.  It is a model of the device, not a second oracle."""
import collections
import os

import numpy as np

TILE = 16                    # GFT_TILE_X = GFT_TILE_Y
SUPER_MAX = 1024             # GFT_SUPER_MAX   (gft_internal.h:97)
SLAB_MAX = 16                # GFT_SLAB_MAX    (gft_internal.h:98)
SUPER_CELLS = SUPER_MAX * SLAB_MAX
DEPTH_BINS = 4096            # GFT_DEPTH_BINS  (gft_internal.h:100)
HEAD_SLOT = 2048             # GFT_HEAD_SLOT = TPULL_KEYS: the longest sorted head
HEAD_DIRECT = 2048           # GFT_HEAD_DIRECT (gft_internal.h:102)
HEAD_TARGET = 940            # GFT_HEAD_TARGET (gft_internal.h:103)
NO_TAIL = 0xffffffff         # GFT_NO_TAIL

Shape = collections.namedtuple("Shape", "gx gy T sshift sgx sgy NS K kshift cells staged copies")
Heads = collections.namedtuple("Heads", "tile_cnt front_len has_tail cut kstop more_slabs by_crossing")


def _env_int(name):
    """atoi of the variable, 0 when it is unset or no number (the library's getenv + atoi)"""
    try:
        return int(os.environ.get(name, "0").strip() or 0)
    except ValueError:
        return 0


def super_shape(W, H, slabs=None, copies=None):
    """The supertile shape of a W x H frame.  slabs / copies: what GFT_SLABS / GFT_SUPER_COPIES would hold (None: what this
    process's environment holds, so a child process's model follows the child's knobs).  sshift = 5 means that the frame
    has no tile pull (gft_tile_pull_ok, k_pull.hip:1256): NS, K, cells are then those of the shape the loop ends at, and
    nobody uses them."""
    slabs = _env_int("GFT_SLABS") if slabs is None else int(slabs)
    copies = _env_int("GFT_SUPER_COPIES") if copies is None else int(copies)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    sshift = 1
    while True:                                                     # k_pull.hip:1228-1236
        S = 1 << sshift
        sgx, sgy = (gx + S - 1) // S, (gy + S - 1) // S
        NS = sgx * sgy
        if NS <= SUPER_MAX:
            break
        sshift += 1
    K = 4 if sshift >= 2 else 1                                     # k_pull.hip:1237-1238
    if slabs in (1, 2, 4, 8, 16):
        K = slabs
    kshift = 12 - (K.bit_length() - 1)                              # k_pull.hip:1240-1241
    cells = NS * K
    c = copies if copies in (1, 2, 4) else 8                        # k_pull.hip:1282-1283
    while c > 1 and c * cells > SUPER_CELLS:
        c >>= 1
    staged = 1024 <= cells <= 4096                                  # k_pull.hip:1292 (the scatter passes)
    return Shape(gx, gy, gx * gy, sshift, sgx, sgy, NS, K, kshift, cells, staged, c)


def tile_pull_ok(shape):
    return shape.sshift <= 4                                        # k_pull.hip:1256


def sched_words(shape):
    """gft_cell_sched_words (gft_api.hip:154-160, k_pull.hip:1263)"""
    return 2 * shape.NS * shape.K + 4 if tile_pull_ok(shape) else 0


def bin_params(znear, zfar):
    """(near_bits, bin_shift) of gft_super_shape (k_pull.hip:1242-1251); the planes are the config's floats"""
    nr = np.float32(znear) if np.float32(znear) > np.float32(1e-6) else np.float32(1e-6)
    fr = np.float32(zfar) if np.float32(zfar) > nr else np.float32(2.0) * nr
    nb, fb = int(np.array(nr, np.float32).view(np.uint32)), int(np.array(fr, np.float32).view(np.uint32))
    shift = 0
    while ((fb - nb) >> shift) >= DEPTH_BINS - 1:
        shift += 1
    return nb, shift


def depth_bins(depth_bits, znear, zfar):
    """gft_depth_bin (gft_internal.h:289-294) of uint32 depth bits"""
    nb, shift = bin_params(znear, zfar)
    d = np.asarray(depth_bits).astype(np.int64) - nb
    return np.minimum(np.maximum(d, 0) >> shift, DEPTH_BINS - 1).astype(np.int64)


def head_model(ranges, point_list, depth_bits, shape, znear, zfar):
    """What k_tile_pull leaves for every tile of an UNHINTED frame whose sorted lists are (ranges, point_list); depth_bits:
    uint32[P], the Gaussians' depth bits.  Arrays over the tiles:

      tile_cnt     hits in the slabs 0 .. kstop, kstop = the first slab at which the running count reaches HEAD_TARGET, else
                   K - 1 (k_pull.hip:675-684, 890)
      front_len    all tile_cnt hits when there are at most HEAD_DIRECT; else whole bins up to the one where the running
                   count reaches HEAD_TARGET: that bin is taken if the run stays <= 1024, or if fewer than 512 hits lie in
                   front of it and the run stays <= 2048 (k_pull.hip:729-748, 889)
      has_tail     front_len < tile_cnt, or a later slab of the tile's SUPERTILE holds an entry -- of any of its tiles
                   (more_slabs, k_pull.hip:686-687, 775)
      cut          tile_cut: NO_TAIL without a tail, else the first bin outside the head: (kstop + 1) << kshift, or the
                   crossing bin (+ 1 if taken) (k_pull.hip:729, 740, 777, 891)
      kstop, more_slabs, by_crossing (the head was chosen by the crossing rule: tile_cnt > HEAD_DIRECT)

    A supertile's slab list holds an entry iff one of its tiles has a hit there: a rectangle that meets the supertile covers
    a tile of it (the rectangles are clipped to the grid)."""
    ranges = np.asarray(ranges).astype(np.int64)
    T, K = shape.T, shape.K
    assert ranges.shape == (T, 2)
    bins_of = depth_bins(depth_bits, znear, zfar)
    per_slab = np.zeros((T, K), np.int64)
    tile_bins = []
    for t in range(T):
        b = bins_of[point_list[ranges[t, 0]:ranges[t, 1]].astype(np.int64)]
        tile_bins.append(b)
        if b.size:
            per_slab[t] = np.bincount(b >> shape.kshift, minlength=K)
    tx, ty = np.arange(T) % shape.gx, np.arange(T) // shape.gx
    q = (ty >> shape.sshift) * shape.sgx + (tx >> shape.sshift)
    cell = np.zeros((shape.NS, K), bool)
    np.logical_or.at(cell, q, per_slab > 0)
    cum = np.cumsum(per_slab, 1)
    reached = cum >= HEAD_TARGET
    kstop = np.where(reached.any(1), reached.argmax(1), K - 1)
    n = cum[np.arange(T), kstop]
    later = np.arange(K)[None, :] > kstop[:, None]
    more = (cell[q] & later).any(1)
    front = n.copy()
    first_tail = (kstop + 1) << shape.kshift
    for t in np.flatnonzero(n > HEAD_DIRECT):
        b = tile_bins[t]
        b = b[(b >> shape.kshift) <= kstop[t]]
        cnt = np.bincount(b, minlength=DEPTH_BINS)
        run = np.cumsum(cnt)
        x = int(np.argmax(run >= HEAD_TARGET))                      # the crossing bin
        before, after = int(run[x] - cnt[x]), int(run[x])
        take = after <= 1024 or (before < 512 and after <= HEAD_SLOT)
        first_tail[t] = x + (1 if take else 0)
        front[t] = after if take else before
    has_tail = (front < n) | more
    cut = np.where(has_tail, first_tail, NO_TAIL).astype(np.uint32)
    return Heads(n.astype(np.uint32), front.astype(np.uint32), has_tail, cut, kstop, more, n > HEAD_DIRECT)


def head_model_of(f, scene, shape=None):
    """head_model on an oracle forward `f` of `scene` (helpers.small_scene's layout)"""
    cfg, cam = scene["cfg"], scene["cam"]
    shape = super_shape(cfg["W"], cfg["H"]) if shape is None else shape
    bits = np.ascontiguousarray(f.geom["depths"], np.float32).view(np.uint32)
    return head_model(f.ranges, f.point_list, bits, shape, cam["znear"], cam["zfar"])
