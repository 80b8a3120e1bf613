"""The order of the fixed-order sum (include/gftorf_detsum.h), restated in numpy on downloaded buffers.

For a Gaussian g and a value k: the tiles whose list holds g in ascending tile index; for each, s = r0 + r1 + r2 + r3 (the four
quadrant rows, left to right); if s != 0, acc = acc + s, starting from 0.  Every addition is a float32 addition.
"""
import numpy as np


def detsum(ranges, quad_max, point_list, rows, P, nv, tile_order=None, quad_order=(0, 1, 2, 3)):
    """ranges [T, 2] uint32 (a tile's list starts at ranges[t, 0] in point_list), quad_max [T, 4] uint32 (the entries each
    quadrant walked), point_list [slots] uint32, rows [slots, 4, stride] float32 -> acc [P, nv] float32.

    tile_order / quad_order: another order of the tiles / of the four quadrant rows than the stated one -- for showing that
    the bits depend on it."""
    ranges, quad_max = np.asarray(ranges).reshape(-1, 2), np.asarray(quad_max).reshape(-1, 4)
    point_list, rows = np.asarray(point_list), np.asarray(rows, dtype=np.float32)
    assert rows.ndim == 3 and rows.shape[1] == 4 and nv <= rows.shape[2]
    acc = np.zeros((P, nv), np.float32)
    tiles = range(ranges.shape[0]) if tile_order is None else tile_order
    for tile in tiles:
        walked = int(quad_max[tile].max())              # entries some quadrant of the tile walked
        if walked == 0:
            continue
        p = int(ranges[tile, 0]) + np.arange(walked)
        g = point_list[p].astype(np.int64)
        assert len(np.unique(g)) == len(g), "a tile's list holds a Gaussian once"
        r = rows[p][:, :, :nv]
        q0, q1, q2, q3 = quad_order
        s = r[:, q0] + r[:, q1]
        s = s + r[:, q2]
        s = s + r[:, q3]
        assert s.dtype == np.float32
        acc[g] = np.where(s != 0, acc[g] + s, acc[g])
    return acc
