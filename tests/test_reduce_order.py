"""The order of the two-stage sums' first stage (``csrc/gft_reduce.h``), restated in numpy and compared bit for bit with the
rows of partials the kernels write.  The other suites prove "the same bits twice" and "close to float64"; after the finish
in double the final value is almost blind to the order of the fp32 additions, the rows are not.

The order: with B workgroups of 256 threads, lane l of workgroup b adds the elements i = b * 256 + l + r * B * 256,
r = 0, 1, ..., in fp32 from +0; within each wave of 64, v = fl32(v + v[lane ^ o]) for o = 32, 16, 8, 4, 2, 1; the
workgroup's value is ((w0 + w1) + w2) + w3 in fp32.  B = clamp(ceil(total / (256 * per_thread)), 1, 1024).

Only channels whose per-element term has no multiply feeding the add are compared: the compiler may contract those into a
multiply-add, which numpy cannot follow.
"""
import numpy as np
import pytest

THREADS, MAX_BLOCKS = 256, 1024


def grid_blocks(total, per_thread):
    return min(max(-(-total // (THREADS * per_thread)), 1), MAX_BLOCKS)


def lane_layout(terms, blocks):
    """float32 [total] or [total, inner] -> [rounds, blocks, 256, inner]: what lane l of workgroup b adds in round r, the
    elements past the end as +0 (adding +0 is exact)"""
    terms = np.asarray(terms, np.float32)
    terms = terms.reshape(len(terms), -1)
    stride = blocks * THREADS
    rounds = max(-(-len(terms) // stride), 1)
    padded = np.zeros((rounds * stride, terms.shape[1]), np.float32)
    padded[:len(terms)] = terms
    return padded.reshape(rounds, blocks, THREADS, terms.shape[1])


def fold(lanes):
    """[blocks, 256] of any dtype -> [blocks]: the xor butterfly of each wave, then the waves in order"""
    v = lanes.reshape(-1, THREADS // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    t = v[:, 0, 0]
    for w in range(1, THREADS // 64):
        t = t + v[:, w, 0]
    return t


def block_sums(terms, blocks):
    """the fp32 row value of every workgroup: [blocks] float32"""
    lay = lane_layout(terms, blocks)
    lanes = np.zeros(lay.shape[1:3], np.float32)
    for r in range(lay.shape[0]):
        for c in range(lay.shape[3]):
            lanes = lanes + lay[r, :, :, c]
    assert lanes.dtype == np.float32
    return fold(lanes)


def block_counts(flags, blocks):
    lay = lane_layout(np.asarray(flags, np.float32), blocks)
    return fold(lay.sum(axis=(0, 3)).astype(np.uint32))


def noisy(rng, *shape):
    """magnitudes over six decades: fp32 addition is visibly non-associative"""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(what, got, want):
    got, want = bits(got), bits(want)
    bad = np.flatnonzero(got != want)
    print("%s: %d of %d rows differ" % (what, len(bad), len(want)))
    assert len(bad) == 0, "%s: rows %s differ" % (what, bad[:8])


@pytest.mark.parametrize("total,per_thread,inner", [(4000, 4, 1), (1000, 1, 1), (301000, 4, 1), (307200, 1, 1), (1000, 4, 3)])
def test_restatement_is_a_sum(total, per_thread, inner):
    """every row within 256 * 2^-24 * sum |x| of the float64 sum of the same elements; the rows differ from the exactly
    rounded sums, so the comparison with the kernels discriminates"""
    rng = np.random.default_rng(7)
    x = noisy(rng, total, inner)
    blocks = grid_blocks(total, per_thread)
    got = block_sums(x, blocks)
    lay = lane_layout(x, blocks).astype(np.float64)
    exact, mag = lay.sum(axis=(0, 2, 3)), np.abs(lay).sum(axis=(0, 2, 3))
    assert got.shape == (blocks,) and got.dtype == np.float32
    assert np.all(np.abs(got.astype(np.float64) - exact) <= 256 * 2.0 ** -24 * mag)
    assert np.isclose(float(exact.sum()), float(x.astype(np.float64).sum()), rtol=1e-12)
    if total >= 4000:
        assert np.any(bits(got) != bits(exact.astype(np.float32)))
    ones = rng.random(total) < 0.3
    assert int(block_counts(ones, blocks).sum()) == int(ones.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1000, 100000])
def test_reg_rows(rows, gpu):
    """[1000, 3] with 1000 pixels: 4 workgroups and a partial last round; [100000, 3]: 294 rows, the finish's loop runs twice"""
    import torch
    from gftorf_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(rows)
    d_xyz, dd = noisy(rng, rows, 3), noisy(rng, 1, 25, 40)
    n, pixels = d_xyz.size, dd.size
    blocks = grid_blocks(n + pixels, 4)
    assert int(lib.gft_reg_blocks(n, 0, pixels)) == blocks == (4 if rows == 1000 else 294)
    a, d = torch.from_numpy(d_xyz).to(gpu), torch.from_numpy(dd).to(gpu)
    partials = torch.full((blocks, _lib.REG_PARTIAL_WORDS), -1, device=gpu, dtype=torch.int32)
    res = torch.empty((int(lib.gft_reg_result_words()),), device=gpu, dtype=torch.float32)
    with _lib.on_device(gpu):
        _lib.check(lib.gft_reg_forward(_lib.raw_stream(gpu), n, 0, pixels, a.data_ptr(), None, None, 0, None, 3, 0, None, 0, d.data_ptr(),
                                       None, 1.0, 0.0, 0.0, 1.0, partials.data_ptr(), res.data_ptr()))
    got = partials.cpu().numpy().view(np.uint32)
    zeros = np.zeros(pixels, np.float32), np.zeros(n, np.float32)
    same_bits("reg |d_xyz|", got[:, 0], block_sums(np.concatenate([np.abs(d_xyz).ravel(), zeros[0]]), blocks))
    same_bits("reg dd", got[:, 3], block_sums(np.concatenate([zeros[1], dd.ravel()]), blocks))
    assert not got[:, [1, 2, 4, 5, 6, 7]].any()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,P", [((25, 40), 0), ((25, 40), 1000), ((480, 640), 0)], ids=["25x40-0", "25x40-1000", "480x640-0"])
def test_tof_log_rows(shape, P, gpu):
    """a partial last wave without and with Gaussians; 480 x 640: the 1024-workgroup cap, two rounds for some lanes"""
    import torch
    from gftorf_amd import _lib, tof
    lib = _lib.load()
    H, W = shape
    rng = np.random.default_rng(H + P)
    phasor, gt_phasor = noisy(rng, 3, H, W), noisy(rng, 3, H, W)
    depth, gt_depth, dd = noisy(rng, 1, H, W), noisy(rng, 1, H, W), noisy(rng, 1, H, W)
    amp, radii = noisy(rng, P, 1, 1), rng.integers(-2, 3, P).astype(np.int32)
    pixels = H * W
    blocks = grid_blocks(pixels + P, 1)
    assert int(lib.gft_tof_log_blocks(pixels, P)) == blocks
    on = lambda x: torch.from_numpy(x).to(gpu)
    log = tof.TrainLog(slots=1, device=gpu)
    log._partials.fill_(-1)
    log.record(on(phasor), on(depth), on(gt_phasor), 7.5, -0.2, 2.0, gt_depth=on(gt_depth), depth_distortion=on(dd),
               **(dict(amp_f_dc=on(amp), visible=on(radii)) if P else {}))
    got = log._partials[:blocks].cpu().numpy().view(np.uint32)
    tail = np.zeros(P, np.float32)
    word = _lib.TOF_LOG_FLOATS.index
    same_bits("tof dd", got[:, word("dd")], block_sums(np.concatenate([dd.ravel(), tail]), blocks))
    same_bits("tof depth_err", got[:, word("depth_err")], block_sums(np.concatenate([np.abs(depth - gt_depth).ravel(), tail]), blocks))
    visible = np.concatenate([np.zeros(pixels, bool), radii > 0])
    count = got[:, _lib.TOF_PARTIAL_WORDS - 1]
    print("tof visible: %d" % count.sum())
    assert np.array_equal(count, block_counts(visible, blocks)) and int(count.sum()) == int((radii > 0).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(25, 40), (480, 640)], ids=lambda s: "%dx%d" % s)
def test_pixel_l1_rows(shape, gpu):
    """a lane adds its pixel's three channels, then the next round's pixel; the row is fl32(t * scale)"""
    import torch
    from gftorf_amd import _lib, loss
    lib = _lib.load()
    H, W = shape
    rng = np.random.default_rng(H)
    a, b = noisy(rng, 3, H, W), noisy(rng, 3, H, W)
    blocks = grid_blocks(H * W, 4)
    assert int(lib.gft_pixel_loss_blocks(3, H, W)) == blocks
    scale = np.float32(1.0 / (3 * H * W))
    ta, tb = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    partials = torch.full((blocks,), -1.0, device=gpu, dtype=torch.float32)
    with _lib.on_device(gpu):
        _lib.check(lib.gft_pixel_loss_forward(_lib.raw_stream(gpu), loss.PIXEL_KINDS["l1"], 3, H, W, 3, 0.0, ta.data_ptr(), tb.data_ptr(),
                                              float(scale), partials.data_ptr()))
    want = block_sums(np.abs(a - b).reshape(3, H * W).T, blocks) * scale
    assert want.dtype == np.float32
    same_bits("pixel l1", partials.cpu().numpy(), want)
