"""The arithmetic of gft_split_children (include/gftorf_densify.h) and of the children's scaling statements (scene/
gaussian_model.py:582-585) restated in numpy float32, one rounding per operation, and the float64 value the children's
positions are bounded against.  Helpers of tests/test_split_children.py; no device.

Child k * S + j belongs to the j-th split row.  Inputs: the split rows' own values, already gathered: xyz [S, 3], rotation
[S, 4] raw, scaling [S, 3] activated, z [N * S, 3] standard normals."""
import numpy as np

EPS = 2.0 ** -23
f32 = np.float32


def rotation_matrices(r, sqrt=np.sqrt):
    """build_rotation (utils/general_utils.py:91-112) in float32: [S, 3, 3].  `sqrt`: the square root of a float32 array;
    numpy's is correctly rounded, as the device's is."""
    r = np.asarray(r, f32)
    with np.errstate(all="ignore"):
        norm = np.asarray(sqrt(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]) + r[:, 3] * r[:, 3]), f32)
        q = r / norm[:, None]
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = np.zeros((r.shape[0], 3, 3), f32)
        one, two = f32(1), f32(2)
        R[:, 0, 0] = one - two * (y * y + z * z)
        R[:, 0, 1] = two * (x * y - w * z)
        R[:, 0, 2] = two * (x * z + w * y)
        R[:, 1, 0] = two * (x * y + w * z)
        R[:, 1, 1] = one - two * (x * x + z * z)
        R[:, 1, 2] = two * (y * z - w * x)
        R[:, 2, 0] = two * (x * z - w * y)
        R[:, 2, 1] = two * (y * z + w * x)
        R[:, 2, 2] = one - two * (x * x + y * y)
    assert R.dtype == f32
    return R


def fma(a, b, c):
    """a * b + c with one rounding: the product of two float32 is exact in float64; the sum is rounded to float64 and then
    to float32, which differs from the single rounding in rare ties only (the tests' bounds hold either)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def samples(scaling, z, N):
    """torch.normal(mean=zeros, std=scaling.repeat(N, 1)) after its normal_(0, 1): z * std + 0 ([N * S, 3])."""
    with np.errstate(all="ignore"):
        return np.asarray(z, f32) * np.tile(np.asarray(scaling, f32), (N, 1)) + f32(0)


def children(xyz, rotation, scaling, z, N, scaling_cols=3, sqrt=np.sqrt):
    """(new_xyz, new_scaling, child_max_scaling, R, s): the kernel's statements for the positions, the reference's for the
    scalings (a float32 tensor divided by a Python number is multiplied with the float32 reciprocal on the device)."""
    xyz, scaling = np.asarray(xyz, f32), np.asarray(scaling, f32)
    R = rotation_matrices(rotation, sqrt)
    s = samples(scaling, z, N)
    Rn = np.tile(R, (N, 1, 1))
    with np.errstate(all="ignore"):
        rot = fma(Rn[:, :, 2], s[:, None, 2], fma(Rn[:, :, 1], s[:, None, 1], Rn[:, :, 0] * s[:, None, 0]))
        new_xyz = rot + np.tile(xyz, (N, 1))
        inv = f32(1) / f32(0.8 * N)
        new_scaling = np.log(np.tile(scaling[:, :scaling_cols], (N, 1)) * inv)
        e = np.exp(new_scaling)
        child_max = np.where(np.isnan(e).any(axis=1), f32(np.nan), e.max(axis=1))
    assert new_xyz.dtype == new_scaling.dtype == f32
    return new_xyz, new_scaling, child_max.astype(f32), R, s


def exact(xyz, rotation, scaling, z, N):
    """The children's positions in float64 from the same float32 inputs, the quaternion normalised in float64."""
    r = np.asarray(rotation, np.float64)
    with np.errstate(all="ignore"):
        q = r / np.sqrt((r * r).sum(axis=1))[:, None]
    w, x, y, zz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([np.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - w * zz), 2 * (x * zz + w * y)], 1),
                  np.stack([2 * (x * y + w * zz), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - w * x)], 1),
                  np.stack([2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    s = np.asarray(z, np.float64) * np.tile(np.asarray(scaling, np.float64), (N, 1))
    return np.einsum("nij,nj->ni", np.tile(R, (N, 1, 1)), s) + np.tile(np.asarray(xyz, np.float64), (N, 1))


def position_bound(scaling, z, N, ref):
    """16 eps (|s_0| + |s_1| + |s_2|) + 2 eps |ref| per element: the float32 entries of R carry at most ~8 eps of absolute
    error (five roundings on magnitudes <= 2), the three products and two sums of the rotation at most 3 eps sum |R_ij s_j|
    <= 3 eps sum |s_j| (|R_ij| <= 1 up to its error), the sample's own rounding 1 eps |s_j|, the last add 1 eps |ref|."""
    s = np.abs(samples(scaling, z, N).astype(np.float64)).sum(axis=1)
    return 16 * EPS * s[:, None] + 2 * EPS * np.abs(ref)


def assert_positions(got, xyz, rotation, scaling, z, N, what):
    """Every element of `got` is NaN exactly where the exact value is, and within position_bound of it elsewhere."""
    got = np.asarray(got, np.float64)
    ref = exact(xyz, rotation, scaling, z, N)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN rows differ")
    bound = position_bound(scaling, z, N, ref)
    err = np.abs(got - ref)
    ok = nan | (err <= bound)
    worst = float(np.nanmax(np.where(nan, 0.0, err / np.where(bound > 0, bound, 1.0)))) if got.size else 0.0
    assert ok.all(), (what, "worst error / bound", worst, "elements outside", int((~ok).sum()))
    return worst
