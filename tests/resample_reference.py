"""A NumPy restatement of include/tissue_scan_resample.h, without the library: the source index of every target voxel in the
stated order of operations (NumPy never fuses a product into a sum), floor(s + 0.5) for nearest neighbour, three nested lerps
and rint for trilinear, `fill` and the count of it outside the source; and the launch plan of kernels_resample.hip.  The GPU
tests ask for EXACT equality with this file."""
import fractions

import numpy as np

NEAREST, LINEAR = 0, 1
RS_WAVES, RS_PLANES, RS_MAX_GROUPS, RS_VOXEL_CAP_LOG2 = 4, 4, 4096, 31      # kernels_resample.hip


def source_index(A, shape, origin0=0):
    """s[x] (three float64 arrays of `shape`): ((A[x][0] i0 + A[x][1] i1) + A[x][2] i2) + A[x][3], every operation rounded on its
    own; target plane k along axis 0 is the global plane origin0 + k."""
    A = np.asarray(A, dtype=np.float64).reshape(3, 4)
    i0, i1, i2 = np.meshgrid(np.arange(shape[0], dtype=np.float64) + float(origin0), np.arange(shape[1], dtype=np.float64),
                             np.arange(shape[2], dtype=np.float64), indexing="ij")
    return [((A[x, 0] * i0 + A[x, 1] * i1) + A[x, 2] * i2) + A[x, 3] for x in range(3)]


def resample(S, A, shape, mode=NEAREST, fill=0, origin0=0):
    """(output of `shape` in S's dtype, bool image: the voxel received `fill`)."""
    S = np.asarray(S)
    m = S.shape
    s = source_index(A, shape, origin0)
    fillv = np.array(int(fill) & 0xFFFFFFFF).astype(np.uint32).astype(S.dtype)
    if mode == NEAREST:
        q = [np.floor(sx + 0.5) for sx in s]
        inside = np.ones(shape, dtype=bool)
        for x in range(3):
            inside &= (q[x] >= 0.0) & (q[x] < float(m[x]))
        qi = [np.where(inside, q[x], 0.0).astype(np.int64) for x in range(3)]
        out = np.where(inside, S[qi[0], qi[1], qi[2]], fillv).astype(S.dtype)
        return out, ~inside
    if S.dtype.itemsize == 4:
        raise ValueError("linear mode takes 1- or 2-byte sources")
    inside = np.ones(shape, dtype=bool)
    for x in range(3):
        inside &= (s[x] >= -0.5) & (s[x] < float(m[x]) - 0.5)
    f = [np.floor(np.where(inside, s[x], 0.0)) for x in range(3)]
    w = [np.where(inside, s[x], 0.0) - f[x] for x in range(3)]
    lo = [np.clip(f[x].astype(np.int64), 0, m[x] - 1) for x in range(3)]
    hi = [np.clip(f[x].astype(np.int64) + 1, 0, m[x] - 1) for x in range(3)]
    D = S.astype(np.float64)

    def lerp(a, b, t):
        return a + t * (b - a)

    def along2(q0, q1):
        return lerp(D[q0, q1, lo[2]], D[q0, q1, hi[2]], w[2])

    def along1(q0):
        return lerp(along2(q0, lo[1]), along2(q0, hi[1]), w[1])

    v = np.rint(lerp(along1(lo[0]), along1(hi[0]), w[0]))
    out = np.where(inside, v, float(fillv)).astype(S.dtype)
    return out, ~inside


def outside(filled, first_owned=0):
    return int(np.count_nonzero(filled[first_owned:]))


def exact_axis(a, i, b):
    """a * i + b with ONE rounding at the end (what a fused multiply-add gives), by rational arithmetic."""
    return float(fractions.Fraction(a) * int(i) + fractions.Fraction(b))


def plan(dims, itemsize):
    """(ncb, nrb, npb, tiles, tiles_per_group, groups) of the gather over a buffer of memory dims `dims`: every plane, the halo
    plane too, is tiled."""
    n0, n1, n2 = (int(d) for d in dims)
    cols = 64 * (16 // int(itemsize))
    ceil = lambda a, b: (a + b - 1) // b
    ncb, nrb, npb = ceil(n2, cols), ceil(n1, RS_WAVES), ceil(n0, RS_PLANES)
    tiles = ncb * nrb * npb
    per = min(ceil(tiles, RS_MAX_GROUPS), (1 << RS_VOXEL_CAP_LOG2) // (RS_WAVES * cols * RS_PLANES))
    return ncb, nrb, npb, tiles, per, ceil(tiles, per)


def rotation_with_scales():
    """The 30 degree rotation about axis 0 with axis scales 0.9 / 0.45 / 0.2 and offset (0.3, 3.1, 0.7): target 5 x 7 x 70 from
    source 6 x 9 x 24."""
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    R = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    A = np.zeros((3, 4))
    A[:, :3] = R * np.array([0.9, 0.45, 0.2])[None, :]
    A[:, 3] = (0.3, 3.1, 0.7)
    return A


def random_source(shape, dtype, seed=20261020):
    rng = np.random.default_rng(seed)
    return rng.integers(0, int(np.iinfo(dtype).max) + 1, size=shape, dtype=np.uint64).astype(dtype)
