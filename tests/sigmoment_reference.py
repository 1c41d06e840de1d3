"""The signal-weighted moments of include/tissue_scan_sigmoments.h restated in NumPy and Python integers, without the library:
(1) the eleven exact integers per row, (2) the floats that follow from them, and (3) the launch plan of kernels_sigmoments.hip --
the signal plan of range_tiles.py with the exactness cap of the header -- and the spills no hash can avoid.
test_signal_moments_cpu.py checks the restatement; test_gpu_signal_moments.py runs the kernels against it."""
import collections

import numpy as np

import range_tiles

PAIR_ORDER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
LABEL_SLOTS = range_tiles.LABEL_SLOTS["sigmoments"]      # rows of a workgroup's LDS table (SM_SLOTS of csrc/ta_sigmoments.h)
MAX_GROUPS = range_tiles.MAX_GROUPS["sigmoments"]        # SM_MAX_GROUPS


# ---- the integers ---------------------------------------------------------------------------------------------------------------
class _ByRow(object):
    """Sums of uint64 values over the voxels of every row (modulo 2^64: the callers keep them below), the voxels sorted once."""

    def __init__(self, row_of_voxel, nrows):
        self.nrows = nrows
        self.order = np.argsort(row_of_voxel, kind="stable")
        self.uniq, self.start = np.unique(row_of_voxel[self.order], return_index=True)

    def __call__(self, values):
        out = np.zeros(self.nrows, dtype=np.uint64)
        if self.order.size:
            out[self.uniq] = np.add.reduceat(values[self.order], self.start)
        return out


def rows(V, S, nrows, rows=None, first_owned=0):
    """The integers of every row over the voxels of V[first_owned:], coordinates = the indices along the axes of V as given (pass
    the memory-order view of an image that is not C-ordered), axis 0 counted from plane `first_owned`.  rows: the row of every
    voxel when the ids are sparse (else the label is the row).  Returns n, w (uint64 [R]), m1 (uint64 [R, 3]), m2 (object
    [R, 6]: Python integers, they pass 2^64) and m2_words (uint64 [R, 6, 2]: low, high)."""
    V = np.asarray(V)
    S = np.asarray(S)
    assert V.shape == S.shape and V.ndim == 3
    lab = (V if rows is None else np.asarray(rows))[first_owned:].astype(np.int64).reshape(-1)
    s = S[first_owned:].astype(np.uint64).reshape(-1)
    shape = (V.shape[0] - first_owned,) + V.shape[1:]
    x = [g.astype(np.uint64).reshape(-1) for g in np.meshgrid(*[np.arange(d) for d in shape], indexing="ij")]
    total = _ByRow(lab, nrows)
    out = dict(n=total(np.ones(lab.size, dtype=np.uint64)), w=total(s))
    out["m1"] = np.stack([total(s * x[k]) for k in range(3)], axis=1)      # (below 2^64 by the header's bound)
    m2 = np.zeros((nrows, 6), dtype=object)
    low = np.uint64(0xFFFFFFFF)
    for k, (j, i) in enumerate(PAIR_ORDER):
        t = s * x[j] * x[i]                                   # one voxel's term: below 2^16 * 2^48
        lo, hi = total(t & low), total(t >> np.uint64(32))      # 32-bit halves never wrap a u64 sum
        m2[:, k] = [int(a) + (int(b) << 32) for a, b in zip(lo.tolist(), hi.tolist())]
    out["m2"] = m2
    words = np.zeros((nrows, 6, 2), dtype=np.uint64)
    for r in range(nrows):
        for k in range(6):
            words[r, k] = (m2[r, k] & ((1 << 64) - 1), m2[r, k] >> 64)
    out["m2_words"] = words
    return out


def shifted(ref, o):
    """`ref` with o added to every axis-0 coordinate (Python integers throughout); m1 as an object array."""
    n, w = ref["n"], ref["w"]
    m1 = np.array([[int(v) for v in row] for row in np.asarray(ref["m1"]).tolist()], dtype=object).reshape(-1, 3)
    m2 = ref["m2"].copy()
    for r in range(n.size):
        wr = int(w[r])
        m2[r, 0] += 2 * o * m1[r, 0] + o * o * wr
        m2[r, 1] += o * m1[r, 1]
        m2[r, 2] += o * m1[r, 2]
        m1[r, 0] += o * wr
    return dict(n=n, w=w, m1=m1, m2=m2)


# ---- the floats -----------------------------------------------------------------------------------------------------------------
def floats(ref, geometry, voxelsize=(1.0, 1.0, 1.0)):
    """float64 centroid [R, 3], polarity [R, 3] and covariance [R, 3, 3] from the integers of `ref` and the geometric count
    [R], sum1 [R, 3] of `geometry` (an Extraction, or anything with those two attributes, in the same axis order as `ref`);
    every difference is taken in exact integers before the one division.  NaN where a row holds no signal."""
    vs = [float(v) for v in voxelsize]
    R = ref["n"].size
    cen = np.full((R, 3), np.nan)
    pol = np.full((R, 3), np.nan)
    cov = np.full((R, 3, 3), np.nan)
    for r in range(R):
        w = int(ref["w"][r])
        if not w:
            continue
        a = [int(v) for v in ref["m1"][r]]
        q = [int(v) for v in ref["m2"][r]]
        n = int(geometry.count[r])
        for k in range(3):
            cen[r, k] = float(a[k]) / float(w) * vs[k]
            if n:
                pol[r, k] = float(a[k] * n - int(geometry.sum1[r, k]) * w) / (float(w) * float(n)) * vs[k]
        for k, (j, i) in enumerate(PAIR_ORDER):
            cov[r, j, i] = cov[r, i, j] = float(w * q[k] - a[j] * a[i]) / (float(w) * float(w)) * (vs[j] * vs[i])
    return dict(centroid=cen, polarity=pol, covariance=cov)


# ---- the plan -------------------------------------------------------------------------------------------------------------------
Plan = collections.namedtuple("Plan", "ncb nrb npb tiles per groups tiles_in_last_group most uncapped")


def smax(signal_itemsize):
    return 255 if int(signal_itemsize) == 1 else 65535


def first_moments_fit(dims, signal_itemsize):
    """The u64 first moments cannot wrap: nvox g smax < 2^64 (else ta_sigmom_extract answers TA_EINVAL)."""
    n0, n1, n2 = (int(d) for d in dims)
    g = max(max(n0, n1, n2) - 1, 1)
    return n0 * n1 * n2 * g * smax(signal_itemsize) < 1 << 64


def plan(dims, first_owned, label_itemsize, signal_itemsize):
    """dims: the buffer dims in memory order (the halo plane included when first_owned == 1).  range_tiles.plan(..., "sigmoments")
    with the exactness cap: a workgroup takes no more tiles than keep voxels x g^2 x smax below 2^64, g = the largest buffer dim
    minus one.  most == 0 (then per == groups == 0): the pass refuses the dims.  uncapped: what the plan would be without the cap."""
    base = range_tiles.plan(dims, first_owned, label_itemsize, "sigmoments")
    tile_voxels = range_tiles.WAVES * range_tiles.columns(label_itemsize) * range_tiles.PLANES
    g = max(max(int(d) for d in dims) - 1, 1)
    exact = (1 << 64) // (g * g * smax(signal_itemsize)) // tile_voxels
    most = min((1 << range_tiles.VOXEL_CAP_LOG2["sigmoments"]) // tile_voxels, exact)
    if most == 0:
        return Plan(base.ncb, base.nrb, base.npb, base.tiles, 0, 0, 0, 0, base.per)
    per = min(base.per, most)
    groups = -(-base.tiles // per)
    return Plan(base.ncb, base.nrb, base.npb, base.tiles, per, groups, base.tiles - (groups - 1) * per, most, base.per)


def group_image(dims, first_owned, label_itemsize, signal_itemsize):
    """int64 image of the buffer: the workgroup that walks each voxel, -1 in the halo plane."""
    return range_tiles.group_image(dims, first_owned, label_itemsize, "sigmoments", plan(dims, first_owned, label_itemsize, signal_itemsize))


def label_spill_bound(V, first_owned, signal_itemsize):
    """A workgroup's table holds LABEL_SLOTS labels: of the D distinct labels of its range at least D - LABEL_SLOTS never get a slot,
    and each of them hands over at least one record.  Summed over the workgroups: a lower bound of the spill counter that holds
    whatever the hash does."""
    g = group_image(V.shape, first_owned, V.dtype.itemsize, signal_itemsize)
    own = g >= 0
    ngroups = plan(V.shape, first_owned, V.dtype.itemsize, signal_itemsize).groups
    return range_tiles._unavoidable(range_tiles._distinct_per_group(g[own], V[own].astype(np.uint64), ngroups), LABEL_SLOTS)
