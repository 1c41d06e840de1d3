"""The oriented extents of include/tissue_scan_extents.h restated in NumPy, without the library: (1) lo = min p and hi = max p per
row with p = (x0 w[k][0] + x1 w[k][1]) + x2 w[k][2], every product and every sum an array operation of its own, so each is rounded
to float64 on its own and in that order; (2) the same with the two fused multiply-adds a contracting compiler makes of it, which
must NOT agree; (3) the launch plan of kernels_extents.hip and the spills no hash can avoid; (4) weight tables on which (1) and
(2) differ."""
import fractions
import math

import numpy as np

import range_tiles

LABEL_SLOTS = 768                 # rows of a workgroup's LDS table (EX_SLOTS of csrc/ta_extents.h)
MAX_GROUPS = 1024                 # EX_MAX_GROUPS
WAVES, PLANES = range_tiles.WAVES, range_tiles.PLANES        # EX_WAVES, EX_PLANES: the tile of the other range passes
VOXEL_CAP_LOG2 = 62               # EX_RANGE: no u32 counter, the widest shift plan_ranges takes
SCALE = (0.37, 0.53, 1.1)         # a voxel size whose entries are no short binary fractions


def weights(nrows, seed, scale=SCALE, sign=None):
    """float64 [nrows, 3, 3]: per row three random unit vectors times `scale`; sign = -1 makes every entry negative, +1 positive."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(int(nrows), 3, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    if sign is not None:
        u = float(sign) * np.abs(u)
    return np.ascontiguousarray(u * np.asarray(scale, dtype=np.float64))


def _grouped(Vm, nrows):
    """The voxels of the memory-order volume Vm with a label below nrows, sorted by label: (labels present, first index of each
    in the sorted order, x0, x1, x2 float64 in that order, the label of every voxel)."""
    flat = np.asarray(Vm).reshape(-1).astype(np.int64)
    order = np.argsort(flat, kind="stable")
    order = order[flat[order] < int(nrows)]
    lab = flat[order]
    x0, x1, x2 = (c.astype(np.float64) for c in np.unravel_index(order, Vm.shape))
    present, starts = np.unique(lab, return_index=True)
    return present, starts, x0, x1, x2, lab


def _reduce(p, present, starts, nrows):
    lo = np.full(int(nrows), np.inf)
    hi = np.full(int(nrows), -np.inf)
    if present.size:
        lo[present] = np.minimum.reduceat(p, starts) + 0.0        # (-0.0 + 0.0 == +0.0: one zero, whichever was met)
        hi[present] = np.maximum.reduceat(p, starts) + 0.0
    return lo, hi


def rows(Vm, w, nrows=None):
    """(lo f64[R, 3], hi f64[R, 3]) of the memory-order label volume Vm and the table w[R, 3, 3]; +inf, -inf without voxels."""
    w = np.asarray(w, dtype=np.float64)
    nrows = w.shape[0] if nrows is None else int(nrows)
    present, starts, x0, x1, x2, lab = _grouped(Vm, nrows)
    lo, hi = np.zeros((nrows, 3)), np.zeros((nrows, 3))
    for k in range(3):
        a = x0 * w[lab, k, 0]
        b = x1 * w[lab, k, 1]
        a = a + b
        b = x2 * w[lab, k, 2]
        lo[:, k], hi[:, k] = _reduce(a + b, present, starts, nrows)
    return lo, hi


def fma(x, y, z):
    """x * y + z rounded once."""
    if hasattr(math, "fma"):
        return math.fma(x, y, z)
    return float(fractions.Fraction(x) * fractions.Fraction(y) + fractions.Fraction(z))       # (exact, then one correct rounding)


def rows_fused(Vm, w, nrows=None):
    """rows() as a compiler that contracts would compute it: p = fma(x2, w2, fma(x1, w1, x0 * w0)).  Small volumes only."""
    w = np.asarray(w, dtype=np.float64)
    nrows = w.shape[0] if nrows is None else int(nrows)
    present, starts, x0, x1, x2, lab = _grouped(Vm, nrows)
    lo, hi = np.zeros((nrows, 3)), np.zeros((nrows, 3))
    for k in range(3):
        wk = w[lab, k].tolist()
        p = np.array([fma(c, v[2], fma(b, v[1], a * v[0])) for a, b, c, v in zip(x0.tolist(), x1.tolist(), x2.tolist(), wk)])
        lo[:, k], hi[:, k] = _reduce(p, present, starts, nrows)
    return lo, hi


def plan(dims, label_itemsize):
    """range_tiles.plan with this pass's RangeShape (dims: the buffer dims in memory order; the pass takes no slab)."""
    n0, n1, n2 = (int(d) for d in dims)
    cols = range_tiles.columns(label_itemsize)
    ncb, nrb, npb = range_tiles._ceil(n2, cols), range_tiles._ceil(n1, WAVES), range_tiles._ceil(n0, PLANES)
    tiles = ncb * nrb * npb
    most = (1 << VOXEL_CAP_LOG2) // (WAVES * cols * PLANES)
    per = min(range_tiles._ceil(tiles, MAX_GROUPS), most)
    groups = range_tiles._ceil(tiles, per)
    return range_tiles.Plan(ncb, nrb, npb, tiles, per, groups, tiles - (groups - 1) * per)


def label_spill_bound(V):
    """range_tiles.label_spill_bound with this pass's plan and slots: of the D distinct labels of a workgroup's range at least
    D - LABEL_SLOTS never get a slot, and each of them hands over at least one record."""
    p = plan(V.shape, V.dtype.itemsize)
    g = range_tiles.group_image(V.shape, 0, V.dtype.itemsize, None, p)
    distinct = range_tiles._distinct_per_group(g.reshape(-1), V.reshape(-1).astype(np.uint64), p.groups)
    return range_tiles._unavoidable(distinct, LABEL_SLOTS)
