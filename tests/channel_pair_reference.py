"""include/tissue_scan_cosignal.h restated in NumPy, without the library: the eleven integer columns of two channels A, B over a
label volume V (exact, whatever their size: every sum is formed from 16-bit halves whose float64 sums are exact far beyond any
volume a test can hold), and the floats of `ChannelPairStats` by the formulas of the header, from those integers."""
import math

import numpy as np

COLUMNS = ("n", "sum_a", "sum_b", "sq_aa", "sq_bb", "sq_ab", "n_a", "n_b", "n_ab", "sum_a_over", "sum_b_over")
WIDE = ("sq_aa", "sq_bb", "sq_ab")
MASK = (1 << 64) - 1


def _exact_sums(rows, values, nrows):
    """Per row the sum of `values` (uint64 below 2^32) as Python integers: two bincounts of 16-bit halves, each exact in float64."""
    lo = np.bincount(rows, weights=(values & np.uint64(0xFFFF)).astype(np.float64), minlength=nrows)
    hi = np.bincount(rows, weights=(values >> np.uint64(16)).astype(np.float64), minlength=nrows)
    assert rows.size * 65535 < 2 ** 53
    return [int(l) + (int(h) << 16) for l, h in zip(lo.tolist(), hi.tolist())]


def words(values):
    """Python integers below 2^128 as uint64 [R, 2]: low, high word."""
    return np.array([[v & MASK, v >> 64] for v in values], dtype=np.uint64).reshape(-1, 2)


def labels(V, A, B, nrows, thr_a=0, thr_b=0, rows=None, first_owned=0):
    """The columns of ta_cosignal_get for the buffer V (memory order) with channels A, B: a dict of COLUMNS -- uint64 [nrows], the
    sq_* columns uint64 [nrows, 2] -- plus "<sq>_int", the same three as lists of Python integers.  rows: the row of every voxel
    when that is not its label (a compacted context); first_owned = 1: plane 0 is a halo and adds nothing."""
    r = (V if rows is None else rows)[first_owned:].reshape(-1).astype(np.int64)
    a = A[first_owned:].reshape(-1).astype(np.uint64)
    b = B[first_owned:].reshape(-1).astype(np.uint64)
    over_a, over_b = a > np.uint64(min(int(thr_a), 2 ** 32 - 1)), b > np.uint64(min(int(thr_b), 2 ** 32 - 1))
    zero = np.uint64(0)
    exact = {
        "n": _exact_sums(r, np.ones(r.size, dtype=np.uint64), nrows),
        "sum_a": _exact_sums(r, a, nrows), "sum_b": _exact_sums(r, b, nrows),
        "sq_aa": _exact_sums(r, a * a, nrows), "sq_bb": _exact_sums(r, b * b, nrows), "sq_ab": _exact_sums(r, a * b, nrows),
        "n_a": _exact_sums(r, over_a.astype(np.uint64), nrows), "n_b": _exact_sums(r, over_b.astype(np.uint64), nrows),
        "n_ab": _exact_sums(r, (over_a & over_b).astype(np.uint64), nrows),
        "sum_a_over": _exact_sums(r, np.where(over_b, a, zero), nrows), "sum_b_over": _exact_sums(r, np.where(over_a, b, zero), nrows),
    }
    out = {}
    for k in COLUMNS:
        if k in WIDE:
            out[k] = words(exact[k])
            out[k + "_int"] = exact[k]
        else:
            out[k] = np.array(exact[k], dtype=np.uint64)
    return out


def sq_ints(columns, name):
    if name + "_int" in columns:
        return columns[name + "_int"]
    return [(int(hi) << 64) | int(lo) for lo, hi in np.asarray(columns[name]).reshape(-1, 2).tolist()]


def _div(num, den):
    return num / den if den else math.nan


def floats(columns):
    """ratio, covariance, pearson, manders_m1, manders_m2, overlap_coefficient, mask_jaccard: float64 [R] each, by the formulas of
    the header from the integer columns; NaN for a row without voxels and where a denominator is zero."""
    R = len(columns["n"])
    names = ("ratio", "covariance", "pearson", "manders_m1", "manders_m2", "overlap_coefficient", "mask_jaccard")
    out = dict((k, np.full(R, np.nan)) for k in names)
    qaa, qbb, qab = (sq_ints(columns, k) for k in WIDE)
    for r in range(R):
        n, sa, sb = int(columns["n"][r]), int(columns["sum_a"][r]), int(columns["sum_b"][r])
        if not n:
            continue
        out["ratio"][r] = _div(sa, sb)
        c, va, vb = n * qab[r] - sa * sb, n * qaa[r] - sa * sa, n * qbb[r] - sb * sb
        out["covariance"][r] = c / (n * n)
        if n >= 2 and va > 0 and vb > 0:
            out["pearson"][r] = c / (math.sqrt(va) * math.sqrt(vb))
        out["manders_m1"][r] = _div(int(columns["sum_a_over"][r]), sa)
        out["manders_m2"][r] = _div(int(columns["sum_b_over"][r]), sb)
        if qaa[r] and qbb[r]:
            out["overlap_coefficient"][r] = qab[r] / (math.sqrt(qaa[r]) * math.sqrt(qbb[r]))
        out["mask_jaccard"][r] = _div(int(columns["n_ab"][r]), int(columns["n_a"][r]) + int(columns["n_b"][r]) - int(columns["n_ab"][r]))
    return out
