"""NumPy restatement of include/tissue_scan_sighist.h (no GPU): what the histogram pass and the radix select are checked against.

histogram(V, S, nrows, log2_width)      counts u64[R, B] by np.bincount(row * B + (S >> w))
order_statistics(V, S, nrows, ranks)    u32[R, n] by sorting each row's values; UINT32_MAX where rank >= n
                                        (order_statistics_by_counting: the same from a full-resolution histogram, for large volumes)
two_pass_select(V, S, nrows, ranks)     the same through the device's steps: digit histogram, prefix, remainder, selectors, dedupe
plan(dims, first_owned, itemsize)       the launch plan of the digit kernel: range_tiles.plan(..., "sighist")
`first_owned` = 1: plane 0 of V / S is a halo plane and adds nothing; `rows`: the row of every voxel (default: the label)."""
import numpy as np

import range_tiles as rt
from tissue_analysis_amd import _capi

NONE = np.uint32(0xFFFFFFFF)
NO_RANK = np.uint64(0xFFFFFFFFFFFFFFFF)
SLOTS = _capi.SIGHIST_SLOTS
MAX_GROUPS = rt.MAX_GROUPS["sighist"]       # (== _capi.SIGHIST_MAX_GROUPS: test_signal_quantiles_cpu.py)


def _flat(V, S, rows, first_owned):
    V, S = np.asarray(V), np.asarray(S)
    if V.ndim == 2:
        V, S = V[:, :, None], S[:, :, None]
    R = V if rows is None else rows
    return R[first_owned:].reshape(-1).astype(np.int64), S[first_owned:].reshape(-1).astype(np.int64)


def histogram(V, S, nrows, log2_width, rows=None, first_owned=0):
    r, s = _flat(V, S, rows, first_owned)
    B = 1 << (8 * np.asarray(S).dtype.itemsize - int(log2_width))
    return np.bincount(r * B + (s >> int(log2_width)), minlength=nrows * B).reshape(nrows, B).astype(np.uint64)


def values_by_row(V, S, nrows, rows=None, first_owned=0):
    """The sorted values of every row: a list of nrows int64 arrays."""
    r, s = _flat(V, S, rows, first_owned)
    order = np.lexsort((s, r))
    r, s = r[order], s[order]
    cuts = np.searchsorted(r, np.arange(nrows + 1))
    return [s[cuts[i]:cuts[i + 1]] for i in range(nrows)]


def order_statistics(V, S, nrows, ranks, rows=None, first_owned=0):
    ranks = np.asarray(ranks, dtype=np.uint64)
    out = np.full(ranks.shape, NONE, dtype=np.uint32)
    for i, vals in enumerate(values_by_row(V, S, nrows, rows, first_owned)):
        for j, k in enumerate(ranks[i].tolist()):
            if k < vals.size:
                out[i, j] = vals[k]
    return out


def standard_ranks(n):
    """The ranks the GPU tests ask of every row: 0, floor((n - 1) / 2), ceil((n - 1) / 2), n - 1 and n (which no row has)."""
    n = np.asarray(n, dtype=np.uint64)
    top = np.where(n > 0, n - np.uint64(1), NO_RANK)
    lo = np.where(n > 0, top // np.uint64(2), NO_RANK)
    hi = np.where(n > 0, (top + np.uint64(1)) // np.uint64(2), NO_RANK)
    return np.stack([np.where(n > 0, np.uint64(0), NO_RANK), lo, hi, top, n], axis=1).astype(np.uint64)


def _select(hist, rank):
    """(digit, remainder) of the 0-based rank in a histogram of 256 counts, None when the rank is not below their sum."""
    cum = np.cumsum(hist.astype(np.int64))
    if rank >= int(cum[-1]):
        return None
    d = int(np.searchsorted(cum, rank, side="right"))
    return d, int(rank - (int(cum[d - 1]) if d else 0))


def order_statistics_by_counting(V, S, nrows, ranks, rows=None, first_owned=0):
    """order_statistics() without a sort, for the large volumes: the full-resolution histogram (2^bits bins a row), its prefix sums
    and a search.  test_signal_quantiles_cpu.py checks that the two agree."""
    ranks = np.asarray(ranks, dtype=np.uint64)
    cum = np.cumsum(histogram(V, S, nrows, 0, rows, first_owned).astype(np.int64), axis=1)
    out = np.full(ranks.shape, NONE, dtype=np.uint32)
    for i in range(nrows):
        ok = ranks[i] < np.uint64(cum[i, -1])
        out[i, ok] = np.searchsorted(cum[i], ranks[i, ok].astype(np.int64), side="right")
    return out


def two_pass_select(V, S, nrows, ranks, rows=None, first_owned=0):
    """The device's steps.  Returns (values u32[R, n], selectors: the list of distinct high bytes per row -- what the second digit pass
    counts under; empty lists for a uint8 signal)."""
    ranks = np.asarray(ranks, dtype=np.uint64)
    bits = 8 * np.asarray(S).dtype.itemsize
    r, s = _flat(V, S, rows, first_owned)
    n = ranks.shape[1]
    out = np.full(ranks.shape, NONE, dtype=np.uint32)
    first = np.bincount(r * 256 + ((s >> (bits - 8)) & 255), minlength=nrows * 256).reshape(nrows, 256)
    selectors = []
    for i in range(nrows):
        picks = [_select(first[i], int(k)) for k in ranks[i].tolist()]
        if bits == 8:
            selectors.append([])
            for j, p in enumerate(picks):
                if p is not None:
                    out[i, j] = p[0]
            continue
        # dedupe: the distinct high bytes, each at the first rank that chose it; every voxel is added once per selector
        sel, where = [], {}
        for j, p in enumerate(picks):
            if p is not None and p[0] not in where:
                where[p[0]] = len(sel)
                sel.append(p[0])
        selectors.append(sel)
        mine = s[r == i]
        second = [np.bincount(mine[(mine >> 8) == h] & 255, minlength=256) for h in sel]
        assert sum(int(c.sum()) for c in second) == int(np.isin(mine >> 8, sel).sum())       # once per distinct selector
        for j, p in enumerate(picks):
            if p is not None:
                low = _select(second[where[p[0]]], p[1])
                out[i, j] = (p[0] << 8) | low[0]
    return out, selectors


def quantile(values, q, method):
    """The host's rank rule on the sorted int64 `values` of one row: float64 (Q,), NaN without voxels."""
    from tissue_analysis_amd import signal_quantiles as sq
    lo, hi, h = sq.quantile_ranks(np.array([values.size], dtype=np.uint64), q)
    pick = lambda k: np.array([[values[int(i)] if values.size else 0xFFFFFFFF for i in k[0]]], dtype=np.uint32)
    return sq.interpolate(pick(lo), pick(hi), h, method)[0]


# ---- the launch plan of the digit kernel --------------------------------------------------------------------------------------
def plan(dims, first_owned, label_itemsize):
    """dims: the buffer dims in memory order (the halo plane included when first_owned == 1).  The tile of the signal pass, a
    workgroup for every `per` consecutive tiles, MAX_GROUPS workgroups at most."""
    return rt.plan(dims, first_owned, label_itemsize, "sighist")


def two_tile_dims(label_itemsize, vector):
    """The smallest dims (one column block of one or two strips, whole row blocks) at which the plan gives per == 2: one tile more
    than MAX_GROUPS."""
    vpl = 16 // int(label_itemsize)
    nrb = 1
    while nrb * nrb < MAX_GROUPS + 1:
        nrb *= 2
    npb = rt._ceil(MAX_GROUPS + 1, nrb)
    return ((npb - 1) * rt.PLANES + 1, (nrb - 1) * rt.WAVES + 1, vpl if vector else vpl + 1)
