"""Reference for the distance-shell profiles (include/tissue_scan_profile.h), host only, plain NumPy.

table(V, d2, S, edges2, rows): the shell of a voxel is numpy.searchsorted(edges2, d2, side='right') - 1, kept where it lies in
0 .. K - 1 (so a voxel below the first edge, at or above the last, or at +inf is counted nowhere: searchsorted puts +inf behind a
last edge of +inf too); then numpy.add.at / minimum.at / maximum.at per (row, shell), the sum of squares in Python integers."""
import numpy as np


def shells(d2, edges2):
    """(shell of every voxel, bool: it is counted)."""
    edges2 = np.asarray(edges2, dtype=np.float64)
    k = np.searchsorted(edges2, np.asarray(d2, dtype=np.float64), side="right").astype(np.int64) - 1
    return k, (k >= 0) & (k < edges2.size - 1)


def table(V, d2, S, edges2, rows):
    """dict n u64[rows, K]; with S also sum u64, sumsq object (Python integers), min u32 (UINT32_MAX where empty), max u32 (0)."""
    V = np.asarray(V)
    K = len(edges2) - 1
    k, keep = shells(np.asarray(d2).reshape(V.shape), edges2)
    at = (V[keep].astype(np.int64), k[keep])
    out = dict(n=np.zeros((rows, K), dtype=np.uint64))
    np.add.at(out["n"], at, np.uint64(1))
    if S is not None:
        s = np.asarray(S)[keep]
        out["sum"] = np.zeros((rows, K), dtype=np.uint64)
        np.add.at(out["sum"], at, s.astype(np.uint64))
        out["sumsq"] = np.zeros((rows, K), dtype=object)
        np.add.at(out["sumsq"], at, s.astype(object) ** 2)
        out["min"] = np.full((rows, K), 0xFFFFFFFF, dtype=np.uint32)
        np.minimum.at(out["min"], at, s.astype(np.uint32))
        out["max"] = np.zeros((rows, K), dtype=np.uint32)
        np.maximum.at(out["max"], at, s.astype(np.uint32))
    return out


def table_by_id(V, d2, S, edges2):
    """(ids ascending, table) with one row per id present."""
    ids = np.unique(V)
    return ids, table(np.searchsorted(ids, V), d2, S, edges2, len(ids))


def words(sumsq):
    """The (rows, K, 2) uint64 low and high words of an object array of Python integers."""
    lo = np.vectorize(lambda q: int(q) & 0xFFFFFFFFFFFFFFFF, otypes=[np.uint64])
    hi = np.vectorize(lambda q: int(q) >> 64, otypes=[np.uint64])
    if not sumsq.size:
        return np.zeros(sumsq.shape + (2,), dtype=np.uint64)
    return np.stack([lo(sumsq), hi(sumsq)], axis=-1)
