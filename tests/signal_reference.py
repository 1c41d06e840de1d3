"""NumPy restatement of the signal statistics of include/tissue_scan_signal.h (no GPU): what the GPU pass is checked against.

labels(V, S, nrows, rows=None)  per row: n, sum, sumsq (Python-int exact, as object array), min, max
walls(V, S, first_owned=0)      per pair lo < hi (sorted): keys lo << 32 | hi, faces, side_lo, side_hi
Every number is an exact integer; `first_owned` = 1 means plane 0 of V / S is a halo plane: it adds nothing to the per-label
rows, and only its faces with plane 1 count."""
import numpy as np

UINT32_MAX = np.uint32(0xFFFFFFFF)


def labels(V, S, nrows, rows=None, first_owned=0):
    """rows: the row of every voxel (default: the label itself); nrows rows.  Worked through in chunks of planes."""
    V = np.asarray(V)
    S = np.asarray(S)
    if V.ndim == 2:
        V, S = V[:, :, None], S[:, :, None]
    R = V if rows is None else rows
    n = np.zeros(nrows, dtype=np.int64)
    total = np.zeros(nrows, dtype=np.int64)
    sq = np.zeros(nrows, dtype=np.uint64)          # (wraps like the device's low word: the tests keep it below 2^64)
    vmin = np.full(nrows, UINT32_MAX, dtype=np.uint32)
    vmax = np.zeros(nrows, dtype=np.uint32)
    step = max(1, (1 << 25) // max(1, V[0].size))
    for p in range(first_owned, V.shape[0], step):
        r = R[p:p + step].reshape(-1).astype(np.int64)
        s = S[p:p + step].reshape(-1).astype(np.int64)
        n += np.bincount(r, minlength=nrows)
        np.add.at(total, r, s)
        np.add.at(sq, r, (s * s).astype(np.uint64))
        np.minimum.at(vmin, r, s.astype(np.uint32))
        np.maximum.at(vmax, r, s.astype(np.uint32))
    return dict(n=n.astype(np.uint64), sum=total.astype(np.uint64), sumsq=sq, min=vmin, max=vmax)


def moments(ref):
    """mean, population std (ddof = 0), min, max in float64 (NaN for rows without voxels) from the integer rows."""
    n = ref["n"].astype(np.float64)
    present = ref["n"] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(present, ref["sum"].astype(np.float64) / n, np.nan)
        num = np.array([float(int(a) * int(b) - int(c) ** 2) for a, b, c in zip(ref["n"], ref["sumsq"], ref["sum"])])
        std = np.where(present, np.sqrt(num / (n * n)), np.nan)
    return dict(mean=mean, std=std, min=np.where(present, ref["min"].astype(np.float64), np.nan),
                max=np.where(present, ref["max"].astype(np.float64), np.nan))


def walls(V, S, first_owned=0):
    V = np.asarray(V)
    S = np.asarray(S)
    if V.ndim == 2:
        V, S = V[:, :, None], S[:, :, None]
    keys, faces, slo, shi = [], [], [], []
    for ax in range(3):
        a = np.swapaxes(V, 0, ax)
        b = np.swapaxes(S, 0, ax)
        lower, upper = a[:-1], a[1:]
        slower, supper = b[:-1], b[1:]
        m = lower != upper
        if ax != 0 and first_owned:               # faces inside the halo plane belong to the neighbour slab (those between
                                                  # it and plane 1 are this slab's)
            keep = np.ones(lower.shape, dtype=bool)
            idx = [slice(None)] * 3
            idx[ax] = 0                           # (axis 0 of V is axis `ax` of the swapped arrays)
            keep[tuple(idx)] = False
            m &= keep
        x, y = lower[m].astype(np.int64), upper[m].astype(np.int64)
        sx, sy = slower[m].astype(np.int64), supper[m].astype(np.int64)
        lo, hi = np.minimum(x, y).astype(np.uint64), np.maximum(x, y).astype(np.uint64)
        keys.append((lo << np.uint64(32)) | hi)
        slo.append(np.where(x < y, sx, sy))
        shi.append(np.where(x < y, sy, sx))
        faces.append(np.full(x.size, ax))
    keys = np.concatenate(keys)
    slo, shi, axes = np.concatenate(slo), np.concatenate(shi), np.concatenate(faces)
    uk, inv = np.unique(keys, return_inverse=True)
    f = np.zeros((uk.size, 3), dtype=np.uint64)
    np.add.at(f, (inv, axes), 1)
    side_lo = np.zeros(uk.size, dtype=np.int64)
    side_hi = np.zeros(uk.size, dtype=np.int64)
    np.add.at(side_lo, inv, slo)
    np.add.at(side_hi, inv, shi)
    return dict(keys=uk, lo=(uk >> np.uint64(32)).astype(np.uint32), hi=(uk & np.uint64(0xFFFFFFFF)).astype(np.uint32), faces=f,
                side_lo=side_lo.astype(np.uint64), side_hi=side_hi.astype(np.uint64))
