"""Per-cell and per-wall statistics of an intensity image (uint8 / uint16) over a label volume, from the exact integer sums of
the signal pass (include/tissue_scan_signal.h, csrc/kernels_signal.hip).  Float work -- means, the population standard
deviation, the wall means -- is float64 here on the host, like the rest of the package."""
from __future__ import annotations

import numpy as np

from . import _capi
from ._tables import _ByLabel

STATISTICS = ("mean", "std", "min", "max", "sum")
WALL_STATISTICS = ("mean", "sides")


class SignalStats(_ByLabel):
    """Signal statistics whose rows line up with an `Extraction`: per label, rows 0..max_label (or one per id of `.ids` when
    the ids are sparse); per wall, the pairs `.lo` < `.hi` of its pair list.

        n, sum         voxels and sum of the signal per row (uint64)
        sumsq          sum of the squared signal, uint64 [R, 2] = low, high word of a 128-bit integer
        mean, std      float64, NaN for a row without voxels; std is the population one (ddof = 0), from n*sumsq - sum^2
        min, max       float64, NaN for a row without voxels
        side_lo/_hi    per wall, the sum of the signal on the lo / hi side of every face of the pair (uint64)
        wall_mean      (side_lo + side_hi) / (2 * faces): face-weighted -- a voxel touching the wall through two faces counts
                       twice, as its area does in wall_areas()
        wall_side_means  (side_lo / faces, side_hi / faces)
    """

    def __init__(self, extraction, n, sum_, sumsq, vmin, vmax, side_lo=None, side_hi=None, ms=None):
        self.extraction = extraction
        self.ids = extraction.ids
        self.n = np.asarray(n, dtype=np.uint64)
        self.sum = np.asarray(sum_, dtype=np.uint64)
        self.sumsq = np.asarray(sumsq, dtype=np.uint64).reshape(-1, 2)
        self._min = np.asarray(vmin, dtype=np.uint32)
        self._max = np.asarray(vmax, dtype=np.uint32)
        self.side_lo = None if side_lo is None else np.asarray(side_lo, dtype=np.uint64)
        self.side_hi = None if side_hi is None else np.asarray(side_hi, dtype=np.uint64)
        self.ms = ms
        present = self.n > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            nf = self.n.astype(np.float64)
            self.mean = np.where(present, self.sum.astype(np.float64) / nf, np.nan)
            self.std = np.where(present, np.sqrt(self._variance_numerator() / (nf * nf)), np.nan)
        self.min = np.where(present, self._min.astype(np.float64), np.nan)
        self.max = np.where(present, self._max.astype(np.float64), np.nan)

    def _variance_numerator(self):
        """n * sumsq - sum^2 per row, exactly (Python integers: sumsq is 128-bit), as float64 -- never negative."""
        out = np.zeros(self.n.size, dtype=np.float64)
        for r in np.flatnonzero(self.n > 1):
            q = (int(self.sumsq[r, 1]) << 64) | int(self.sumsq[r, 0])
            out[r] = float(int(self.n[r]) * q - int(self.sum[r]) ** 2)
        return out

    def sumsq_int(self, row):
        """The 128-bit sum of squares of one row as a Python integer."""
        return (int(self.sumsq[row, 1]) << 64) | int(self.sumsq[row, 0])

    @property
    def lo(self):
        return self.extraction.pair_lo

    @property
    def hi(self):
        return self.extraction.pair_hi

    @property
    def faces(self):
        """Faces of every wall (the extraction's, summed over the three axes)."""
        return self.extraction.pair_faces.sum(axis=1)

    def _walls(self):
        if self.side_lo is None:
            raise ValueError("these statistics were computed without walls (walls=False)")

    @property
    def wall_mean(self):
        self._walls()
        f = self.faces.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (self.side_lo.astype(np.float64) + self.side_hi.astype(np.float64)) / (2.0 * f)

    @property
    def wall_side_means(self):
        self._walls()
        f = self.faces.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.side_lo.astype(np.float64) / f, self.side_hi.astype(np.float64) / f

    # ------------------------------------------------------------------ lookups by label id
    def of_labels(self, labels, statistic="mean"):
        """`statistic` ('mean', 'std', 'min', 'max' or 'sum') of every label id in `labels` (NaN / 0 for ids without voxels)."""
        if statistic not in STATISTICS:
            raise ValueError("statistic must be one of %s, not %r" % ("|".join(STATISTICS), statistic))
        return self._pick(getattr(self, statistic), labels, 0 if statistic == "sum" else np.nan)

    def wall_rows(self, lo, hi):
        """Row of every pair (lo < hi) in the pair list, -1 for a pair it does not hold."""
        keys = (self.lo.astype(np.uint64) << np.uint64(32)) | self.hi.astype(np.uint64)
        want = (np.asarray(lo, dtype=np.uint64) << np.uint64(32)) | np.asarray(hi, dtype=np.uint64)
        if keys.size == 0:
            return np.full(want.shape, -1, dtype=np.int64)
        pos = np.minimum(np.searchsorted(keys, want), keys.size - 1)
        return np.where(keys[pos] == want, pos, -1).astype(np.int64)


def resident_signal(resident, signal, walls=True):
    """The signal pass over the volume resident in `resident` (a ResidentVolume), with the rows of its current extraction --
    swept first when the context holds none that fits (walls need the pair list)."""
    ctx = resident.ctx
    ctx.set_signal(signal)
    what = _capi.SIG_LABELS | (_capi.SIG_WALLS if walls else 0)
    x, _ = resident.over_extraction(lambda x: ctx.signal_extract(what))
    n, s, q, mn, mx = ctx.signal_labels()
    side_lo = side_hi = None
    if walls:
        side_lo, side_hi = ctx.signal_walls()
    return SignalStats(x, n, s, q, mn, mx, side_lo, side_hi, ms=ctx.signal_timing())
