"""Distance-shell profiles of a label image: per label and per shell of distance (to the cell's own wall, or to one chosen label)
the voxels and the statistics of an intensity image (include/tissue_scan_profile.h, csrc/kernels_profile.hip).

How much of a membrane marker lies within 1 um of the wall and how much in the interior, the volume of a cell's cortical shell or
of the cell eroded by a ball of radius r, how a signal falls off with depth below the tissue surface: each is one row of this
table.  The table holds exact integers; means, standard deviations and fractions are float64 work of the host, here.  No label is
special in the table: the methods take `labels` and `exclude`, like those of `DistanceMap`."""
from __future__ import annotations

import numpy as np

from ._tables import voxelsize3


class ShellProfile(object):
    """The profile table of one label image over K shells of distance.

        labels      int64 (R,)       the label id of every row, ascending
        edges       float64 (K + 1,) the shell boundaries, DISTANCES in real units (not squared), strictly ascending from >= 0; the
                                     last may be +inf.  Shell k holds the voxels with edges[k] <= distance < edges[k + 1]; a voxel
                                     without a site (distance +inf) is in no shell
        n           uint64 (R, K)    voxels
        sum         uint64 (R, K)    sum of the signal                                         (None without a signal, as the next)
        sumsq       object (R, K)    sum of the squared signal as PYTHON INTEGERS (it is 128-bit on the device); the constructor
                                     also takes the device's (R, K, 2) uint64 low and high words
        min, max    uint32 (R, K)    extremes of the signal; UINT32_MAX / 0 where n == 0
        voxelsize   three floats     the spacing the distances were taken with
        present     bool (R,)        the label has voxels (default: it has counted ones)
        ms          milliseconds of the pass on the device; None for host tables
    """

    def __init__(self, labels, edges, n, sum=None, sumsq=None, min=None, max=None, voxelsize=(1.0, 1.0, 1.0), present=None, ms=None):
        self.labels = np.asarray(labels).astype(np.int64).reshape(-1)
        R = self.labels.size
        if R > 1 and not (np.diff(self.labels) > 0).all():
            raise ValueError("the labels of a profile table ascend")
        self.edges = np.asarray(edges, dtype=np.float64).reshape(-1)
        K = self.edges.size - 1
        if K < 1:
            raise ValueError("a profile needs two edges at least")
        if not (self.edges[0] >= 0.0) or not (np.diff(self.edges) > 0).all():
            raise ValueError("the edges of a profile ascend strictly from a distance >= 0 (and none is NaN)")
        self.n = np.asarray(n).astype(np.uint64)
        if self.n.shape != (R, K):
            raise ValueError("n must have shape (labels, shells) = (%d, %d), not %s" % (R, K, self.n.shape))
        given = [c is not None for c in (sum, sumsq, min, max)]
        if any(given) and not all(given):
            raise ValueError("the signal columns sum, sumsq, min and max come together or not at all")
        self.has_signal = all(given)
        self.sum = self.sumsq = self.min = self.max = None
        if self.has_signal:
            self.sum = np.asarray(sum).astype(np.uint64)
            q = np.asarray(sumsq)
            if q.shape == (R, K, 2):
                words = q.astype(object)
                q = words[:, :, 0] + words[:, :, 1] * (1 << 64)
            self.sumsq = np.empty((R, K), dtype=object)
            if q.shape != (R, K):
                raise ValueError("sumsq must have shape (labels, shells) or (labels, shells, 2)")
            self.sumsq[...] = np.vectorize(int, otypes=[object])(q) if q.size else q
            self.min = np.asarray(min).astype(np.uint32)
            self.max = np.asarray(max).astype(np.uint32)
            for name in ("sum", "min", "max"):
                if getattr(self, name).shape != (R, K):
                    raise ValueError("%s must have shape (labels, shells)" % name)
        self.voxelsize = voxelsize3(voxelsize)
        self.present = (self.n.sum(axis=1) > 0) if present is None else np.asarray(present, dtype=bool).reshape(-1)
        if self.present.shape != (R,):
            raise ValueError("present has one entry per label")
        self.ms = ms

    def __len__(self):
        return int(self.labels.size)

    @property
    def shells(self):
        return int(self.edges.size - 1)

    def rows_of(self, labels):
        """int64 row of every label id, -1 for an id without a row."""
        want = np.asarray(labels, dtype=np.int64).reshape(-1)
        if self.labels.size == 0:
            return np.full(want.shape, -1, dtype=np.int64)
        pos = np.minimum(np.searchsorted(self.labels, want), self.labels.size - 1)
        return np.where(self.labels[pos] == want, pos, -1).astype(np.int64)

    def _selection(self, labels, exclude):
        out = set(int(l) for l in exclude)
        if labels is None:
            ids = self.labels[self.present]
        else:
            ids = np.asarray(labels, dtype=np.int64).reshape(-1)
            rows = self.rows_of(ids)
            known = rows >= 0
            known[known] = self.present[rows[known]]
            ids = ids[known]
        return [int(l) for l in ids.tolist() if int(l) not in out]

    def _answer(self, column, labels, exclude):
        ids = self._selection(labels, exclude)
        rows = self.rows_of(ids)
        return dict((l, column[r].copy()) for l, r in zip(ids, rows.tolist()))

    def _signal(self):
        if not self.has_signal:
            raise ValueError("this profile was computed without a signal")

    def count(self, labels=None, exclude=()):
        """{label: uint64 (K,) voxels of every shell} of the labels that have voxels, without those in `exclude`."""
        return self._answer(self.n, labels, exclude)

    def volume(self, real=True, labels=None, exclude=()):
        """{label: float64 (K,) volume of every shell}, in real units (voxels times the voxel volume) or in voxels."""
        unit = float(np.prod(self.voxelsize)) if real else 1.0
        return self._answer(self.n.astype(np.float64) * unit, labels, exclude)

    def total(self, labels=None, exclude=()):
        """{label: uint64 (K,) sum of the signal in every shell}."""
        self._signal()
        return self._answer(self.sum, labels, exclude)

    def mean(self, labels=None, exclude=()):
        """{label: float64 (K,) mean of the signal in every shell}; NaN for an empty shell."""
        self._signal()
        with np.errstate(invalid="ignore", divide="ignore"):
            col = np.where(self.n > 0, self.sum.astype(np.float64) / self.n.astype(np.float64), np.nan)
        return self._answer(col, labels, exclude)

    def std(self, labels=None, exclude=()):
        """{label: float64 (K,) population standard deviation (ddof = 0) of the signal in every shell}, from n * sumsq - sum^2 in
        exact integers; NaN for an empty shell."""
        self._signal()
        n, s = self.n.astype(object), self.sum.astype(object)
        numerator = (n * self.sumsq - s * s).astype(np.float64)
        nf = self.n.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            col = np.where(self.n > 0, np.sqrt(numerator / (nf * nf)), np.nan)
        return self._answer(col, labels, exclude)

    def minimum(self, labels=None, exclude=()):
        """{label: float64 (K,) smallest signal value in every shell}; NaN for an empty shell."""
        self._signal()
        return self._answer(np.where(self.n > 0, self.min.astype(np.float64), np.nan), labels, exclude)

    def maximum(self, labels=None, exclude=()):
        """{label: float64 (K,) largest signal value in every shell}; NaN for an empty shell."""
        self._signal()
        return self._answer(np.where(self.n > 0, self.max.astype(np.float64), np.nan), labels, exclude)

    def fraction(self, labels=None, exclude=()):
        """{label: float64 (K,) the shell's share of the signal the label's counted voxels hold}; NaN where they hold none."""
        self._signal()
        s = self.sum.astype(np.float64)
        whole = s.sum(axis=1, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            col = np.where(whole > 0, s / whole, np.nan)
        return self._answer(col, labels, exclude)
