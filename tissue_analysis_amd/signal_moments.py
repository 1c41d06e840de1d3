"""Where in a cell the signal sits: the signal-weighted centroid, its displacement from the cell's barycentre (polarity) and the
signal-weighted covariance and inertia axes, from the exact integer rows of the signal-moment pass
(include/tissue_scan_sigmoments.h, csrc/kernels_sigmoments.hip).  The integers stay in the memory-axis order of the pass; the
axis permutation of an image that is not C-ordered, the voxel size and every float (float64) are the host's work, here."""
from __future__ import annotations

import numpy as np

from ._tables import _ByLabel, to_array_axes, voxelsize3

PAIR_ORDER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
COLUMNS = ("centroid", "polarity", "polarity_index", "covariance")
_MASK = (1 << 64) - 1


def _words(value):
    """A non-negative Python integer below 2^128 as (low, high) 64-bit words."""
    if value < 0 or value >> 128:
        raise OverflowError("a second moment needs more than 128 bits")
    return value & _MASK, value >> 64


class SignalMoments(_ByLabel):
    """Signal-weighted moments whose rows line up with an `Extraction`: rows 0..max_label, or one per id of `.ids` when the ids
    are sparse.  Integer columns as the pass gives them, in MEMORY-axis order k = 0, 1, 2 (`perm[k]` is the array axis of k):

        n, w       voxels and sum of the signal S per row (uint64)
        m1         sum of S x_k, uint64 [R, 3]
        m2         sum of S x_j x_k for (j, k) = 00, 01, 02, 11, 12, 22: uint64 [R, 6, 2] = low, high word of a 128-bit integer
        origin0    what x_0 counts from: 0 = the volume's first plane (a slab's rows start LOCAL, at its own first owned plane:
                   `shifted` moves them)

    Floats, float64 [R, ...] in ARRAY-axis order, voxel units or (real=True) times the voxel size:

        centroid()       m1 / w, NaN where w == 0
        polarity()       centroid minus the geometric barycentre of the extraction; normalised: over the cell's radius of gyration
        covariance()     (w m2_jk - m1_j m1_k) / w^2, the numerator formed in exact integers first
        inertia_axis()   eigenvectors (rows) and eigenvalues of the covariance, by decreasing eigenvalue
    """

    def __init__(self, extraction, n, w, m1, m2, perm=(0, 1, 2), voxelsize=(1.0, 1.0, 1.0), origin0=0, ms=None):
        self.extraction = extraction
        self.ids = None if extraction is None else extraction.ids
        self.n = np.asarray(n, dtype=np.uint64).reshape(-1)
        self.w = np.asarray(w, dtype=np.uint64).reshape(-1)
        self.m1 = np.asarray(m1, dtype=np.uint64).reshape(-1, 3)
        self.m2 = np.asarray(m2, dtype=np.uint64).reshape(-1, 6, 2)
        R = self.n.size
        if self.w.size != R or self.m1.shape[0] != R or self.m2.shape[0] != R:
            raise ValueError("n, w, m1 and m2 must have one row per label")
        self.perm = tuple(int(p) for p in perm)
        if sorted(self.perm) != [0, 1, 2]:
            raise ValueError("perm must be a permutation of (0, 1, 2), not %r" % (perm,))
        self.voxelsize = voxelsize3(voxelsize)
        self.origin0 = int(origin0)
        self.ms = ms

    def __len__(self):
        return int(self.n.size)

    # ------------------------------------------------------------------ exact integers
    def m2_int(self, row):
        """The six 128-bit second moments of one row as Python integers."""
        return [(int(hi) << 64) | int(lo) for lo, hi in self.m2[row].tolist()]

    def shifted(self, origin0):
        """The same rows with x_0 counted from plane `origin0` of the volume instead of this one's `origin0` -- for a slab,
        shifted(0) is the volume's frame.  Exact: Python integers, no float."""
        o = self.origin0 - int(origin0)                       # added to every x_0
        m1 = self.m1.copy()
        m2 = self.m2.copy()
        if o:
            for r in np.flatnonzero(self.w).tolist():
                w = int(self.w[r])
                a = [int(v) for v in self.m1[r]]
                q = self.m2_int(r)
                q[0] += 2 * o * a[0] + o * o * w
                q[1] += o * a[1]
                q[2] += o * a[2]
                a[0] += o * w
                if a[0] < 0 or a[0] >> 64:
                    raise OverflowError("a first moment needs more than 64 bits after the shift")
                m1[r, 0] = a[0]
                for k in range(3):
                    m2[r, k] = _words(q[k])
        return SignalMoments(self.extraction, self.n, self.w, m1, m2, self.perm, self.voxelsize, int(origin0), self.ms)

    @staticmethod
    def merge(parts, extraction=None):
        """The rows of the slabs of one volume (each a SignalMoments of the same row count, axis order and voxel size) as one, in
        the volume's frame: every slab is shifted to origin 0 and the integers are summed exactly.  `extraction`: the whole
        volume's, for polarity()."""
        parts = [p.shifted(0) for p in parts]
        if not parts:
            raise ValueError("nothing to merge")
        R = len(parts[0])
        if any(len(p) != R or p.perm != parts[0].perm for p in parts):
            raise ValueError("the parts must have the same rows and the same axis order")
        n = np.zeros(R, dtype=np.uint64)
        w = np.zeros(R, dtype=np.uint64)
        m1 = np.zeros((R, 3), dtype=np.uint64)
        m2 = np.zeros((R, 6, 2), dtype=np.uint64)
        for r in range(R):
            n[r] = sum(int(p.n[r]) for p in parts)                # (numpy raises OverflowError past 64 bits)
            w[r] = sum(int(p.w[r]) for p in parts)
            for k in range(3):
                m1[r, k] = sum(int(p.m1[r, k]) for p in parts)
            q = [sum(v) for v in zip(*[p.m2_int(r) for p in parts])]
            for k in range(6):
                m2[r, k] = _words(q[k])
        return SignalMoments(extraction, n, w, m1, m2, parts[0].perm, parts[0].voxelsize, 0)

    # ------------------------------------------------------------------ floats, array axes
    def _scale(self):
        return np.asarray(self.voxelsize, dtype=np.float64)

    def centroid(self, real=True):
        """float64 [R, 3]: the signal-weighted centroid m1 / w per array axis, in the frame of `center_of_mass` (plus `origin0`
        along the slowest memory axis); NaN where the row holds no signal."""
        wf = self.w.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            c = self.m1.astype(np.float64) / wf[:, None]
        c[:, 0] += float(self.origin0)
        c = np.where(wf[:, None] > 0, to_array_axes(c, self.perm), np.nan)
        return c * self._scale() if real else c

    def _geometry(self):
        x = self.extraction
        if x is None:
            raise ValueError("polarity needs the extraction of the volume (merge(parts, extraction=...))")
        if self.origin0:
            raise ValueError("polarity needs rows in the volume's frame: shifted(0)")
        return x

    def gyration_radius(self, real=True):
        """float64 [R]: sqrt(trace of the geometric covariance (n sum2_kk - sum1_k^2) / n^2) of every cell of the extraction (it
        needs the second moments of the sweep), in voxel units or scaled by the voxel size; NaN for a row without voxels."""
        x = self._geometry()
        vs = self._scale() if real else np.ones(3)
        out = np.full(len(self), np.nan, dtype=np.float64)
        diag = (0, 3, 5)
        for r in np.flatnonzero(x.count).tolist():
            n = int(x.count[r])
            out[r] = sum(float(n * int(x.sum2[r, diag[k]]) - int(x.sum1[r, k]) ** 2) * vs[k] * vs[k] for k in range(3)) / (float(n) * float(n))
        return np.sqrt(np.maximum(out, 0.0))

    def polarity(self, real=True, normalised=False):
        """float64 [R, 3]: the signal centroid minus the geometric barycentre of the cell.  normalised: divided by the cell's
        radius of gyration in the same units -- dimensionless, 0 for a uniform signal.  NaN where the row holds no signal."""
        x = self._geometry()
        p = np.full((len(self), 3), np.nan, dtype=np.float64)
        for r in np.flatnonzero((self.w > 0) & (x.count > 0)).tolist():
            w, n = int(self.w[r]), int(x.count[r])
            for k in range(3):                                    # m1 / w - sum1 / n over one exact numerator: no cancellation
                a = self.perm[k]
                p[r, a] = float(int(self.m1[r, k]) * n - int(x.sum1[r, a]) * w) / (float(w) * float(n))
        if real:
            p = p * self._scale()
        if normalised:
            with np.errstate(invalid="ignore", divide="ignore"):
                p = p / self.gyration_radius(real)[:, None]
        return p

    def polarity_index(self, real=True):
        """float64 [R]: the length of the normalised polarity vector."""
        return np.linalg.norm(self.polarity(real, normalised=True), axis=1)

    def _covariance_numerator(self):
        """w m2_jk - m1_j m1_k per row, exactly (Python integers: m2 is 128-bit), as float64 [R, 6] in memory-axis pair order."""
        out = np.zeros((len(self), 6), dtype=np.float64)
        for r in np.flatnonzero(self.w).tolist():
            w = int(self.w[r])
            a = [int(v) for v in self.m1[r]]
            q = self.m2_int(r)
            out[r] = [float(w * q[k] - a[j] * a[i]) for k, (j, i) in enumerate(PAIR_ORDER)]
        return out

    def covariance(self, real=True):
        """float64 [R, 3, 3]: the signal-weighted covariance of the voxel positions, array axes; NaN where w == 0.  (It does not
        depend on `origin0`: the numerator is the same in every frame.)"""
        num = self._covariance_numerator()
        wf = self.w.astype(np.float64)
        cov = np.full((len(self), 3, 3), np.nan, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            for k, (j, i) in enumerate(PAIR_ORDER):
                c = np.where(wf > 0, num[:, k] / (wf * wf), np.nan)
                cov[:, self.perm[j], self.perm[i]] = c
                cov[:, self.perm[i], self.perm[j]] = c
        if real:
            vs = self._scale()
            cov = cov * (vs[:, None] * vs[None, :])
        return cov

    def inertia_axis(self, real=True):
        """(vectors float64 [R, 3, 3], rows = axes; values float64 [R, 3]) of the signal-weighted covariance by
        `numpy.linalg.eigh`, sorted by decreasing eigenvalue -- the shape `inertia_axis()` of the analysis returns; NaN where
        w == 0.  The plain weighted covariance: no 1 / max(3, N) and no scaling of the values by the axes' norms."""
        cov = self.covariance(real)
        vecs = np.full(cov.shape, np.nan, dtype=np.float64)
        vals = np.full(cov.shape[:2], np.nan, dtype=np.float64)
        ok = np.isfinite(cov).all(axis=(1, 2))
        if ok.any():
            val, vec = np.linalg.eigh(cov[ok])                    # ascending, eigenvectors in columns
            vals[ok] = val[:, ::-1]
            vecs[ok] = np.transpose(vec[:, :, ::-1], (0, 2, 1))
        return vecs, vals

    # ------------------------------------------------------------------ lookups by label id
    def of_labels(self, labels, column="centroid", real=True):
        """`column` ('centroid', 'polarity', 'polarity_index' or 'covariance') of every label id in `labels`, NaN for ids without
        a row."""
        if column not in COLUMNS:
            raise ValueError("column must be one of %s, not %r" % ("|".join(COLUMNS), column))
        if column == "polarity_index":
            col = self.polarity_index(real)
        elif column == "polarity":
            col = self.polarity(real)
        else:
            col = getattr(self, column)(real)
        return self._pick(col, labels, np.nan)


def resident_signal_moments(resident, signal, voxelsize=(1.0, 1.0, 1.0)):
    """The signal-moment pass over the volume resident in `resident` (a ResidentVolume), with the rows of its current extraction
    -- swept first when the context holds none that fits."""
    ctx = resident.ctx
    ctx.set_signal(signal)
    x, _ = resident.over_extraction(lambda x: ctx.sigmom_extract())
    n, w, m1, m2 = ctx.sigmom_rows()
    return SignalMoments(x, n, w, m1, m2, ctx.memory_axes(), voxelsize, ms=ctx.sigmom_timing())
