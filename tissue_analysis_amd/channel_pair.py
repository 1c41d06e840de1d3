"""Two intensity channels A and B per cell: the ratio of their sums, their covariance and Pearson correlation, Manders' colocalisation
coefficients, the overlap coefficient and the Jaccard index of their thresholded masks, from the exact integer rows of the two-channel
pass (include/tissue_scan_cosignal.h, csrc/kernels_cosignal.hip).  Every float (float64) is the host's work, here: its numerator and
its denominator are formed as Python integers first, so no difference of large sums is ever taken in floating point."""
from __future__ import annotations

import math

import numpy as np

from ._capi import COSIGNAL_COLUMNS
from ._tables import _ByLabel

WIDE = ("sq_aa", "sq_bb", "sq_ab")                        # the 128-bit columns: uint64 [R, 2] = low, high word
WHAT = ("ratio", "covariance", "pearson", "manders_m1", "manders_m2", "overlap_coefficient", "mask_jaccard")
_MASK = (1 << 64) - 1


def _words(value):
    """A non-negative Python integer below 2^128 as (low, high) 64-bit words."""
    if value < 0 or value >> 128:
        raise OverflowError("a sum of products needs more than 128 bits")
    return value & _MASK, value >> 64


def _quotient(num, den):
    """num / den of two Python integers as a float64, correctly rounded; NaN where den == 0."""
    return num / den if den else math.nan


class ChannelPairStats(_ByLabel):
    """Two-channel statistics whose rows line up with an `Extraction`: rows 0..max_label, or one per id of `.ids` when the ids are
    sparse.  Integer columns as the pass gives them (uint64 [R]; sq_* uint64 [R, 2] = low, high word of a 128-bit integer):

        n                    voxels
        sum_a, sum_b         sum of A, of B
        sq_aa, sq_bb, sq_ab  sum of A^2, of B^2, of A B
        n_a, n_b, n_ab       voxels with A > thresholds[0]; with B > thresholds[1]; with both
        sum_a_over           sum of A over the voxels with B > thresholds[1]
        sum_b_over           sum of B over the voxels with A > thresholds[0]

    Floats, float64 [R], NaN where the denominator is zero:

        ratio()                sum_a / sum_b
        covariance()           (n sq_ab - sum_a sum_b) / n^2
        pearson()              (n sq_ab - sum_a sum_b) / sqrt((n sq_aa - sum_a^2)(n sq_bb - sum_b^2)); NaN for n < 2 or a constant channel
        manders()              (sum_a_over / sum_a, sum_b_over / sum_b): M1, M2
        overlap_coefficient()  sq_ab / sqrt(sq_aa sq_bb)
        mask_jaccard()         n_ab / (n_a + n_b - n_ab)
    """

    def __init__(self, extraction, columns, thresholds=(0, 0), ms=None):
        self.extraction = extraction
        self.ids = None if extraction is None else extraction.ids
        missing = [k for k in COSIGNAL_COLUMNS if k not in columns]
        if missing:
            raise ValueError("columns lacks %s" % ", ".join(missing))
        for k in COSIGNAL_COLUMNS:
            col = np.asarray(columns[k], dtype=np.uint64)
            setattr(self, k, col.reshape(-1, 2) if k in WIDE else col.reshape(-1))
        R = self.n.size
        if any(getattr(self, k).shape[0] != R for k in COSIGNAL_COLUMNS):
            raise ValueError("every column must have one row per label")
        self.thresholds = (int(thresholds[0]), int(thresholds[1]))
        self.ms = ms

    def __len__(self):
        return int(self.n.size)

    def columns(self):
        return dict((k, getattr(self, k)) for k in COSIGNAL_COLUMNS)

    # ------------------------------------------------------------------ exact integers
    def sq_int(self, column, row):
        """The 128-bit sum of products `column` ('sq_aa', 'sq_bb' or 'sq_ab') of one row as a Python integer."""
        if column not in WIDE:
            raise ValueError("column must be one of %s, not %r" % ("|".join(WIDE), column))
        lo, hi = getattr(self, column)[row].tolist()
        return (int(hi) << 64) | int(lo)

    def _ints(self, row):
        """(n, sum_a, sum_b, sq_aa, sq_bb, sq_ab) of one row as Python integers."""
        return (int(self.n[row]), int(self.sum_a[row]), int(self.sum_b[row]),
                self.sq_int("sq_aa", row), self.sq_int("sq_bb", row), self.sq_int("sq_ab", row))

    @staticmethod
    def merge(parts, extraction=None):
        """The rows of the slabs of one volume (each a ChannelPairStats of the same row count and thresholds) as one: every column is
        a sum over voxels, so the integers are added exactly.  `extraction`: the whole volume's, for lookups by sparse ids."""
        parts = list(parts)
        if not parts:
            raise ValueError("nothing to merge")
        R = len(parts[0])
        if any(len(p) != R or p.thresholds != parts[0].thresholds for p in parts):
            raise ValueError("the parts must have the same rows and the same thresholds")
        cols = {}
        for k in COSIGNAL_COLUMNS:
            if k in WIDE:
                out = np.zeros((R, 2), dtype=np.uint64)
                for r in range(R):
                    out[r] = _words(sum(p.sq_int(k, r) for p in parts))
            else:
                out = np.zeros(R, dtype=np.uint64)
                for r in range(R):
                    out[r] = sum(int(getattr(p, k)[r]) for p in parts)            # (numpy raises OverflowError past 64 bits)
            cols[k] = out
        return ChannelPairStats(extraction, cols, parts[0].thresholds)

    # ------------------------------------------------------------------ floats
    def _per_row(self, fn):
        out = np.full(len(self), np.nan, dtype=np.float64)
        for r in np.flatnonzero(self.n).tolist():
            out[r] = fn(r)
        return out

    def ratio(self):
        """float64 [R]: sum_a / sum_b; NaN where sum_b == 0 (a row without voxels too)."""
        return self._per_row(lambda r: _quotient(int(self.sum_a[r]), int(self.sum_b[r])))

    def covariance(self):
        """float64 [R]: the population covariance (n sq_ab - sum_a sum_b) / n^2; NaN for a row without voxels."""
        def one(r):
            n, sa, sb, _, _, qab = self._ints(r)
            return _quotient(n * qab - sa * sb, n * n)
        return self._per_row(one)

    def pearson(self):
        """float64 [R]: Pearson's r; NaN for n < 2 and where a channel is constant over the cell.  The three integers
        c = n sq_ab - sum_a sum_b, va = n sq_aa - sum_a^2 and vb = n sq_bb - sum_b^2 are exact, and c^2 <= va vb (Cauchy-Schwarz):
        where c^2 == va vb the result is exactly +1 or -1 (B = A, B = max - A), else sqrt(c^2 / (va vb)) of the correctly rounded
        quotient with the sign of c."""
        def one(r):
            n, sa, sb, qaa, qbb, qab = self._ints(r)
            if n < 2:
                return math.nan
            c, va, vb = n * qab - sa * sb, n * qaa - sa * sa, n * qbb - sb * sb
            if va == 0 or vb == 0:
                return math.nan
            if c * c == va * vb:
                return 1.0 if c > 0 else -1.0
            return math.copysign(math.sqrt((c * c) / (va * vb)), c)
        return self._per_row(one)

    def manders(self):
        """(M1, M2), float64 [R] each: sum_a_over / sum_a, the fraction of A that lies where B is over its threshold, and
        sum_b_over / sum_b; NaN where the channel's sum is 0."""
        m1 = self._per_row(lambda r: _quotient(int(self.sum_a_over[r]), int(self.sum_a[r])))
        m2 = self._per_row(lambda r: _quotient(int(self.sum_b_over[r]), int(self.sum_b[r])))
        return m1, m2

    def overlap_coefficient(self):
        """float64 [R]: Manders' overlap coefficient sq_ab / sqrt(sq_aa sq_bb); NaN where a channel is zero all over the cell."""
        def one(r):
            _, _, _, qaa, qbb, qab = self._ints(r)
            if qaa == 0 or qbb == 0:
                return math.nan
            if qab * qab == qaa * qbb:
                return 1.0
            return math.sqrt((qab * qab) / (qaa * qbb))
        return self._per_row(one)

    def mask_jaccard(self):
        """float64 [R]: n_ab / (n_a + n_b - n_ab), the Jaccard index of the two thresholded masks; NaN where both are empty."""
        return self._per_row(lambda r: _quotient(int(self.n_ab[r]), int(self.n_a[r]) + int(self.n_b[r]) - int(self.n_ab[r])))

    # ------------------------------------------------------------------ lookups by label id
    def of_labels(self, labels, what="ratio"):
        """`what` (one of WHAT) of every label id in `labels`, NaN for ids without a row."""
        if what not in WHAT:
            raise ValueError("what must be one of %s, not %r" % ("|".join(WHAT), what))
        if what.startswith("manders_"):
            col = self.manders()[0 if what.endswith("m1") else 1]
        else:
            col = getattr(self, what)()
        return self._pick(col, labels, np.nan)


def resident_channel_pair(resident, a, b, thresholds=(0, 0)):
    """The two-channel pass over the volume resident in `resident` (a ResidentVolume), with the rows of its current extraction --
    swept first when the context holds none that fits.  One upload per channel, one pass over labels + A + B."""
    thr = tuple(int(t) for t in thresholds)
    if len(thr) != 2 or any(t < 0 or t >> 32 for t in thr):
        raise ValueError("thresholds must be two integers in [0, 2^32)")
    ctx = resident.ctx
    ctx.set_signal(a)
    ctx.set_cosignal(b)
    x, _ = resident.over_extraction(lambda x: ctx.cosignal_extract(*thr))
    return ChannelPairStats(x, ctx.cosignal_rows(), ctx.cosignal_thresholds(), ms=ctx.cosignal_timing())
