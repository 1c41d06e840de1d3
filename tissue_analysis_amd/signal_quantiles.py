"""Exact per-cell histograms, medians and quantiles of an intensity image (uint8 / uint16) over a label volume, from the integer
tables of include/tissue_scan_sighist.h (csrc/kernels_sighist.hip): the device counts voxels per (label, bin) and selects order
statistics by radix; bin edges, fractions and interpolated quantiles are float64 here on the host, like the rest of the package."""
from __future__ import annotations

import numpy as np

from . import _capi
from ._tables import _ByLabel

METHODS = ("linear", "lower", "higher", "midpoint")
NO_RANK = np.uint64(0xFFFFFFFFFFFFFFFF)


def quantile_ranks(n, q):
    """The two 0-based ranks numpy's rule needs for every (row, quantile): h = (n - 1) * q in float64, lo = floor(h), hi = ceil(h).
    n: voxels per row (R,); q: (Q,) in [0, 1].  Returns (lo u64[R, Q], hi u64[R, Q], h f64[R, Q]); rows without voxels get
    NO_RANK."""
    n = np.asarray(n, dtype=np.uint64).reshape(-1)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    if q.size and not (np.all(q >= 0.0) and np.all(q <= 1.0)):
        raise ValueError("quantiles must lie in [0, 1]")
    present = n > 0
    h = (np.where(present, n, 1).astype(np.float64) - 1.0)[:, None] * q[None, :]
    lo = np.where(present[:, None], np.floor(h), 0).astype(np.uint64)
    hi = np.where(present[:, None], np.ceil(h), 0).astype(np.uint64)
    lo[~present] = NO_RANK
    hi[~present] = NO_RANK
    return lo, hi, h


def interpolate(s_lo, s_hi, h, method="linear"):
    """The quantile from the two order statistics (u32, SIGRANK_NONE = no voxels) and h of quantile_ranks(): float64, NaN for a
    row without voxels."""
    if method not in METHODS:
        raise ValueError("method must be one of %s, not %r" % ("|".join(METHODS), method))
    none = np.asarray(s_lo) == _capi.SIGRANK_NONE
    a = np.asarray(s_lo).astype(np.float64)
    b = np.asarray(s_hi).astype(np.float64)
    if method == "lower":
        out = a
    elif method == "higher":
        out = b
    elif method == "midpoint":
        out = (a + b) / 2.0
    else:
        out = a + (b - a) * (h - np.floor(h))
    return np.where(none, np.nan, out)


class SignalHistogram(_ByLabel):
    """Per-label histogram of the signal.

        counts      uint64 (R, B)   voxels of the row with signal >> log2(bin_width) == b
        bin_width   a power of two; edges = arange(B + 1) * bin_width (bin b holds edges[b] <= S < edges[b + 1])
        n           uint64 (R,)     voxels of the row (the row sums)
    """

    def __init__(self, extraction, counts, bin_width, ms=None):
        self.extraction = extraction
        self.ids = extraction.ids
        self.counts = np.asarray(counts, dtype=np.uint64)
        self.bin_width = int(bin_width)
        self.edges = np.arange(self.counts.shape[1] + 1, dtype=np.int64) * self.bin_width
        self.n = self.counts.sum(axis=1, dtype=np.uint64)
        self.ms = ms

    def of_labels(self, labels):
        """uint64 (len(labels), B): the histogram of every label id in `labels` (zeros for ids without voxels)."""
        return self._pick(self.counts, labels, 0)

    def fraction_above(self, threshold):
        """float64 (R,): the share of every row's voxels with signal >= threshold; exact for a threshold on a bin edge, which it
        must be.  NaN for a row without voxels."""
        t = int(threshold)
        if t != threshold or t % self.bin_width or not 0 <= t <= int(self.edges[-1]):
            raise ValueError("threshold %r is not one of the bin edges (multiples of %d up to %d)" % (threshold, self.bin_width, int(self.edges[-1])))
        above = self.counts[:, t // self.bin_width:].sum(axis=1, dtype=np.uint64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.n > 0, above.astype(np.float64) / self.n.astype(np.float64), np.nan)

    def fraction_above_of(self, labels, threshold):
        """fraction_above() of every label id in `labels` (NaN for ids without voxels)."""
        return self._pick(self.fraction_above(threshold), labels, np.nan)


class SignalQuantiles(_ByLabel):
    """Per-label quantiles of the signal from exact order statistics.

        q           float64 (Q,)    the quantiles asked for
        n           uint64 (R,)     voxels of the row
        lower, higher  uint32 (R, Q)   the order statistics of ranks floor(h) and ceil(h), h = (n - 1) * q (numpy's rule);
                                    SIGRANK_NONE for a row without voxels
        values      float64 (R, Q)  the quantiles by `method` ('linear', 'lower', 'higher', 'midpoint'), NaN for such a row
    """

    def __init__(self, extraction, n, q, lower, higher, method="linear", ms=None):
        self.extraction = extraction
        self.ids = extraction.ids
        self.n = np.asarray(n, dtype=np.uint64)
        self.q = np.asarray(q, dtype=np.float64).reshape(-1)
        self.lower = np.asarray(lower, dtype=np.uint32)
        self.higher = np.asarray(higher, dtype=np.uint32)
        self.method = method
        self.ms = ms
        self.values = self.by_method(method)

    def by_method(self, method):
        return interpolate(self.lower, self.higher, quantile_ranks(self.n, self.q)[2], method)

    def of_labels(self, labels, method=None):
        """float64 (len(labels), Q): the quantiles of every label id in `labels` (NaN for ids without voxels)."""
        table = self.values if method is None or method == self.method else self.by_method(method)
        return self._pick(table, labels, np.nan)


def _bits(signal):
    if hasattr(signal, "adopt_as_signal"):           # an image on another grid with its index matrix (resample.OnGrid)
        return signal, 8 * signal.dtype.itemsize
    a = np.asarray(signal)
    if a.dtype not in _capi.SIGNAL_DTYPES:
        raise TypeError("signal images must be uint8 or uint16, not %s" % a.dtype)
    return a, 8 * a.dtype.itemsize


def resident_signal_histogram(resident, signal, bin_width=None):
    """The histogram pass over the volume resident in `resident` (a ResidentVolume).  bin_width: a power of two that leaves at
    most 256 bins (default: 1 for uint8, 256 for uint16)."""
    a, bits = _bits(signal)
    width = (1 << (bits - 8)) if bin_width is None else int(bin_width)
    log2 = width.bit_length() - 1
    if width < 1 or width != 1 << log2 or not bits - 8 <= log2 <= bits:
        raise ValueError("bin_width must be a power of two from %d to %d for a %d-bit signal, not %r" % (1 << (bits - 8), 1 << bits, bits, bin_width))
    ctx = resident.ctx
    ctx.set_signal(a)
    x, _ = resident.over_extraction(lambda x: ctx.sighist_extract(log2))
    counts = ctx.sighist_get()
    return SignalHistogram(x, counts, width, ms=ctx.sighist_timing()[0])


def resident_signal_quantiles(resident, signal, q, method="linear"):
    """Quantiles `q` of the signal per label of the volume resident in `resident`: a SignalQuantiles.  Q quantiles take up to 2 Q
    ranks a row; the device selects SIGRANK_MAX_RANKS a pass, more run in batches."""
    if method not in METHODS:
        raise ValueError("method must be one of %s, not %r" % ("|".join(METHODS), method))
    a, _ = _bits(signal)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    if q.size and not (np.all(q >= 0.0) and np.all(q <= 1.0)):
        raise ValueError("quantiles must lie in [0, 1]")
    ctx = resident.ctx
    step = _capi.SIGRANK_MAX_RANKS

    def ranks_of(x):
        lo, hi, _ = quantile_ranks(x.count, q)
        return np.concatenate([lo, hi], axis=1)                    # [R, 2 Q]

    ctx.set_signal(a)
    x, _ = resident.over_extraction(lambda x: ctx.sigrank_extract(ranks_of(x)[:, :step]) if q.size else None)
    n = np.asarray(x.count, dtype=np.uint64)
    ranks = ranks_of(x)
    values = np.zeros(ranks.shape, dtype=np.uint32)
    ms = 0.0
    for j in range(0, ranks.shape[1], step):
        if j:
            ctx.sigrank_extract(ranks[:, j:j + step])
        values[:, j:j + step] = ctx.sigrank_get()
        ms += ctx.sighist_timing()[1]
    return SignalQuantiles(x, n, q, values[:, :q.size], values[:, q.size:], method, ms=ms)
