"""Signal histograms and quantiles without a GPU: the reference's model of the two-pass radix select against sorted order
statistics, the host's rank rule against numpy.quantile, include/tissue_scan_sighist.h against the binding and the library, and the
restated launch plan."""
import ctypes
import os
import re

import numpy as np
import pytest

import range_tiles as rt
import sighist_reference as ref
from tissue_analysis_amd import _capi
from tissue_analysis_amd import signal_quantiles as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON_DEBUG = r"TA_API\s+int\s+(ta_\w+_debug)\s*\(\s*ta_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+out\[4\]\s*\)\s*;"


def header():
    return open(os.path.join(ROOT, "include", "tissue_scan_sighist.h")).read()


# ---- the select ---------------------------------------------------------------------------------------------------------------
def edge_case_volume(dtype):
    """Rows of 0 (label 0), 1 (label 1) and 2 (label 2) voxels; label 3 holds the extreme values; labels 4 .. 9 random ones."""
    rng = np.random.default_rng(3)
    top = int(np.iinfo(dtype).max)
    V = rng.integers(4, 9, size=(6, 7, 50), endpoint=True).astype(np.uint16)
    S = rng.integers(0, top, size=V.shape, endpoint=True).astype(dtype)
    V[0, 0, 0] = 1
    V[0, 0, 1:3] = 2
    S[0, 0, 1:3] = (top, 0)
    extremes = [0, 255, top] if top == 255 else [0, 255, 256, 65535, 65535, 256, 255, 0, 257]
    V[1, 0, :len(extremes)] = 3
    S[1, 0, :len(extremes)] = extremes
    return V, S


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_the_two_pass_model_equals_the_sorted_order_statistics(dtype):
    V, S = edge_case_volume(dtype)
    n = np.bincount(V.reshape(-1), minlength=10).astype(np.uint64)
    assert n[:4].tolist() == [0, 1, 2, 3 if dtype == np.uint8 else 9]
    ranks = ref.standard_ranks(n)                                  # 0, the two middles, n - 1, n
    got, selectors = ref.two_pass_select(V, S, 10, ranks)
    want = ref.order_statistics(V, S, 10, ranks)
    assert np.array_equal(got, want) and np.array_equal(want, ref.order_statistics_by_counting(V, S, 10, ranks))
    assert (got[:, 4] == ref.NONE).all() and (got[0] == ref.NONE).all() and (got[1:, :4] != ref.NONE).all()
    assert got[2].tolist()[:4] == [0, 0, int(np.iinfo(dtype).max), int(np.iinfo(dtype).max)]
    assert got[3, 0] == 0 and got[3, 3] == np.iinfo(dtype).max
    if dtype == np.uint16:
        assert got[3, 1] == 256 and selectors[3] == [0, 1, 255] and selectors[0] == []
    every = np.arange(int(n[3]), dtype=np.uint64)[None, :8]          # every rank of the small row
    rows = np.full((10, every.shape[1]), ref.NO_RANK, dtype=np.uint64)
    rows[3] = every
    assert ref.two_pass_select(V, S, 10, rows)[0][3].tolist() == np.sort(S[V == 3])[:8].tolist()


def test_ranks_of_a_row_in_one_high_byte_or_in_eight():
    rng = np.random.default_rng(4)
    V = np.repeat(np.array([1, 2], dtype=np.uint16), 4000).reshape(2, 40, 100)
    S = np.empty(V.shape, dtype=np.uint16)
    S[0] = 0x7F00 + rng.integers(0, 255, size=(40, 100), endpoint=True)          # label 1: one high byte
    S[1] = rng.integers(0, 65535, size=(40, 100), endpoint=True)                 # label 2: all of them
    ranks = np.zeros((3, 8), dtype=np.uint64)
    ranks[0] = ref.NO_RANK
    ranks[1] = np.arange(8) * 571
    ranks[2] = np.arange(8) * 571
    got, selectors = ref.two_pass_select(V, S, 3, ranks)
    assert np.array_equal(got, ref.order_statistics(V, S, 3, ranks))
    assert selectors[1] == [0x7F] and len(selectors[2]) == 8 and len(set(selectors[2])) == 8
    ranks[2] = [0, 1, 2, 3, 3999, 3998, 3997, 2000]                              # duplicates of a high byte, out of order
    got, selectors = ref.two_pass_select(V, S, 3, ranks)
    assert np.array_equal(got, ref.order_statistics(V, S, 3, ranks)) and len(selectors[2]) < 8


# ---- the host's rank rule -----------------------------------------------------------------------------------------------------
Q = [0.0, 0.01, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.9, 0.999, 1.0]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("method", sq.METHODS)
def test_the_rank_rule_is_numpys(dtype, method):
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 4, 7, 10, 101, 1000, 4097):
        values = np.sort(rng.integers(0, np.iinfo(dtype).max, size=n, endpoint=True).astype(np.int64))
        got = ref.quantile(values, Q, method)
        want = np.quantile(values.astype(np.float64), Q, method=method)
        if method in ("lower", "higher"):
            assert np.array_equal(got, want), (n, method)
        else:
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg="%d %s" % (n, method))
        assert ref.quantile(values, [0.5], "midpoint")[0] == np.median(values.astype(np.float64))      # signal_median: bit-equal
    assert np.isnan(ref.quantile(np.zeros(0, dtype=np.int64), Q, method)).all()
    assert "nearest" not in sq.METHODS
    with pytest.raises(ValueError):
        sq.interpolate(np.zeros((1, 1), np.uint32), np.zeros((1, 1), np.uint32), np.zeros((1, 1)), "nearest")
    with pytest.raises(ValueError):
        sq.quantile_ranks([3], [1.01])


def test_quantile_ranks():
    lo, hi, h = sq.quantile_ranks([0, 1, 2, 5], [0.0, 0.5, 1.0])
    assert (lo[0] == sq.NO_RANK).all() and (hi[0] == sq.NO_RANK).all()
    assert lo[1:].tolist() == [[0, 0, 0], [0, 0, 1], [0, 2, 4]] and hi[1:].tolist() == [[0, 0, 0], [0, 1, 1], [0, 2, 4]]
    assert h[3].tolist() == [0.0, 2.0, 4.0]


class _Rows(object):
    ids = None

    def rows_of(self, labels, missing=None):
        labels = np.asarray(labels, dtype=np.int64)
        return np.where((labels >= 0) & (labels < 3), labels, missing)


def test_histogram_and_quantile_tables_on_the_host():
    counts = np.array([[0, 0, 0, 0], [1, 2, 3, 4], [0, 0, 0, 8]], dtype=np.uint64)
    h = sq.SignalHistogram(_Rows(), counts, 64)
    assert h.edges.tolist() == [0, 64, 128, 192, 256] and h.n.tolist() == [0, 10, 8]
    f = h.fraction_above(128)
    assert np.isnan(f[0]) and f[1:].tolist() == [0.7, 1.0]
    assert h.fraction_above(0)[1:].tolist() == [1.0, 1.0] and h.fraction_above(256)[1:].tolist() == [0.0, 0.0]
    for bad in (100, 257, -64, 64.5):
        with pytest.raises(ValueError):
            h.fraction_above(bad)
    assert h.of_labels([2, 7, 1]).tolist() == [[0, 0, 0, 8], [0, 0, 0, 0], [1, 2, 3, 4]]
    got = h.fraction_above_of([1, 9], 64)
    assert got[0] == 0.9 and np.isnan(got[1])
    none = _capi.SIGRANK_NONE
    q = sq.SignalQuantiles(_Rows(), [0, 4, 2], [0.5, 1.0], [[none, none], [10, 40], [7, 9]], [[none, none], [20, 40], [9, 9]])
    assert np.isnan(q.values[0]).all() and q.values[1:].tolist() == [[15.0, 40.0], [8.0, 9.0]]
    assert q.of_labels([2, 5], method="lower").tolist()[0] == [7.0, 9.0] and np.isnan(q.of_labels([2, 5])[1]).all()


# ---- the header, the binding and the library ----------------------------------------------------------------------------------
def test_header_and_binding_agree():
    text = header()
    declared = sorted(set(re.findall(r"TA_API\s+int\s+(ta_\w+)\s*\(", text)))
    assert declared == sorted(_capi.SIGHIST_SYMBOLS) and len(declared) == 6
    assert not set(declared) & set(_capi.SYMBOLS)
    assert re.findall(r"TA_API\s+int\s+(ta_\w+_debug)\s*\(", text) == ["ta_sighist_debug"]
    assert re.findall(COMMON_DEBUG, text) == ["ta_sighist_debug"]
    for other in ("tissue_scan_signal.h", "tissue_scan_profile.h"):          # ... the signature the other headers use
        assert len(re.findall(COMMON_DEBUG, open(os.path.join(ROOT, "include", other)).read())) == 1, other
    lib = _capi.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.ta_version() == 5


def test_constants_agree():
    assert int(re.search(r"#define\s+TA_SIGRANK_MAX_RANKS\s+(\d+)", header()).group(1)) == _capi.SIGRANK_MAX_RANKS
    kernel_header = open(os.path.join(ROOT, "tissue_analysis_amd", "csrc", "ta_sighist.h")).read()
    assert int(re.search(r"#define\s+TA_SH_SLOTS\s+(\d+)", kernel_header).group(1)) == _capi.SIGHIST_SLOTS == ref.SLOTS
    assert int(re.search(r"#define\s+TA_SH_MAX_GROUPS\s+(\d+)", kernel_header).group(1)) == _capi.SIGHIST_MAX_GROUPS == ref.MAX_GROUPS
    assert int(re.search(r"SH_MAX_RANKS\s*=\s*(\d+)", kernel_header).group(1)) == _capi.SIGRANK_MAX_RANKS
    assert (ref.SLOTS * 257) * 4 <= 65536                                      # keys and rows of 256 u32 counters in 64 KB of LDS


def test_a_null_context_is_refused_without_a_gpu():
    lib = _capi.load()
    ranks = (ctypes.c_uint64 * 4)()
    assert lib.ta_sighist_extract(None, 0) == _capi.TA_EINVAL
    assert b"NULL" in lib.ta_last_error()
    assert lib.ta_sighist_get(None, None) == _capi.TA_EINVAL
    assert lib.ta_sigrank_extract(None, 1, ranks) == _capi.TA_EINVAL
    assert lib.ta_sigrank_get(None, None) == _capi.TA_EINVAL
    out = (ctypes.c_uint32 * 4)()
    assert lib.ta_sighist_debug(None, out) == _capi.TA_EINVAL
    a, b = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    assert lib.ta_sighist_timing(None, ctypes.byref(a), ctypes.byref(b)) == _capi.TA_EINVAL and (a.value, b.value) == (-1.0, -1.0)


# ---- the plan -----------------------------------------------------------------------------------------------------------------
def test_the_plan_restatement():
    G = ref.MAX_GROUPS
    p = ref.plan((16, 4, 512), 0, 2)                               # exactly one tile of uint16 labels
    assert (p.tiles, p.per, p.groups) == (1, 1, 1)
    p = ref.plan((17, 5, 513), 0, 2)                               # one voxel more along every axis: 2 x 2 x 2 tiles
    assert (p.ncb, p.nrb, p.npb, p.tiles, p.per, p.groups) == (2, 2, 2, 8, 1, 8)
    assert ref.plan((18, 5, 513), 1, 2).npb == 2 and ref.plan((17, 5, 513), 1, 2).npb == 1      # the halo plane is nobody's
    assert ref.plan((16, 4, 257), 0, 4).ncb == 2                   # uint32 labels: 256 columns a tile
    p = ref.plan((1024, 1024, 1024), 0, 4)                         # C4
    assert p.tiles == 4 * 256 * 64 and p.per == rt._ceil(p.tiles, G) and p.groups == rt._ceil(p.tiles, p.per) <= G
    for itemsize, vector in ((2, True), (2, False), (4, True), (4, False)):
        dims = ref.two_tile_dims(itemsize, vector)
        p = ref.plan(dims, 0, itemsize)
        assert p.per == 2 and G < p.tiles <= 2 * G and p.groups * 2 >= p.tiles and rt.vector_path(dims, itemsize) == vector
        smaller = (dims[0] - 1, dims[1], dims[2])                  # one plane block less: one tile a workgroup
        assert ref.plan(smaller, 0, itemsize).per == 1 or ref.plan((dims[0], dims[1] - 1, dims[2]), 0, itemsize).per == 1
    huge = ref.plan((1 << 14, 1 << 16, 1 << 18), 0, 2)             # 2^48 voxels: the u32 counters cap a workgroup at 2^31 voxels
    assert huge.per * rt.WAVES * rt.columns(2) * rt.PLANES == 1 << 31 and huge.groups > G
