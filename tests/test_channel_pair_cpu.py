"""Two-channel statistics without a GPU: include/tissue_scan_cosignal.h against the binding and the library, `ChannelPairStats`
from hand-made integer rows (exactness of Pearson's r, the NaN rules, slabs, the 128-bit words), and the restatement of
tests/channel_pair_reference.py against a brute loop per label and numpy.corrcoef."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import channel_pair_reference as ref
from tissue_analysis_amd import ChannelPairStats, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "tissue_scan_cosignal.h")).read()


# ---- header, binding, library -------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    text = header()
    declared = sorted(set(re.findall(r"TA_API\s+int\s+(ta_\w+)\s*\(", text)))
    assert declared == sorted(_capi.COSIGNAL_SYMBOLS) and len(declared) == 7
    assert not set(_capi.COSIGNAL_SYMBOLS) & set(_capi.SYMBOLS)
    debug = [name for name in declared if name.endswith("_debug")]
    assert debug == ["ta_cosignal_debug"]
    assert re.search(r"TA_API\s+int\s+ta_cosignal_debug\s*\(ta_ctx\*\s*ctx,\s*uint32_t\s+out\[4\]\)", text)
    get = re.search(r"TA_API\s+int\s+ta_cosignal_get\s*\(([^;]*)\);", text).group(1)
    assert tuple(re.findall(r"uint64_t\*\s+(\w+)", get)) == _capi.COSIGNAL_COLUMNS == ref.COLUMNS


def test_the_constants_of_the_kernel_header():
    text = open(os.path.join(ROOT, "tissue_analysis_amd", "csrc", "ta_cosignal.h")).read()
    assert int(re.search(r"COSIG_SLOTS\s*=\s*(\d+)", text).group(1)) == _capi.COSIG_SLOTS
    assert int(re.search(r"COSIG_MAX_GROUPS\s*=\s*(\d+)", text).group(1)) == _capi.COSIG_MAX_GROUPS
    assert 4 * 76 * _capi.COSIG_SLOTS <= 160 * 1024               # four workgroups a CU


def test_library_exports_and_rejects_null():
    lib = _capi.load()
    for name in _capi.COSIGNAL_SYMBOLS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert lib.ta_cosignal_extract(None, 0, 0) == _capi.TA_EINVAL
    assert b"NULL" in lib.ta_last_error()
    assert lib.ta_cosignal_set(None, None, 1, None, None) == _capi.TA_EINVAL
    assert lib.ta_cosignal_set_device(None, None, 1) == _capi.TA_EINVAL
    assert lib.ta_cosignal_get(*([None] * 12)) == _capi.TA_EINVAL
    out = (ctypes.c_uint32 * 4)()
    assert lib.ta_cosignal_debug(None, out) == _capi.TA_EINVAL and list(out) == [0, 0, 0, 0]
    ms = ctypes.c_double(-1.0)
    assert lib.ta_cosignal_timing(None, ctypes.byref(ms)) == _capi.TA_EINVAL and ms.value == -1.0
    assert lib.ta_cosignal_thresholds(None, None, None) == _capi.TA_EINVAL


# ---- the reference against a brute loop ---------------------------------------------------------------------------------------------
def brute(V, A, B, nrows, thr_a, thr_b, first_owned=0):
    out = dict((k, [0] * nrows) for k in ref.COLUMNS)
    for v, a, b in zip(V[first_owned:].reshape(-1).tolist(), A[first_owned:].reshape(-1).tolist(), B[first_owned:].reshape(-1).tolist()):
        ia, ib = a > thr_a, b > thr_b
        for k, add in (("n", 1), ("sum_a", a), ("sum_b", b), ("sq_aa", a * a), ("sq_bb", b * b), ("sq_ab", a * b), ("n_a", int(ia)),
                       ("n_b", int(ib)), ("n_ab", int(ia and ib)), ("sum_a_over", a if ib else 0), ("sum_b_over", b if ia else 0)):
            out[k][v] += add
    return out


@pytest.mark.parametrize("adt,bdt,thr", [(np.uint16, np.uint16, (30000, 20000)), (np.uint8, np.uint16, (0, 65535)),
                                         (np.uint16, np.uint8, (300, 300)), (np.uint8, np.uint8, (0, 0))])
def test_reference_against_a_brute_loop(adt, bdt, thr):
    rng = np.random.default_rng(3)
    V = rng.integers(0, 9, size=(5, 6, 7)).astype(np.uint16)
    A = rng.integers(0, np.iinfo(adt).max, size=V.shape, endpoint=True).astype(adt)
    B = rng.integers(0, np.iinfo(bdt).max, size=V.shape, endpoint=True).astype(bdt)
    for first_owned in (0, 1):
        got, want = ref.labels(V, A, B, 11, thr[0], thr[1], first_owned=first_owned), brute(V, A, B, 11, thr[0], thr[1], first_owned)
        for k in ref.COLUMNS:
            if k in ref.WIDE:
                assert got[k + "_int"] == want[k], k
                assert [(int(hi) << 64) | int(lo) for lo, hi in got[k].tolist()] == want[k], k
            else:
                assert got[k].dtype == np.uint64 and got[k].tolist() == want[k], k
        assert int(got["n"].sum()) == V[first_owned:].size and not got["n"][9:].any()
    if thr == (300, 300):                                          # above a uint8 channel's largest value: nothing is over in it
        assert not got["n_b"].any() and not got["n_ab"].any() and not got["sum_a_over"].any() and got["n_a"].any()


# ---- ChannelPairStats from reference integers ---------------------------------------------------------------------------------------
def stats_of(V, A, B, nrows, thr=(0, 0)):
    cols = ref.labels(V, A, B, nrows, *thr)
    return ChannelPairStats(None, cols, thr), cols


def cells(sizes):
    """One label per entry of sizes, label k holding sizes[k] voxels, as a (1, 1, n) volume."""
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.uint32).reshape(1, 1, -1)


def test_pearson_against_numpy_corrcoef():
    rng = np.random.default_rng(11)
    sizes = [2, 3, 7, 50, 1000, 50000, 2, 40, 5000, 300]
    V = cells(sizes)
    n = V.size
    base = rng.integers(0, 65535, size=n, endpoint=True)
    kinds = rng.integers(0, 4, size=len(sizes))
    A = base.copy()
    B = rng.integers(0, 65535, size=n, endpoint=True)
    start = np.concatenate([[0], np.cumsum(sizes)])
    for k, kind in enumerate(kinds.tolist()):
        s = slice(start[k], start[k + 1])
        noise = rng.integers(-200, 200, size=sizes[k], endpoint=True)
        if kind == 1:                                              # correlated
            B[s] = np.clip(base[s] // 2 + 1000 + noise, 0, 65535)
        elif kind == 2:                                            # anti-correlated
            B[s] = np.clip(60000 - base[s] // 2 + noise, 0, 65535)
        elif kind == 3:                                            # near-constant: one voxel differs by one
            B[s] = 41234
            B[start[k]] = 41235
    A, B = A.astype(np.uint16).reshape(V.shape), B.astype(np.uint16).reshape(V.shape)
    st, cols = stats_of(V, A, B, len(sizes))
    got = st.pearson()
    worst = 0.0
    for k in range(len(sizes)):
        s = slice(start[k], start[k + 1])
        want = np.corrcoef(A.reshape(-1)[s].astype(np.float64), B.reshape(-1)[s].astype(np.float64))[0, 1]
        worst = max(worst, abs(got[k] - want))
    print("worst |pearson - corrcoef| =", worst)
    assert worst <= 1e-12
    f = ref.floats(cols)
    np.testing.assert_allclose(got, f["pearson"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(st.covariance(), f["covariance"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(st.ratio(), f["ratio"], rtol=1e-12, atol=0)


def test_pearson_is_exactly_one_for_b_equal_a_and_minus_one_for_its_complement():
    rng = np.random.default_rng(12)
    sizes = [2, 3, 17, 999, 50000]
    V = cells(sizes)
    A = rng.integers(0, 65535, size=V.shape, endpoint=True).astype(np.uint16)
    A[0, 0, :2] = (0, 65535)
    same, _ = stats_of(V, A, A, len(sizes))
    assert same.pearson().tolist() == [1.0] * len(sizes)
    assert same.overlap_coefficient().tolist() == [1.0] * len(sizes)
    assert np.array_equal(same.ratio(), np.ones(len(sizes)))
    comp, _ = stats_of(V, A, (65535 - A).astype(np.uint16), len(sizes))
    assert comp.pearson().tolist() == [-1.0] * len(sizes)


def test_nan_rules():
    V = np.array([0, 1, 1, 2, 2, 2, 3, 3, 5, 5], dtype=np.uint16).reshape(1, 1, -1)
    A = np.array([7, 4, 9, 5, 5, 5, 0, 0, 1, 2], dtype=np.uint8).reshape(V.shape)
    B = np.array([3, 8, 2, 1, 6, 9, 0, 0, 0, 0], dtype=np.uint8).reshape(V.shape)
    st, cols = stats_of(V, A, B, 7, (4, 5))
    r = st.pearson()
    assert math.isnan(r[0])                                        # one voxel
    assert r[1] == -1.0                                            # two voxels, not constant
    assert math.isnan(r[2]) and math.isnan(r[3]) and math.isnan(r[5])      # A constant; both constant; B constant
    assert math.isnan(r[4]) and math.isnan(r[6])                   # rows without voxels
    ratio = st.ratio()
    assert ratio[0] == 7 / 3 and ratio[1] == 13 / 10 and math.isnan(ratio[3]) and math.isnan(ratio[5]) and math.isnan(ratio[4])
    assert st.covariance()[0] == 0.0 and math.isnan(st.covariance()[4])
    m1, m2 = st.manders()
    assert m1[1] == 4 / 13 and m2[1] == 2 / 10                     # B > 5 at the voxel with A = 4; A > 4 at the voxel with B = 2
    assert m1[2] == 10 / 15 and m2[2] == 1.0 and math.isnan(m1[3]) and math.isnan(m2[3]) and m1[5] == 0.0 and math.isnan(m2[5])
    j = st.mask_jaccard()
    assert j[1] == 0.0 and j[2] == 2 / 3 and math.isnan(j[3]) and math.isnan(j[5]) and math.isnan(j[4])
    assert math.isnan(st.overlap_coefficient()[3]) and math.isnan(st.overlap_coefficient()[5])
    f = ref.floats(cols)
    for name, got in (("ratio", ratio), ("pearson", r), ("manders_m1", m1), ("manders_m2", m2), ("mask_jaccard", j),
                      ("overlap_coefficient", st.overlap_coefficient()), ("covariance", st.covariance())):
        np.testing.assert_allclose(got, f[name], rtol=1e-12, atol=0, equal_nan=True, err_msg=name)
    # lookups by label: ids without a row are NaN
    got = st.of_labels([2, 99, 1], "manders_m1")
    assert got[0] == m1[2] and math.isnan(got[1]) and got[2] == m1[1]
    with pytest.raises(ValueError):
        st.of_labels([1], "mean")


def test_merge_of_two_slabs_equals_the_whole():
    rng = np.random.default_rng(13)
    V = rng.integers(0, 6, size=(9, 5, 8)).astype(np.uint16)
    A = rng.integers(0, 65535, size=V.shape, endpoint=True).astype(np.uint16)
    B = rng.integers(0, 255, size=V.shape, endpoint=True).astype(np.uint8)
    thr = (20000, 100)
    whole, _ = stats_of(V, A, B, 6, thr)
    low = ChannelPairStats(None, ref.labels(V[:4], A[:4], B[:4], 6, *thr), thr)
    high = ChannelPairStats(None, ref.labels(V[3:], A[3:], B[3:], 6, *thr, first_owned=1), thr)      # plane 3 is its halo
    merged = ChannelPairStats.merge([low, high])
    for k in ref.COLUMNS:
        assert np.array_equal(getattr(merged, k), getattr(whole, k)), k
    assert merged.thresholds == thr and np.array_equal(merged.pearson(), whole.pearson(), equal_nan=True)
    with pytest.raises(ValueError):
        ChannelPairStats.merge([low, ChannelPairStats(None, ref.labels(V[3:], A[3:], B[3:], 6, 0, 0), (0, 0))])


def test_sq_int_rebuilds_a_value_above_two_to_the_64():
    n = 1040 * 2048 * 2048                                         # (the volume of the carry test on the device)
    big = n * 65535 * 65535
    assert big >= 2 ** 64
    cols = dict((k, np.zeros(2, dtype=np.uint64)) for k in ref.COLUMNS if k not in ref.WIDE)
    cols["n"][1] = n
    cols["sum_a"][1] = cols["sum_b"][1] = n * 65535
    for k in ref.WIDE:
        cols[k] = ref.words([0, big])
    st = ChannelPairStats(None, cols)
    assert int(st.sq_aa[1, 1]) == big >> 64 > 0
    assert [st.sq_int(k, 1) for k in ref.WIDE] == [big] * 3 and st.sq_int("sq_ab", 0) == 0
    assert st.ratio()[1] == 1.0 and math.isnan(st.pearson()[1]) and st.overlap_coefficient()[1] == 1.0      # both channels constant
    with pytest.raises(ValueError):
        st.sq_int("sum_a", 1)
    merged = ChannelPairStats.merge([st, st])
    assert merged.sq_int("sq_ab", 1) == 2 * big
