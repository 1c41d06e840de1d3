"""Signal-weighted moments without a GPU: include/tissue_scan_sigmoments.h against the binding and the library, `SignalMoments`
from hand-made integer rows, the restated launch plan with its exactness cap, and the NumPy reference of
tests/sigmoment_reference.py against scipy."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import range_tiles
import sigmoment_reference as ref
from tissue_analysis_amd import SignalMoments, _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- header, binding, library ---------------------------------------------------------------------------------------------------
def header():
    return open(os.path.join(ROOT, "include", "tissue_scan_sigmoments.h")).read()


def test_header_and_binding_agree():
    text = header()
    declared = sorted(set(re.findall(r"TA_API\s+int\s+(ta_\w+)\s*\(", text)))
    assert declared == sorted(_capi.SIGMOM_SYMBOLS) and len(declared) == 4
    assert not set(_capi.SIGMOM_SYMBOLS) & set(_capi.SYMBOLS)
    assert re.search(r"TA_API\s+int\s+ta_sigmom_debug\s*\(ta_ctx\*\s*ctx,\s*uint32_t\s+out\[4\]\)", text)
    lib = _capi.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.ta_version() == _capi.ABI_VERSION == 5


def test_constants_agree():
    kernel_header = open(os.path.join(ROOT, "tissue_analysis_amd", "csrc", "ta_sigmoments.h")).read()
    assert int(re.search(r"SM_SLOTS\s*=\s*(\d+)", kernel_header).group(1)) == _capi.SIGMOM_SLOTS == ref.LABEL_SLOTS
    assert int(re.search(r"SM_MAX_GROUPS\s*=\s*(\d+)", kernel_header).group(1)) == _capi.SIGMOM_MAX_GROUPS == ref.MAX_GROUPS
    assert 4 * 88 * ref.LABEL_SLOTS <= 160 * 1024             # four workgroups of 88-byte rows in a CU's LDS


def test_a_null_context_is_refused_without_a_gpu():
    lib = _capi.load()
    assert lib.ta_sigmom_extract(None) == _capi.TA_EINVAL
    assert b"NULL" in lib.ta_last_error()
    assert lib.ta_sigmom_get(None, None, None, None, None) == _capi.TA_EINVAL
    out = (ctypes.c_uint32 * 4)()
    assert lib.ta_sigmom_debug(None, out) == _capi.TA_EINVAL and list(out) == [0, 0, 0, 0]
    ms = ctypes.c_double(-1.0)
    assert lib.ta_sigmom_timing(None, ctypes.byref(ms)) == _capi.TA_EINVAL and ms.value == -1.0


# ---- SignalMoments from hand-made rows --------------------------------------------------------------------------------------------
def _geometry(V, nrows):
    """count, sum1, sum2 of a label image as the sweep gives them (array axes), from the reference with a signal of ones."""
    g = ref.rows(V, np.ones(V.shape, dtype=np.uint8), nrows)
    def rows_of(labels, missing=None):                        # (dense rows, as Extraction.rows_of answers)
        idx = np.asarray(labels, dtype=np.int64)
        return idx if missing is None else np.where((idx >= 0) & (idx < nrows), idx, missing)
    return types.SimpleNamespace(count=g["n"], sum1=g["m1"], sum2=g["m2_words"][:, :, 0], ids=None, rows_of=rows_of)


def _moments(V, S, nrows, **kw):
    r = ref.rows(V, S, nrows)
    return SignalMoments(_geometry(V, nrows), r["n"], r["w"], r["m1"], r["m2_words"], **kw), r


def _blocks():
    return range_tiles.block_labels((9, 14, 11), np.uint16, 3, nlabels=5)


def test_a_uniform_signal_sits_at_the_barycentre():
    V = _blocks()
    vs = (0.5, 2.0, 1.25)
    m, _ = _moments(V, np.full(V.shape, 7, dtype=np.uint8), 6, voxelsize=vs)
    g = m.extraction
    present = g.count > 0
    assert not present[0] and present[1:].any()
    with np.errstate(invalid="ignore"):
        bary = g.sum1.astype(np.float64) / g.count.astype(np.float64)[:, None]
    np.testing.assert_allclose(m.centroid(real=False)[present], bary[present], rtol=1e-15)
    np.testing.assert_allclose(m.centroid()[present], (bary * vs)[present], rtol=1e-15)
    assert (m.polarity()[present] == 0).all() and (m.polarity(normalised=True)[present] == 0).all()
    assert (m.polarity_index()[present] == 0).all()
    # the covariance is the geometric one: (n sum2 - sum1 sum1^T) / n^2
    cov = m.covariance(real=False)
    for r in np.flatnonzero(present):
        n = float(g.count[r])
        for k, (j, i) in enumerate(ref.PAIR_ORDER):
            want = (int(g.count[r]) * int(g.sum2[r, k]) - int(g.sum1[r, j]) * int(g.sum1[r, i])) / (n * n)
            assert cov[r, j, i] == pytest.approx(want, rel=1e-14) and cov[r, i, j] == cov[r, j, i]
    gyr = m.gyration_radius(real=False)
    np.testing.assert_allclose(gyr[present] ** 2, np.trace(cov, axis1=1, axis2=2)[present], rtol=1e-12)


def test_all_signal_in_one_voxel():
    V = np.full((5, 6, 7), 2, dtype=np.uint16)
    S = np.zeros(V.shape, dtype=np.uint16)
    S[3, 1, 5] = 40000
    m, _ = _moments(V, S, 3, voxelsize=(1.0, 2.0, 3.0))
    assert m.centroid(real=False)[2].tolist() == [3.0, 1.0, 5.0] and m.centroid()[2].tolist() == [3.0, 2.0, 15.0]
    assert (m.covariance()[2] == 0).all()
    vecs, vals = m.inertia_axis()
    assert (vals[2] == 0).all() and np.isfinite(vecs[2]).all()
    np.testing.assert_allclose(m.polarity(real=False)[2], [3 - 2.0, 1 - 2.5, 5 - 3.0], rtol=1e-15)


def test_rows_without_signal_are_nan():
    V = np.full((3, 3, 3), 1, dtype=np.uint16)
    V[0] = 2
    S = np.where(V == 1, 9, 0).astype(np.uint8)               # label 2 has voxels but no signal, row 0 has neither
    m, _ = _moments(V, S, 3)
    for r in (0, 2):
        assert np.isnan(m.centroid()[r]).all() and np.isnan(m.covariance()[r]).all() and np.isnan(m.polarity()[r]).all()
        assert np.isnan(m.inertia_axis()[1][r]).all()
    assert np.isfinite(m.centroid()[1]).all() and np.isfinite(m.inertia_axis()[0][1]).all()
    assert np.isnan(m.of_labels([1, 7], "centroid")[1]).all()


def test_inertia_axes_of_a_bar_along_one_axis():
    V = np.ones((4, 30, 3), dtype=np.uint16)
    S = np.zeros(V.shape, dtype=np.uint8)
    S[1, :, 1] = 200                                          # a line of signal along array axis 1
    m, _ = _moments(V, S, 2)
    vecs, vals = m.inertia_axis(real=False)
    assert vals[1, 0] == pytest.approx((30 ** 2 - 1) / 12.0, rel=1e-14) and abs(vals[1, 1]) < 1e-12 and abs(vals[1, 2]) < 1e-12
    assert abs(vecs[1, 0]).tolist() == [0.0, 1.0, 0.0]
    # the same image stored with its axes permuted: perm carries memory axis k to its array axis
    perm = (2, 0, 1)
    r = ref.rows(V.transpose(perm), S.transpose(perm), 2)
    p = SignalMoments(m.extraction, r["n"], r["w"], r["m1"], r["m2_words"], perm=perm)
    assert np.array_equal(p.centroid(), m.centroid(), equal_nan=True) and np.array_equal(p.covariance(), m.covariance(), equal_nan=True)
    assert np.array_equal(p.polarity(), m.polarity(), equal_nan=True)


def test_shift_and_merge_of_two_halves_is_exact():
    rng = np.random.default_rng(11)
    V = range_tiles.block_labels((12, 10, 9), np.uint16, 5, nlabels=6)
    S = rng.integers(0, 65535, size=V.shape, endpoint=True).astype(np.uint16)
    origin, cut = 1 << 24, 7
    whole = ref.shifted(ref.rows(V, S, 7), origin)            # the volume sits at plane 2^24 of a taller one
    parts = []
    for lo, hi in ((0, cut), (cut, V.shape[0])):
        r = ref.rows(V[lo:hi], S[lo:hi], 7)                   # local coordinates, as a slab context gives them
        parts.append(SignalMoments(None, r["n"], r["w"], r["m1"], r["m2_words"], origin0=origin + lo))
    merged = SignalMoments.merge(parts)
    assert merged.origin0 == 0
    for a in (merged.n, merged.w, merged.m1, merged.m2):
        assert a.dtype == np.uint64                           # no float entered
    assert merged.n.tolist() == whole["n"].tolist() and merged.w.tolist() == whole["w"].tolist()
    assert merged.m1.tolist() == whole["m1"].tolist()
    assert [merged.m2_int(r) for r in range(7)] == whole["m2"].tolist()
    assert max(max(merged.m2_int(r)) for r in range(7)) > 1 << 64
    # shifting back gives the local rows of the whole volume again
    back = merged.shifted(origin)
    local = ref.rows(V, S, 7)
    assert back.origin0 == origin and back.m1.tolist() == local["m1"].tolist() and np.array_equal(back.m2, local["m2_words"])
    np.testing.assert_allclose(back.centroid(real=False)[1:, 0] - origin, local["m1"][1:, 0] / local["w"][1:], rtol=1e-9)
    with pytest.raises(OverflowError):
        merged.shifted(-(1 << 62))
    with pytest.raises(ValueError):
        back.polarity()


def test_second_moments_above_64_bits_give_the_right_covariance():
    """One cell, two voxels a large distance apart at a large offset: m2 needs the high word, the covariance is (d / 2)^2."""
    base, d, s = 1 << 26, 1000, 65535
    n, w = np.array([2], dtype=np.uint64), np.array([2 * s], dtype=np.uint64)
    m1 = np.array([[s * (2 * base + d), 0, 0]], dtype=np.uint64)
    q00 = s * (base * base + (base + d) * (base + d))
    assert q00 > 1 << 64
    m2 = np.zeros((1, 6, 2), dtype=np.uint64)
    m2[0, 0] = (q00 & ((1 << 64) - 1), q00 >> 64)
    m = SignalMoments(None, n, w, m1, m2)
    assert m.m2_int(0)[0] == q00
    assert m.covariance()[0, 0, 0] == (d / 2.0) ** 2 and not m.covariance()[0, 1:, :].any()
    assert m.centroid()[0].tolist() == [base + d / 2.0, 0.0, 0.0]


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def test_the_exactness_cap_does_not_bind_on_the_workloads():
    for name in ("C4", "C5"):
        c = synth.CONFIGS[name]
        for sig in (1, 2):
            p = ref.plan(c["dims"], 0, np.dtype(c["dtype"]).itemsize, sig)
            base = range_tiles.plan(c["dims"], 0, np.dtype(c["dtype"]).itemsize, "signal")
            assert p.per == p.uncapped == base.per and p.groups == base.groups and p.most > p.per
            assert ref.first_moments_fit(c["dims"], sig)
    # the header's figure: 6.7e7 voxels a workgroup at 2048^3 with a uint16 signal
    assert (1 << 64) // (2047 ** 2 * 65535) == pytest.approx(6.7e7, rel=0.01)
    for case in range_tiles.CASES:                            # nor on the range shapes
        p = ref.plan(case.dims, case.first_owned, case.dtype.itemsize, 2)
        assert p[:7] == tuple(range_tiles.plan(case.dims, case.first_owned, case.dtype.itemsize, "signal"))


def test_the_exactness_cap_at_its_limit_shapes():
    # the carry shape: the cap is 2 tiles, the plan asks for 1
    p = ref.plan((4, 4, 65536), 0, 2, 2)
    assert (p.tiles, p.most, p.uncapped, p.per, p.groups) == (128, 2, 1, 1, 128)
    # the clamp shape: 1152 tiles would go 2 a workgroup; 29128 voxels are less than 2 tiles of 16384
    assert (1 << 64) // (98303 ** 2 * 65535) == 29128
    p = ref.plan((1, 12, 98304), 0, 4, 2)
    assert (p.tiles, p.uncapped, p.most, p.per, p.groups, p.tiles_in_last_group) == (1152, 2, 1, 1, 1152, 1)
    assert ref.plan((1, 12, 98304), 0, 4, 1).per == 2         # a uint8 signal leaves room
    # an axis of 2^20 with a uint16 signal: not one tile fits
    for dims in ((1 << 20, 8, 8), (1, 1, (1 << 20) + 8)):
        for itemsize in (2, 4):
            p = ref.plan(dims, 0, itemsize, 2)
            assert p.most == 0 and p.per == 0 and p.groups == 0
    assert ref.plan((1, 1, (1 << 20) + 8), 0, 4, 1).most > 0
    assert ref.first_moments_fit((2048, 2048, 2048), 2) and not ref.first_moments_fit((1 << 14, 1 << 14, 1 << 14), 2)


def test_spill_bound_of_the_permutation_volumes():
    V = range_tiles.permutation_labels(range_tiles.SPILL_DIMS, np.uint16, 1)
    assert ref.plan(V.shape, 0, 2, 2).groups == 1 and ref.label_spill_bound(V, 0, 2) == V.size - ref.LABEL_SLOTS
    W = range_tiles.permutation_labels(range_tiles.SPILL_DIMS_WIDE, np.uint32, 2)
    assert ref.label_spill_bound(W, 0, 2) > 0


# ---- the reference against scipy ------------------------------------------------------------------------------------------------
def test_reference_against_scipy_center_of_mass():
    from scipy import ndimage
    c = synth.CONFIGS["C1"]
    V = synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], np.uint16)
    S = np.random.default_rng(21).integers(0, 65535, size=V.shape, endpoint=True).astype(np.uint16)
    L = int(V.max())
    r = ref.rows(V, S, L + 1)
    ids = np.flatnonzero(r["w"] > 0)
    want = np.asarray(ndimage.center_of_mass(S, V, ids))
    g = types.SimpleNamespace(count=r["n"], sum1=ref.rows(V, np.ones(V.shape, np.uint8), L + 1)["m1"])
    f = ref.floats(r, g)
    np.testing.assert_allclose(f["centroid"][ids], want, rtol=1e-6)
    m = SignalMoments(None, r["n"], r["w"], r["m1"], r["m2_words"])
    np.testing.assert_allclose(m.centroid(real=False), f["centroid"], rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(m.covariance(real=False), f["covariance"], rtol=1e-12, equal_nan=True)
    # covariance against a direct weighted computation of one cell
    l = int(ids[len(ids) // 2])
    pos = np.argwhere(V == l).astype(np.float64)
    wt = S[V == l].astype(np.float64)
    mu = (pos * wt[:, None]).sum(0) / wt.sum()
    direct = ((pos - mu).T * wt) @ (pos - mu) / wt.sum()
    np.testing.assert_allclose(f["covariance"][l], direct, rtol=1e-9)
