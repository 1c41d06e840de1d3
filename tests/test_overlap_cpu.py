"""The label-overlap table without a GPU: the NumPy restatement (tests/overlap_reference.py) against a brute force over voxels,
the host-side derivations of tissue_analysis_amd.label_overlap against the restatement, lineage on a constructed division, and
the C ABI of include/tissue_scan_overlap.h (declarations, exports, NULL-context checks)."""
import ctypes
import os
import re

import numpy as np
import pytest

import overlap_reference as ref
from tissue_analysis_amd import LabelOverlap, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"TA_API\s+(?:const\s+char\s*\*|int)\s+(ta_\w+)\s*\(", text)))


def _volumes():
    rng = np.random.default_rng(20261016)
    for shape, na, nb, da, db in (((6, 7, 9), 5, 4, np.uint16, np.uint16), ((3, 11, 4), 30, 7, np.uint32, np.uint16),
                                  ((9, 1, 13), 3, 40, np.uint16, np.uint32), ((5, 5, 1), 4, 4, np.uint32, np.uint32)):
        yield rng.integers(0, na, size=shape).astype(da), rng.integers(0, nb, size=shape).astype(db)
    ids = np.array([0, 7, 70000, 2**31 + 5, 2**32 - 2, 2**32 - 1], dtype=np.uint32)
    yield ids[rng.integers(0, ids.size, size=(4, 5, 6))], ids[rng.integers(0, ids.size, size=(4, 5, 6))]


def _brute(A, B):
    tot = {}
    for x, y in zip(A.reshape(-1).tolist(), B.reshape(-1).tolist()):
        tot[(x, y)] = tot.get((x, y), 0) + 1
    return tot


def test_restatement_equals_a_brute_force_over_voxels():
    for A, B in _volumes():
        a, b, n = ref.table(A, B)
        tot = _brute(A, B)
        assert list(zip(a.tolist(), b.tolist())) == sorted(tot)
        assert n.tolist() == [tot[k] for k in sorted(tot)]
        assert n.dtype == np.uint64 and int(n.sum()) == A.size


def test_margins_equal_bincount():
    for A, B in _volumes():
        if max(int(A.max()), int(B.max())) > 10**6:
            continue
        a, b, n = ref.table(A, B)
        sa, sb = ref.margins(a, b, n)
        ca, cb = np.bincount(A.reshape(-1).astype(np.int64)), np.bincount(B.reshape(-1).astype(np.int64))
        assert sa == dict((int(l), int(c)) for l, c in enumerate(ca) if c)
        assert sb == dict((int(l), int(c)) for l, c in enumerate(cb) if c)
        ov = LabelOverlap(a, b, n)
        ids, tot = ov.size_a
        assert np.array_equal(ids, np.flatnonzero(ca)) and np.array_equal(tot, ca[ca > 0].astype(np.uint64))
        ids, tot = ov.size_b
        assert np.array_equal(ids, np.flatnonzero(cb)) and np.array_equal(tot, cb[cb > 0].astype(np.uint64))


def check_derived(ov, a, b, n):
    """Everything LabelOverlap derives on the host against the restatement, for the table (a, b, n)."""
    assert len(ov) == a.size
    assert ov.a.dtype == np.int64 and ov.b.dtype == np.int64 and ov.n.dtype == np.uint64
    assert np.array_equal(ov.a, a) and np.array_equal(ov.b, b) and np.array_equal(ov.n, n)
    sa, sb = ref.margins(a, b, n)
    assert dict(zip(ov.size_a[0].tolist(), ov.size_a[1].tolist())) == sa
    assert dict(zip(ov.size_b[0].tolist(), ov.size_b[1].tolist())) == sb
    assert np.array_equal(ov.jaccard(), ref.jaccard(a, b, n))
    for side in ("a", "b"):
        for exclude in ((), (0,), (0, 1)):
            labels, partners, cnt = ov.best_match(side, exclude)
            assert dict(zip(labels.tolist(), zip(partners.tolist(), cnt.tolist()))) == ref.best_match(a, b, n, side, exclude)
            assert np.array_equal(labels, np.sort(labels))
    for frac in (0.0, 0.5, 0.9):
        for exclude in ((), (0,), (0, 1)):
            assert ov.lineage(frac, exclude) == ref.lineage(a, b, n, frac, exclude)
    for i in range(0, a.size, max(1, a.size // 7)):
        assert ov.between(a[i], b[i]) == int(n[i])
    for x, y in ((int(a[0]), int(b[-1])), (12345, 3), (int(a[-1]), 54321)):
        assert ov.between(x, y) == ref_between(a, b, n, x, y)


def ref_between(a, b, n, x, y):
    hit = np.flatnonzero((a == x) & (b == y))
    return int(n[hit[0]]) if hit.size else 0


def test_label_overlap_derivations_equal_the_restatement():
    for A, B in _volumes():
        a, b, n = ref.table(A, B)
        check_derived(LabelOverlap(a, b, n), a, b, n)


def test_tie_rule_and_exclude_on_a_hand_made_table():
    # b = 5 meets 2, 3 and 9 with 4 voxels each and 1 (excluded below) with 6; b = 6 only meets the excluded 1
    a = np.array([1, 1, 2, 3, 3, 9], dtype=np.int64)
    b = np.array([5, 6, 5, 5, 7, 5], dtype=np.int64)
    n = np.array([6, 2, 4, 4, 10, 4], dtype=np.uint64)
    ov = LabelOverlap(a, b, n)
    labels, partners, cnt = ov.best_match("b")
    assert labels.tolist() == [5, 6, 7] and partners.tolist() == [1, 1, 3] and cnt.tolist() == [6, 2, 10]
    labels, partners, cnt = ov.best_match("b", exclude=(1,))
    assert labels.tolist() == [5, 7] and partners.tolist() == [2, 3] and cnt.tolist() == [4, 10]        # the tie goes to 2
    labels, partners, cnt = ov.best_match("a")
    assert labels.tolist() == [1, 2, 3, 9] and partners.tolist() == [5, 5, 7, 5]
    # |5| = 18: 4 of 18 is below one half, 4 >= 0.2 * 18; 7 lies wholly in 3
    assert ov.lineage(0.5, exclude=(1,)) == {3: [7]}
    assert ov.lineage(0.2, exclude=(1,)) == {2: [5], 3: [7]}
    assert ov.lineage(0.0, exclude=()) == {1: [5, 6], 3: [7]}
    assert ov.lineage(0.0, exclude=(5,)) == {1: [6], 3: [7]}             # an excluded daughter
    assert ov.between(3, 7) == 10 and ov.between(3, 6) == 0 and ov.between(4, 5) == 0
    j = ov.jaccard()
    assert j[4] == 10.0 / (14 + 10 - 10) and j[0] == 6.0 / (8 + 18 - 6)
    check_derived(ov, a, b, n)


def test_lineage_recovers_every_mother_of_a_constructed_division():
    A, B, truth = ref.division_fixture()
    a, b, n = ref.table(A, B)
    assert len(truth) == 222 and a.size == 223
    ov = LabelOverlap(a, b, n)
    for lin in (ov.lineage(0.5, exclude=(0, 1)), ref.lineage(a, b, n, 0.5, (0, 1))):
        got = dict((d, m) for m, ds in lin.items() for d in ds)
        assert got == truth                         # every label of B, none left out
    check_derived(ov, a, b, n)


def test_shifted_frames_agree_with_the_restatement():
    A, B, _ = ref.division_fixture()
    Bs = ref.shifted(B, (1, 2, 1))
    a, b, n = ref.table(A, Bs)
    check_derived(LabelOverlap(a, b, n), a, b, n)


def test_slab_tables_merge_to_the_whole():
    for A, B in _volumes():
        if A.shape[0] < 4:
            continue
        whole = ref.table(A, B)
        for cuts in ((A.shape[0] // 2,), (1, 3)):
            edges = (0,) + cuts + (A.shape[0],)
            parts = [ref.table(A[:edges[1]], B[:edges[1]])]
            parts += [ref.table(A[lo - 1:hi], B[lo - 1:hi], first_owned=1) for lo, hi in zip(edges[1:-1], edges[2:])]
            for got, want in zip(ref.merge(parts), whole):
                assert np.array_equal(got, want)


def test_overlap_header_and_binding_agree():
    assert declared_symbols("tissue_scan_overlap.h") == sorted(_capi.OVERLAP_SYMBOLS)
    needed = {"ta_overlap_set", "ta_overlap_set_device", "ta_overlap_extract", "ta_overlap_size", "ta_overlap_get", "ta_overlap_timing"}
    assert needed <= set(_capi.OVERLAP_SYMBOLS)


def test_overlap_symbols_are_apart_from_the_other_lists_and_the_core_header_is_unchanged():
    assert not set(_capi.OVERLAP_SYMBOLS) & (set(_capi.SYMBOLS) | set(_capi.SIGNAL_SYMBOLS) | set(_capi.MESH_SYMBOLS))
    assert declared_symbols("tissue_scan.h") == sorted(_capi.SYMBOLS)
    assert _capi.ABI_VERSION == 5 and "#define TA_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "tissue_scan.h")).read()


def test_library_exports_the_overlap_symbols_and_they_reject_a_null_context():
    lib = _capi.load()
    i64 = (ctypes.c_int64 * 3)(4, 4, 4)
    buf = (ctypes.c_uint64 * 64)()
    dbl = ctypes.c_double(0)
    u64 = ctypes.c_uint64(0)
    calls = {
        "ta_overlap_set": (None, buf, 2, i64, None),
        "ta_overlap_set_device": (None, buf, 2),
        "ta_overlap_set_capacity": (None, 0),
        "ta_overlap_extract": (None,),
        "ta_overlap_size": (None, ctypes.byref(u64)),
        "ta_overlap_get": (None, buf, buf, buf),
        "ta_overlap_timing": (None, ctypes.byref(dbl)),
        "ta_overlap_timing_compaction": (None, ctypes.byref(dbl), None),
        "ta_overlap_debug": (None, (ctypes.c_uint32 * 4)()),
    }
    assert sorted(calls) == sorted(_capi.OVERLAP_SYMBOLS)
    for name in declared_symbols("tissue_scan_overlap.h"):
        assert hasattr(lib, name), name
        assert getattr(lib, name)(*calls[name]) == _capi.TA_EINVAL, name
        err = lib.ta_last_error()
        assert b"NULL" in err or b"ctx" in err, (name, err)


def test_second_volume_is_checked_before_any_device_work():
    ctx = _capi.Context.__new__(_capi.Context)          # (no GPU needed: the checks run before the C call)
    ctx._vol_layout = ((4, 4, 4), (16, 4, 1))
    with pytest.raises(TypeError, match="uint16 or uint32"):
        _capi.Context.set_overlap(ctx, np.zeros((4, 4, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        _capi.Context.set_overlap(ctx, np.zeros((4, 4, 5), dtype=np.uint16))
