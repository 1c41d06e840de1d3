"""The references of the nearest-label maps against each other, the host side of the feature (NearestLabels on injected arrays), and
the C ABI of include/tissue_scan_nearest.h as far as it goes without a GPU."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import nearest_cases as cases
import nearest_reference as ref
from tissue_analysis_amd import NearestLabels, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DYADIC = [(1.0, 1.0, 1.0), (0.5, 1.0, 2.0), (2.0, 0.25, 1.0)]
OTHER = (0.3, 0.7, 1.1)


def volumes():
    rng = np.random.default_rng(21)
    for shape in ((6, 7, 9), (1, 9, 40), (5, 1, 33), (1, 1, 50), (9, 8, 7)):
        for labels in (5, 12):
            yield (rng.integers(1, labels + 1, shape) * (rng.random(shape) < 0.5)).astype(np.uint16)


def test_references_agree():
    tie_volumes = 0
    for V in volumes():
        for not_from in (None, 1):
            for spacing in DYADIC:
                n, d2, ties = ref.brute(V, 0, spacing, not_from, ties=True)
                m, e2 = ref.by_label_edt(V, 0, spacing, not_from)
                assert n.dtype == m.dtype == np.uint32 and np.array_equal(n, m) and np.array_equal(d2, e2), (V.shape, spacing)
                tie_volumes += bool(ties.any())
            n, d2 = ref.brute(V, 0, OTHER, not_from)
            m, e2, (ids, stack) = ref.by_label_edt(V, 0, OTHER, not_from, per_label=True)
            assert np.all(np.abs(d2 - e2) <= 1e-12 * e2)
            own = np.take_along_axis(stack, np.searchsorted(ids, n)[None], axis=0)[0]       # the chosen label's own distance
            assert np.all(own <= e2 * (1 + 1e-12))
    assert tie_volumes > 20


def test_reference_known_values():
    V = np.array([[[3, 0, 0, 0, 2, 0, 1]]])
    n, d2, ties = ref.brute(V, 0, (1, 1, 0.5), ties=True)
    assert n[0, 0].tolist() == [3, 3, 2, 2, 2, 1, 1] and d2[0, 0].tolist() == [0, 0.25, 1, 0.25, 0, 0.25, 0]
    assert ties[0, 0].tolist() == [False, False, True, False, False, True, False]          # the smaller label wins both ties
    n, d2 = ref.brute(V, 0, (1, 1, 1), not_from=2)
    assert n[0, 0].tolist() == [3, 3, 3, 1, 1, 1, 1] and d2[0, 0].tolist() == [0, 1, 4, 9, 4, 1, 0]
    image, gained, filled, left = ref.result(V, n, d2, 0, 1.0)
    assert image[0, 0].tolist() == [3, 3, 0, 0, 2, 1, 1] and gained.tolist() == [0, 1, 0, 1] and (filled, left) == (2, 2)
    n, d2 = ref.by_label_edt(np.zeros((2, 3, 4), dtype=np.uint16))
    assert (n == ref.NONE).all() and np.isinf(d2).all()
    image, gained, filled, left = ref.result(np.zeros((2, 3, 4), dtype=np.uint16), n, d2)
    assert not image.any() and gained.tolist() == [0] and (filled, left) == (0, 24)          # without a site nothing is filled
    n, d2 = ref.brute(V, 9)                                                                 # an empty label the volume does not hold
    assert np.array_equal(n, V) and (d2 == 0).all()


# ---- the reference by sites, and the cases of test_gpu_nearest_ties.py ------------------------------------------------------------
def test_brute_sites_is_brute():
    tie_volumes = 0
    for V in volumes():
        for not_from in (None, 1):
            for spacing in DYADIC:
                n, d2, ties = ref.brute(V, 0, spacing, not_from, ties=True)
                m, e2, ways = ref.brute_sites(V, 0, spacing, not_from, budget=1 << 14)          # several planes, and one, at a time
                assert m.dtype == np.uint32 and e2.dtype == np.float64 and np.array_equal(n, m) and np.array_equal(d2, e2)
                assert ways.shape == V.shape and np.array_equal(ways >= 2, ties) and (ways >= 1).all()
                tie_volumes += bool(ties.any())
    assert tie_volumes > 20
    V = np.array([[[3, 0, 0, 0, 2, 0, 1, 0, 3]]])
    n, d2, ways = ref.brute_sites(V, 0, (1, 1, 0.5))
    assert n[0, 0].tolist() == [3, 3, 2, 2, 2, 1, 1, 1, 3] and ways[0, 0].tolist() == [1, 1, 2, 1, 1, 2, 1, 2, 1]
    n, d2, ways = ref.brute_sites(np.array([[[4, 0, 4, 0, 2]]]), 0)                            # two sites of one label are one way
    assert n[0, 0].tolist() == [4, 4, 4, 2, 2] and ways[0, 0].tolist() == [1, 1, 1, 2, 1]
    n, d2, ways = ref.brute_sites(np.zeros((2, 3, 4), dtype=np.uint16))
    assert (n == ref.NONE).all() and np.isinf(d2).all() and not ways.any()
    with pytest.raises(AssertionError):
        ref.brute_sites(V, 0, OTHER)


# ways >= 3 per shell: of the spheres at least the 100 asked of them; of the ellipsoids what the reference gives, which is all there is
SHELL_WAYS3 = dict(r9=113, r26=303, r41=387, half20=19, half36=31, mixed80=19, mixed144=23)


@pytest.mark.parametrize("name", list(cases.SHELLS))
def test_shells_hold_the_ties_they_are_built_for_and_the_restated_passes_get_them(name):
    spacing, weights, c, pad, count = cases.SHELLS[name]
    sh = cases.shell(name)
    assert sh.sites.shape == (count, 3) and len(set(map(tuple, sh.sites.tolist()))) == count
    assert all(sum((w * (x - o)) ** 2 for w, x, o in zip(weights, p, sh.centre)) == c for p in sh.sites.tolist())
    every = list(cases.assignments(count))
    assert len(every) == 4 + 2 * count and all(sorted(labels.tolist()) == list(range(1, count + 1)) for _, labels in every)
    assert all(any(labels[j] == 1 for _, labels in every[4:]) for j in range(count))       # the smallest label visits every site
    for k, (_, labels) in enumerate(every):
        V = cases.shell_volume(sh, labels)
        n, d2, ways = ref.brute_sites(V, 0, spacing)
        if k == 0:
            assert ways[sh.centre] == count and d2[sh.centre] == cases.shell_d2(name) and n[sh.centre] == 1
            assert int((ways >= 3).sum()) == SHELL_WAYS3[name] and (name[0] != "r" or SHELL_WAYS3[name] >= 100)
        for perm in cases.shell_layouts(name):
            m, e2 = cases.model(V, perm, spacing)
            assert np.array_equal(n, m) and np.array_equal(d2, e2), (name, k, perm)


def test_off_centre_shells_and_rows_by_the_restated_passes():
    sh = cases.shell("r9")
    for column in cases.OFF_CENTRE_COLUMNS:
        for _, labels in itertools.islice(cases.assignments(30), 4):
            V = cases.shell_volume(sh, labels, np.uint16, cases.OFF_CENTRE_SHAPE, (5, 5, column))
            n, d2, ways = ref.brute_sites(V, 0, cases.UNIT)
            assert ways[5, 5, column] == 30 and (ways[:, :, column - 1:column + 2] >= 2).any(axis=(0, 1)).all()     # ties across a chunk's end
            for perm in cases.PERMS:
                m, e2 = cases.model(V, perm, cases.UNIT)
                assert np.array_equal(n, m) and np.array_equal(d2, e2)
    V = cases.row_carry_rows()
    assert V.shape == (1, 11, 200) and [sorted(r) for r in cases.CARRY_ROWS[:6:2]] == [[60, 68], [1, 127], [3, 189]]
    n, d2, ties = ref.brute(V, 0, cases.ROW_SPACING, ties=True)
    m, e2, ways = ref.brute_sites(V, 0, cases.ROW_SPACING)
    assert np.array_equal(n, m) and np.array_equal(d2, e2) and np.array_equal(ways >= 2, ties)
    assert n[0, :6, 64].tolist() == [2, 2, 3, 3, 4, 8] and ways[0, :6, 64].tolist() == [2, 2, 2, 2, 1, 1]
    assert n[0, 4:6, 96].tolist() == [4, 4] and ways[0, 4:6, 96].tolist() == [2, 2] and d2[0, 4, 96] == 93.0 ** 2
    assert n[0, 6].tolist() == [5] * 200 and n[0, 7].tolist() == [6] * 200 and d2[0, 7, 0] == 199.0 ** 2
    assert n[0, 8, 60:68].tolist() == [11] * 4 + [10] * 4 and n[0, 8, 96] == 10 and n[0, 8, 97] == 12 and ways[0, 8, 96] == 2
    assert (d2[0, 9] >= 256.0 ** 2).all() and np.array_equal(n[0, 10], V[0, 10]) and not d2[0, 10].any()
    for perm in cases.PERMS:
        m, e2 = cases.model(V, perm, cases.ROW_SPACING)
        assert np.array_equal(n, m) and np.array_equal(d2, e2)


RULES = ("chain", "boundary", "previous")


def misses(V, spacing, perms, rule):
    """Voxels at which the restated passes without `rule` give another label than the reference (D2 does not depend on the rules)."""
    n, d2, _ = ref.brute_sites(V, 0, spacing)
    total = 0
    for perm in perms:
        m, e2 = cases.model(V, perm, spacing, **{rule: False})
        assert np.array_equal(d2, e2)
        total += int((n != m).sum())
    return total


@pytest.mark.parametrize("rule", RULES)
def test_every_dropped_tie_rule_is_caught_by_the_shells(rule):
    """A kernel that drops one of the three tie rules gives a wrong label on a shell, in the layouts and with the label assignments
    test_gpu_nearest_ties.py runs.  Measured: every shell catches every rule within its four random assignments."""
    for name in cases.SHELLS:
        spacing = cases.SHELLS[name][0]
        sh = cases.shell(name)
        caught = sum(misses(cases.shell_volume(sh, labels), spacing, cases.shell_layouts(name), rule) > 0
                     for _, labels in itertools.islice(cases.assignments(len(sh.sites)), 4))
        assert caught >= 1, name


def test_the_noise_of_the_parity_test_does_not_catch_a_boundary_label_dropped_on_a_chained_pop():
    """Why the shells exist: `carried = tl` in place of `carried = umin(tl, tb)` in the column kernel passes all five volumes of
    test_gpu_nearest.py::test_parity_with_brute_force in every layout and with every spacing that test uses.  In noise the envelopes
    are two or three entries deep and no boundary label that matters has to outlive a second pop.  The two other rules the noise does catch."""
    import test_gpu_nearest as old
    marks = [m for m in old.test_parity_with_brute_force.pytestmark if m.name == "parametrize" and m.args[0] == "shape,labels"]
    assert len(marks) == 1 and len(marks[0].args[1]) == 5
    caught = dict((rule, 0) for rule in RULES)
    for shape, labels in marks[0].args[1]:
        V = old.noise(shape, labels)
        for spacing in (old.UNIT, old.HALF, old.MIXED):
            caught["chain"] += misses(V, spacing, cases.PERMS, "chain")
        for rule in RULES[1:]:
            caught[rule] += misses(V, old.UNIT, cases.PERMS[:1], rule)
    assert caught["chain"] == 0 and caught["boundary"] > 0 and caught["previous"] > 0


# ---- NearestLabels on host arrays ---------------------------------------------------------------------------------------------
def host_table(V, empty=0, max_distance=None, spacing=(1.0, 1.0, 1.0), **kw):
    n, d2 = ref.by_label_edt(V, empty, spacing)
    max_d2 = np.inf if max_distance is None else max_distance ** 2
    rows = int(V.max()) + 1
    _, gained, filled, left = ref.result(V, n, d2, empty, max_d2, rows)
    return NearestLabels(np.arange(rows), gained, filled, left, empty, None, max_distance, spacing, **kw), (n, d2)


def test_nearest_labels_host_logic():
    V = np.asfortranarray(np.array([[[3, 0, 0, 0, 2, 0, 1], [0, 0, 0, 0, 0, 0, 0]]], dtype=np.uint16))
    applied = []
    nl, (n, d2) = host_table(V, max_distance=1.0, source=lambda: V, images=lambda: (n, d2), apply=lambda: applied.append(1) or "swept")
    assert len(nl) == 4 and nl.filled == 6 and nl.remaining == 5 and nl.max_d2 == 1.0 and nl.ms is None
    assert nl.gained() == {1: 2, 2: 2, 3: 2} and nl.gained_voxels.tolist() == [0, 2, 2, 2]
    assert np.array_equal(nl.nearest(), n) and np.array_equal(nl.distance(), np.sqrt(d2))
    image = nl.image()
    assert image.dtype == V.dtype and image.strides == V.strides
    assert image[0].tolist() == [[3, 3, 0, 2, 2, 1, 1], [3, 0, 0, 0, 2, 0, 1]]
    assert nl.filled_mask().sum() == 6 and V[0, 0].tolist() == [3, 0, 0, 0, 2, 0, 1]      # (the source is left alone)
    assert nl.apply() == "swept" and applied == [1]
    everything, _ = host_table(V, source=lambda: V, images=lambda: (n, d2))
    assert everything.max_d2 == np.inf and everything.remaining == 0 and not (everything.image() == 0).any()
    with pytest.raises(ValueError):
        everything.apply()
    bare, _ = host_table(V)
    for call in (bare.nearest, bare.distance, bare.image, bare.apply):
        with pytest.raises(ValueError):
            call()
    two = NearestLabels([4, 9], [0, 3], 3, 1, voxelsize=(0.5, 0.25), empty=7, not_from=4)
    assert two.voxelsize == (0.5, 0.25, 1.0) and two.gained() == {9: 3} and (two.empty, two.not_from) == (7, 4)


def test_nearest_labels_shape_errors():
    with pytest.raises(ValueError):
        NearestLabels([1, 2], [1], 1, 0)
    with pytest.raises(ValueError):
        NearestLabels([2, 1], [1, 0], 1, 0)
    with pytest.raises(ValueError):
        NearestLabels([1, 2], [1, 1], 3, 0)                # the rows do not sum to the total
    with pytest.raises(ValueError):
        NearestLabels([1], [0], 0, 0, voxelsize=(1.0,))
    with pytest.raises(ValueError):
        NearestLabels([1], [0], 0, 0, max_distance=-1.0).max_d2


def test_analysis_methods_need_a_target():
    from oracle import onepass
    from tissue_analysis_amd import Extraction, SpatialImageAnalysis3D
    V = np.ones((2, 2, 2), dtype=np.uint16)
    with pytest.warns(UserWarning):
        sia = SpatialImageAnalysis3D(V, extraction=Extraction.from_arrays(V.shape, onepass.extract(V)))
    with pytest.raises(ValueError, match="background"):
        sia.expand_labels(2.0)


def test_slab_jobs_name_the_pass():
    from tissue_analysis_amd.distributed import PipelinedSlabJob, SlabJob
    for cls in (SlabJob, PipelinedSlabJob):
        with pytest.raises(NotImplementedError, match="nearest"):
            cls.nearest_labels(object.__new__(cls))


# ---- the C ABI without a GPU --------------------------------------------------------------------------------------------------
def declared():
    text = open(os.path.join(ROOT, "include", "tissue_scan_nearest.h")).read()
    return text, sorted(set(re.findall(r"TA_API\s+int\s+(ta_\w+)\s*\(", text)))


def test_header_and_binding_agree():
    text, names = declared()
    assert names == sorted(_capi.NEAREST_SYMBOLS) and len(names) == 7
    assert not set(_capi.NEAREST_SYMBOLS) & set(_capi.SYMBOLS)
    assert re.search(r"TA_API\s+int\s+ta_nearest_debug\s*\(ta_ctx\*\s*ctx,\s*uint32_t\s+out\[4\]\)", text)
    assert not re.search(r"TA_API\s+(?!int\s)", text)      # every entry point answers an int
    lib = _capi.load()
    for name in names:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int, name
    assert lib.ta_version() == _capi.ABI_VERSION == 5
    assert _capi.NEAREST_NOT_FROM == int(re.search(r"#define\s+TA_NEAREST_NOT_FROM\s+(\d+)u", text).group(1))
    assert _capi.NEAREST_NONE == int(re.search(r"#define\s+TA_NEAREST_NONE\s+(0x[0-9A-F]+)u", text).group(1), 16) == ref.NONE


def test_null_context_is_rejected_without_a_gpu():
    lib = _capi.load()
    spacing = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    out = (ctypes.c_uint32 * 4)()
    ms = ctypes.c_double(0.0)
    calls = dict(ta_nearest_extract=(None, 0, 0, spacing, float("inf"), 0), ta_nearest_get=(None, None, None),
                 ta_nearest_image=(None, 0, 0, None, None), ta_nearest_apply=(None,), ta_nearest_timing=(None, ctypes.byref(ms), None),
                 ta_nearest_debug=(None, out), ta_nearest_set_batch=(None, 0))
    assert sorted(calls) == sorted(_capi.NEAREST_SYMBOLS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == _capi.TA_EINVAL, name
        assert b"NULL" in lib.ta_last_error(), name
