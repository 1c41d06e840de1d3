"""The host side of the distance-shell profiles (tissue_analysis_amd/shell_profile.py) against tests/profile_reference.py and
against plain per-label NumPy, on a small Voronoi volume with D2 from distance_reference.brute_d2.  No device."""
import numpy as np
import pytest

import distance_reference as dref
import profile_reference as pref
from tissue_analysis_amd import ShellProfile, synth

HALF = (0.5, 0.5, 1.0)
EDGES = np.array([0.0, 0.6, 1.0, 1.5, 2.5, np.inf])          # distances, real units


@pytest.fixture(scope="module")
def case():
    V = synth.voronoi_labels((8, 12, 30), 12, 4, dtype=np.uint16)
    d2 = dref.brute_d2(V, HALF)
    S = np.random.default_rng(6).integers(0, 65535, V.shape, endpoint=True).astype(np.uint16)
    rows = int(V.max()) + 2                                   # one label more than the volume holds: an absent row
    t = pref.table(V, d2, S, np.square(EDGES), rows)
    prof = ShellProfile(np.arange(rows), EDGES, t["n"], t["sum"], t["sumsq"], t["min"], t["max"], voxelsize=HALF)
    return V, d2, S, t, prof


def test_reference_against_a_loop_over_labels_and_shells(case):
    V, d2, S, t, _ = case
    e2 = np.square(EDGES)
    assert len(np.unique(V)) > 5 and int(t["n"].sum()) == int(np.isfinite(d2).sum()) == V.size
    for l in np.unique(V):
        for k in range(len(EDGES) - 1):
            m = (V == l) & (d2 >= e2[k]) & (d2 < e2[k + 1])
            assert int(t["n"][l, k]) == int(m.sum())
            assert int(t["sum"][l, k]) == int(S[m].astype(np.int64).sum())
            assert t["sumsq"][l, k] == sum(int(v) ** 2 for v in S[m])
            assert int(t["min"][l, k]) == (int(S[m].min()) if m.any() else 0xFFFFFFFF)
            assert int(t["max"][l, k]) == (int(S[m].max()) if m.any() else 0)
    assert (t["n"].sum(axis=0) > 0).all()                    # every shell is used by some label ...
    assert (t["n"][np.unique(V)] == 0).any()                 # ... and some label leaves one empty


def test_arithmetic(case):
    V, d2, S, t, prof = case
    e2 = np.square(EDGES)
    labels = [int(l) for l in np.unique(V)]
    assert sorted(prof.count()) == labels                    # the absent row is not answered
    count, vol, vox = prof.count(), prof.volume(), prof.volume(real=False)
    mean, std, total, lo, hi, frac = prof.mean(), prof.std(), prof.total(), prof.minimum(), prof.maximum(), prof.fraction()
    for l in labels:
        assert count[l].dtype == np.uint64 and np.array_equal(count[l], t["n"][l])
        assert np.array_equal(vox[l], t["n"][l].astype(np.float64)) and np.array_equal(vol[l], vox[l] * 0.25)
        assert np.array_equal(total[l], t["sum"][l])
        whole = float(S[V == l].astype(np.int64).sum())
        for k in range(prof.shells):
            m = (V == l) & (d2 >= e2[k]) & (d2 < e2[k + 1])
            if not m.any():
                assert np.isnan(mean[l][k]) and np.isnan(std[l][k]) and np.isnan(lo[l][k]) and np.isnan(hi[l][k])
                assert frac[l][k] == 0.0
                continue
            v = S[m].astype(np.float64)
            assert mean[l][k] == v.sum() / v.size
            assert abs(std[l][k] - v.std()) <= 1e-9 * max(v.std(), 1.0)
            assert lo[l][k] == v.min() and hi[l][k] == v.max()
            assert frac[l][k] == v.sum() / whole
        assert abs(np.nansum(frac[l]) - 1.0) < 1e-12


def test_labels_and_exclude(case):
    V, _, _, t, prof = case
    labels = [int(l) for l in np.unique(V)]
    absent = int(V.max()) + 1
    assert sorted(prof.mean(exclude=labels[:2])) == labels[2:]
    assert list(prof.count(labels=[labels[3], absent, 99999, labels[1]])) == [labels[3], labels[1]]
    assert prof.count(labels=[labels[3]], exclude=[labels[3]]) == {}
    assert prof.rows_of([labels[0], 99999]).tolist() == [labels[0], -1]
    assert len(prof) == absent + 1 and prof.shells == 5 and not prof.present[absent]
    own = ShellProfile([3, 7], [0.0, 1.0], [[2], [0]], present=[True, True])
    assert list(own.count()) == [3, 7] and own.count()[7].tolist() == [0]


def test_a_voxel_on_an_edge_goes_to_the_upper_shell():
    V = np.ones((1, 1, 6), dtype=np.uint16)
    V[0, 0, 3:] = 2
    d2 = dref.brute_d2(V)                                    # 9, 4, 1 | 1, 4, 9
    assert d2.reshape(-1).tolist() == [9.0, 4.0, 1.0, 1.0, 4.0, 9.0]
    t = pref.table(V, d2, None, [1.0, 4.0, 9.0], 3)          # shells [1, 4) and [4, 9): 9 is counted nowhere, 4 in the upper one
    assert t["n"].tolist() == [[0, 0], [1, 1], [1, 1]]
    assert pref.table(V, d2, None, [0.0, 1.0], 3)["n"].sum() == 0          # d2 == 1 lies at the last edge: nowhere
    inf = np.full(V.shape, np.inf)
    assert pref.table(V, inf, None, [0.0, np.inf], 3)["n"].sum() == 0      # +inf is in no shell, even under a last edge of +inf
    assert pref.table(V, d2, None, [0.0, np.inf], 3)["n"].tolist() == [[0], [3], [3]]


def test_constructor_validation():
    ok = dict(labels=[1, 2], edges=[0.0, 1.0, 2.0], n=[[1, 2], [3, 4]])
    p = ShellProfile(**ok)
    assert not p.has_signal and p.voxelsize == (1.0, 1.0, 1.0)
    for name in ("mean", "std", "total", "minimum", "maximum", "fraction"):
        with pytest.raises(ValueError):
            getattr(p, name)()
    for bad in (dict(labels=[2, 1]), dict(edges=[0.0]), dict(edges=[0.0, 1.0, 1.0]), dict(edges=[-1.0, 1.0, 2.0]),
                dict(edges=[0.0, float("nan"), 2.0]), dict(n=[[1, 2, 3], [4, 5, 6]]), dict(n=[[1, 2]]), dict(voxelsize=(1.0,)),
                dict(present=[True]), dict(sum=[[1, 1], [1, 1]])):
        with pytest.raises(ValueError):
            ShellProfile(**dict(ok, **bad))
    cols = dict(sum=[[1, 2], [3, 4]], min=[[1, 2], [3, 4]], max=[[1, 2], [3, 4]])
    with pytest.raises(ValueError):
        ShellProfile(sumsq=[[1, 2, 3]], **dict(ok, **cols))
    big = (1 << 64) + 5                                      # the device's two words and Python integers are the same table
    a = ShellProfile(sumsq=np.array([[[5, 1], [2, 0]], [[3, 0], [4, 0]]], dtype=np.uint64), **dict(ok, **cols))
    b = ShellProfile(sumsq=np.array([[big, 2], [3, 4]], dtype=object), **dict(ok, **cols))
    assert a.sumsq.dtype == object and a.sumsq.tolist() == b.sumsq.tolist() == [[big, 2], [3, 4]]
    assert pref.words(a.sumsq).tolist() == [[[5, 1], [2, 0]], [[3, 0], [4, 0]]]
    two = ShellProfile([4], [0.0, 2.0], [[6]], voxelsize=(0.5, 0.25))
    assert two.voxelsize == (0.5, 0.25, 1.0) and two.volume()[4].tolist() == [0.75] and two.volume(real=False)[4].tolist() == [6.0]
