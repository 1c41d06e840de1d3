"""The census of tests/random_cases.py (no GPU): what keeps "random" honest.  Every class the generator can draw must occur often
enough in the fixed list for test_gpu_random_features.py to see it; if a change to the generator loses one, this file fails and
SEED (or a drawing weight) changes -- never a count below, never a case by hand.

Also: two of the smallest cases through every reference with the `first_owned` / `rows` arguments the runner passes."""
import collections

import numpy as np

import random_cases as rc
import range_tiles as rt
from tissue_analysis_amd import _capi


def count(pred):
    return sum(1 for c in rc.cases() if pred(c))


def labels_of(c):
    return int(np.unique(rc.volume(c)).size)


def test_the_list_is_fixed_and_small():
    assert rc.N_CASES == 48 and len(rc.cases()) == 48
    rc.case.cache_clear()
    rc.volume.cache_clear()
    first = [(c, rc.volume(c).copy()) for c in rc.cases()]
    rc.case.cache_clear()
    rc.volume.cache_clear()
    for (c, V), d in zip(first, rc.cases()):
        assert c == d and c.name == d.name and np.array_equal(V, rc.volume(d)) and V.dtype == np.dtype(c.ldtype)
    assert len(set(c.name for c in rc.cases())) == 48
    for c in rc.cases():
        assert rc.voxels(c) <= 160000 and rc.volume(c).shape == rc.signal(c).shape == rc.second(c).shape == c.dims
        assert rc.signal(c).dtype == np.dtype(c.sdtype) and rc.second(c).dtype == np.dtype(c.bdtype)
        assert sorted(rc.pass_order(c.index)) == sorted(rc.PASSES) and sorted(rc.fetch_order(c.index)) == sorted(rc.FETCHES)
        assert rc.pass_order(c.index).index("distance") < rc.pass_order(c.index).index("profile")
        assert rc.pass_order(c.index) == rc.pass_order(c.index) and rc.fetch_order(c.index) == rc.fetch_order(c.index)
        e = rc.edges2(c)
        assert e.size == c.prof_bins + 1 and e[0] >= 0.0 and (np.diff(e) > 0).all()
        assert rc.ranks(c).shape == (rc.row_image(c)[1], c.rank_kind or 5)
    assert len(set(rc.pass_order(i) for i in range(48))) > 40 and len(set(rc.fetch_order(i) for i in range(48))) > 40


def test_every_mode_layout_and_dtype_pair_occurs():
    for mode in rc.MODES:
        assert count(lambda c: c.mode == mode) >= 4, mode
    assert count(lambda c: c.mode == "slab") == 8
    for c in rc.cases():
        if c.mode == "slab":
            assert c.origin > 0 and c.dims[0] >= 2
        if c.mode == "adopt_offset":
            assert c.label_off == 1
    assert count(lambda c: c.mode == "adopt_offset" and c.signal_off) >= 1 and count(lambda c: c.mode == "adopt_offset" and not c.signal_off) >= 1
    assert count(lambda c: c.mode == "adopt_offset" and c.second_off) >= 1 and count(lambda c: c.mode == "adopt_offset" and not c.second_off) >= 1
    for ldtype in ("uint16", "uint32"):
        for sdtype in ("uint8", "uint16"):
            assert count(lambda c: (c.ldtype, c.sdtype) == (ldtype, sdtype)) >= 6, (ldtype, sdtype)
        for bdtype in ("uint16", "uint32"):
            assert count(lambda c: (c.ldtype, c.bdtype) == (ldtype, bdtype)) >= 6, (ldtype, bdtype)


def test_ids_above_the_dense_limit_run_compacted():
    for c in rc.cases():
        top = int(rc.volume(c).max())
        if top > rc.DENSE_ID_LIMIT:
            assert rc.compacted(c), c.name
        rows, nrows, ids = rc.row_image(c)
        assert nrows <= rc.DENSE_ID_LIMIT + 1 and (ids is None) == (not rc.compacted(c))
    for ids in rc.IDS:
        assert count(lambda c: c.ids == ids) >= 3, ids
    assert count(lambda c: int(rc.volume(c).max()) == 65535) >= 1 and count(lambda c: int(rc.volume(c).max()) == 1 << 20) >= 1
    assert count(lambda c: 0 in rc.volume(c)) >= 6


def test_both_load_paths_and_the_thin_and_tall_shapes_occur():
    for ldtype in ("uint16", "uint32"):
        for path in (True, False):
            n = count(lambda c: c.ldtype == ldtype and rt.vector_path(rc.memory_dims(c), np.dtype(ldtype).itemsize) == path)
            assert n >= 10, (ldtype, path, n)
    assert count(lambda c: rc.memory_dims(c)[0] > 16) >= 8
    assert count(lambda c: rc.memory_dims(c)[1] < 4) >= 8
    assert count(lambda c: c.dims[2] == 1 or c.dims[0] == 1) >= 6


def test_every_class_of_labels_and_signal_occurs():
    for field in rc.FIELDS:
        assert count(lambda c: c.field == field) >= 4, field
    for sig in rc.SIGNALS:
        assert count(lambda c: c.signal == sig) >= 4, sig
    assert count(lambda c: labels_of(c) > _capi.SIGHIST_SLOTS) >= 6
    # ... and in ONE tile of the histogram pass (4 rows x 64 * VPL columns x 16 planes of the memory order)
    def crowded(c):
        V = rc.memory_view(c, rc.volume(c))
        tile = V[rc.first_owned(c):][:rt.PLANES, :rt.WAVES, :rt.columns(V.dtype.itemsize)]
        return np.unique(tile).size > _capi.SIGHIST_SLOTS
    assert count(crowded) >= 4
    for c in rc.cases():
        if c.field == "unique":
            assert labels_of(c) == rc.voxels(c) <= 4096
        if c.field == "speckle":
            assert labels_of(c) <= 6
        assert np.unique(rc.second(c)).size <= 7


def test_every_option_occurs():
    for tp in (0, 1, 5, 32):
        assert count(lambda c: c.tile_planes == tp) >= 4, tp
    for shape in (-1, 0, 1):
        assert count(lambda c: c.ldtype == "uint32" and c.sweep_shape == shape) >= 3, shape
    assert count(lambda c: c.dist_mode == rc.OWN_WALL) >= 8
    assert count(lambda c: c.dist_mode == rc.FROM_LABEL and c.site_present) >= 4
    assert count(lambda c: c.dist_mode == rc.FROM_LABEL and not c.site_present) >= 2
    for c in rc.cases():
        if c.dist_mode == rc.FROM_LABEL:
            assert (rc.site_label(c) in rc.volume(c)) == c.site_present
    assert count(lambda c: c.edge_is_site) >= 8 and count(lambda c: not c.edge_is_site) >= 8
    for spacing in rc.SPACINGS:
        assert count(lambda c: c.spacing == spacing) >= 4, spacing
    for bins in (1, 5, 64):
        assert count(lambda c: c.prof_bins == bins) >= 4, bins
    assert count(lambda c: c.prof_last_inf) >= 8 and count(lambda c: not c.prof_last_inf) >= 8
    assert count(lambda c: c.prof_signal) >= 8 and count(lambda c: not c.prof_signal) >= 8
    assert count(lambda c: c.sdtype == "uint8" and c.log2_width in (0, 8)) >= 1 and count(lambda c: c.sdtype == "uint16" and c.log2_width in (8, 16)) >= 1
    for c in rc.cases():
        assert (0 if c.sdtype == "uint8" else 8) <= c.log2_width <= 8 * np.dtype(c.sdtype).itemsize
    assert count(lambda c: c.rank_kind == 0) >= 16
    for n in (1, 2, 3, 8):
        assert count(lambda c: c.rank_kind == n) >= 1, n
    beyond = 0
    for c in rc.cases():
        if c.rank_kind:
            rows, nrows, _ = rc.row_image(c)
            n = np.bincount(rows[rc.first_owned(c):].reshape(-1).astype(np.int64), minlength=nrows).astype(np.uint64)
            r = rc.ranks(c)
            beyond += bool(((r >= n[:, None]) & (r != rc.NO_RANK)).any())
    assert beyond >= 8


def test_every_pass_runs_often_enough():
    for what in rc.FETCHES:
        n = count(lambda c: rc.runs(c, what))
        assert n >= (12 if what == "walls" else 40), (what, n)
    assert count(rc.whole) == 40


def test_profile_edges_lie_on_distances_the_volume_has():
    """An edge that equals a D2 value decides a voxel by `<` against `<=`."""
    import distance_reference
    on = 0
    for c in rc.cases():
        if rc.whole(c) and c.prof_on_lattice and rc.voxels(c) <= 20000:      # (the small ones are enough, and quick)
            d2 = distance_reference.scipy_d2(rc.volume(c), c.spacing, c.dist_mode, rc.site_label(c), c.edge_is_site)
            on += bool(np.isin(rc.edges2(c), d2[np.isfinite(d2)]).any())
    assert on >= 4


def test_the_chains_change_between_compacted_and_dense():
    chains = rc.chains()
    assert len(chains) == 8 and all(len(ch) == 6 for ch in chains)
    assert sorted(i for ch in chains for i in ch) == list(range(48))
    kinds = collections.Counter()
    for ch in chains:
        to_dense, to_compact = rc.transitions(ch)
        assert to_dense >= 1 and to_compact >= 1, ch
        v = [rc.voxels(rc.case(i)) for i in ch]
        assert v[0] == max(v) and v[1] == min(v) and all(x <= v[0] for x in v[1:])
        assert len(set(rc.case(i).ldtype for i in ch)) == 2 or len(set(rc.case(i).dims for i in ch)) > 1
        kinds.update(rc.case(i).mode for i in ch[1:])
    assert all(kinds[m] >= 2 for m in rc.MODES)          # every mode also runs in buffers a bigger case left


def test_two_small_cases_through_every_reference():
    """The runner's plumbing without a GPU: the smallest slab and the smallest compacted case."""
    by_size = sorted(rc.cases(), key=rc.voxels)
    slab = next(c for c in by_size if c.mode == "slab")
    compact = next(c for c in by_size if c.mode == "compact")
    for c in (slab, compact):
        ref = rc.references(c.index)
        V, (rows, nrows, ids) = rc.volume(c), rc.row_image(c)
        fo = rc.first_owned(c)
        owned = V[fo:].size
        assert ref["nrows"] == nrows and int(ref["sweep"]["count"].sum()) == owned and ref["sweep"]["count"].shape == (nrows,)
        assert int(ref["signal_labels"]["n"].sum()) == owned and ref["signal_labels"]["n"].shape == (nrows,)
        assert np.array_equal(ref["signal_labels"]["n"], ref["sweep"]["count"])
        assert np.array_equal(ref["signal_walls"]["lo"], ref["sweep"]["pair_lo"]) and np.array_equal(ref["signal_walls"]["hi"], ref["sweep"]["pair_hi"])
        assert np.array_equal(ref["signal_walls"]["faces"], ref["sweep"]["pair_faces"])
        assert np.array_equal(ref["wallgeo"]["lo"], ref["sweep"]["pair_lo"].astype(np.int64))
        assert np.array_equal(ref["wallgeo"]["fwd"] + ref["wallgeo"]["rev"], ref["sweep"]["pair_faces"])
        assert int(ref["overlap"][2].sum()) == owned
        assert int(ref["components"][0][1].sum()) == owned and ref["components"][1].shape == V.shape
        assert ref["sighist"].shape == (nrows, 1 << (8 * np.dtype(c.sdtype).itemsize - c.log2_width))
        assert np.array_equal(ref["sighist"].sum(axis=1), ref["sweep"]["count"])
        assert len(ref["junctions"]) == 3
    assert "d2" not in rc.references(slab.index) and "mesh" not in rc.references(slab.index) and "walls" not in rc.references(slab.index)
    c, ref = compact, rc.references(compact.index)
    rows, nrows, ids = rc.row_image(c)
    assert np.array_equal(ids[rows.astype(np.int64)], rc.volume(c)) and ref["d2"].shape == c.dims
    assert ref["distance"][0].shape == (nrows,) and ref["profile"]["n"].shape == (nrows, c.prof_bins)
    assert ("sum" in ref["profile"]) == c.prof_signal and ref["sigrank"].shape == rc.ranks(c).shape
    assert np.array_equal(ref["mesh"]["labels"], ids.astype(np.int64))
    if "walls" in ref:
        assert np.isin(ref["walls"][0], ids).all() and ref["medians"][0].size == np.unique(ref["medians"][0]).size
