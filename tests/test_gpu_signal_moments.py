"""Signal-weighted moments on the MI355X (include/tissue_scan_sigmoments.h, csrc/kernels_sigmoments.hip) against the restatement
of tests/sigmoment_reference.py: the eleven integers of every row bit-exact, the floats of `SignalMoments` to 1e-12 relative, the
launch plan the device reports equal to the restated one -- at the shapes where the exactness cap of the header binds too."""
import os
import types

import numpy as np
import pytest

import range_tiles as rt
import sigmoment_reference as ref
from feature_passes import Pass, code, poke, tensor
from tissue_analysis_amd import DICT, LIST, NPLIST, SignalMoments, SpatialImage, SpatialImageAnalysis, _capi, synth
from tissue_analysis_amd.extraction import ResidentVolume
from tissue_analysis_amd.graph_from_image import graph_from_image

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same_integers(got, want):
    """got: (n, w, m1, m2 words) as the library gives them; want: ref.rows()."""
    n, w, m1, m2 = got
    assert np.array_equal(n, want["n"]), "n"
    assert np.array_equal(w, want["w"]), "w"
    assert np.array_equal(m1, want["m1"]), "m1"
    assert np.array_equal(m2, want["m2_words"]), "m2"


def check_moments(m, V, S):
    """m: SignalMoments of signal S over label image V (any dense layout), from a ResidentVolume."""
    x = m.extraction
    V3, S3 = (V, S) if V.ndim == 3 else (V[:, :, None], S[:, :, None])
    Vm, Sm = V3.transpose(m.perm), S3.transpose(m.perm)           # the memory-order views
    assert Vm.flags.c_contiguous or 1 in Vm.shape
    nrows = x.nrows
    rows = None if x.ids is None else np.searchsorted(x.ids, Vm.astype(np.int64))
    r = ref.rows(Vm, Sm, nrows, rows)
    same_integers((m.n, m.w, m.m1, m.m2), r)
    assert np.array_equal(m.n, x.count)
    # floats: the reference's, formed in memory-axis order from the same integers and the extraction's geometry
    perm = list(m.perm)
    geometry = types.SimpleNamespace(count=x.count, sum1=x.sum1[:, perm])
    vs = (0.5, 0.25, 2.0)
    f = ref.floats(r, geometry, [vs[a] for a in perm])
    scaled = SignalMoments(x, m.n, m.w, m.m1, m.m2, m.perm, vs)
    cen, pol, cov = scaled.centroid(), scaled.polarity(), scaled.covariance()
    for k in range(3):
        np.testing.assert_allclose(cen[:, perm[k]], f["centroid"][:, k], rtol=1e-12, atol=0, equal_nan=True)
        np.testing.assert_allclose(pol[:, perm[k]], f["polarity"][:, k], rtol=1e-12, atol=0, equal_nan=True)
        for j in range(3):
            np.testing.assert_allclose(cov[:, perm[k], perm[j]], f["covariance"][:, k, j], rtol=1e-12, atol=0, equal_nan=True)
    return r


def _run(V, S, **kw):
    rv = ResidentVolume(V)
    try:
        rv.extract(**kw)
        m = rv.signal_moments(S)
        assert rv.ctx.sigmom_debug()["groups"] >= 1
    finally:
        rv.close()
    assert isinstance(m, SignalMoments) and m.ms is not None and m.ms >= 0
    return m


def _c1(dtype=np.uint16):
    c = synth.CONFIGS["C1"]
    return synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], dtype)


# ---- 1. types and load paths ----------------------------------------------------------------------------------------------------
def test_adversarial_golden_volumes():
    z = np.load(os.path.join(GOLD, "adversarial_small.npz"))
    names = sorted(set(k.split("__")[0] for k in z.files))
    for i, name in enumerate(names):
        V = z[name + "__volume"]
        for sdt in (np.uint8, np.uint16):
            S = rt.random_image(V.shape, sdt, i)
            check_moments(_run(V, S), V, S)


@pytest.mark.parametrize("ldt", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("sdt", [np.uint8, np.uint16], ids=["s8", "s16"])
def test_config1_label_and_signal_types(ldt, sdt):
    V = _c1().astype(ldt)
    S = rt.random_image(V.shape, sdt, 7)
    check_moments(_run(V, S), V, S)


def test_fortran_ordered_pair():
    V, S = np.asfortranarray(_c1()), np.asfortranarray(rt.random_image(synth.CONFIGS["C1"]["dims"], np.uint16, 8))
    m = _run(V, S)
    assert m.perm == (2, 1, 0)
    check_moments(m, V, S)
    # the floats are those of the C-ordered copy: the layout does not show in array axes
    c = _run(np.ascontiguousarray(V), np.ascontiguousarray(S))
    assert c.perm == (0, 1, 2)
    np.testing.assert_allclose(m.centroid(), c.centroid(), rtol=1e-12, equal_nan=True)
    np.testing.assert_allclose(m.covariance(), c.covariance(), rtol=1e-12, equal_nan=True)


def test_rows_that_are_no_whole_strips():
    V = np.ascontiguousarray(_c1()[:, :, :61])                    # the element loads
    S = rt.random_image(V.shape, np.uint8, 9)
    check_moments(_run(V, S), V, S)


def test_sparse_ids_compacted_context():
    rng = np.random.default_rng(5)
    ids = np.array([0, 7, 70000, 2**31 + 5, 2**32 - 2, 2**32 - 1], dtype=np.uint32)
    V = ids[rng.integers(0, ids.size, size=(12, 9, 33))]
    S = rt.random_image(V.shape, np.uint16, 6)
    m = _run(V, S, sparse=True)
    assert m.ids is not None and np.array_equal(m.ids, ids.astype(np.int64)) and len(m) == ids.size      # the rows are ranks
    check_moments(m, V, S)
    got = m.of_labels([2**32 - 1, 7, 12345], "centroid", real=False)
    assert np.array_equal(got[0], m.centroid(real=False)[5]) and np.array_equal(got[1], m.centroid(real=False)[1]) and np.isnan(got[2]).all()


# ---- 2 .. 5: ranges, spills, the carry, the cap ------------------------------------------------------------------------------------
def check_pass(p, S):
    """Run the pass on the context of p (a feature_passes.Pass with an extraction and the signal S set): rows against the reference,
    the plan the device reports against the restated one.  Returns (debug, reference rows, restated plan)."""
    p.ctx.sigmom_extract()
    debug = p.ctx.sigmom_debug()
    plan = ref.plan(p.V.shape, p.first_owned, p.V.dtype.itemsize, S.dtype.itemsize)
    assert (debug["tiles_per_group"], debug["groups"]) == (plan.per, plan.groups), (debug, plan)
    r = ref.rows(p.V, S, p.max_label + 1, first_owned=p.first_owned)
    same_integers(p.ctx.sigmom_rows(), r)
    assert int(r["n"].sum()) == p.V[p.first_owned:].size
    return debug, r, plan


@pytest.mark.parametrize("name,per,last", [("a_u16", 2, 1), ("c_u32", 5, None), ("a_u16_halo", 2, 1)])
def test_tile_ranges(name, per, last):
    case = rt.CASE[name]
    V = rt.block_labels(case.dims, case.dtype, 41)
    S = rt.random_image(case.dims, np.uint16 if case.dtype == np.uint16 else np.uint8, 42)
    with Pass(V, first_owned=case.first_owned) as p:
        p.extract()
        p.set_signal(S)
        _, _, plan = check_pass(p, S)
        assert plan.per == per == plan.uncapped and plan.groups > 1 and (last is None or plan.tiles_in_last_group == last)


@pytest.mark.parametrize("dims,dtype", [(rt.SPILL_DIMS, np.uint16), (rt.SPILL_DIMS_WIDE, np.uint32)], ids=["one_tile_u16", "wide_u32"])
def test_label_table_spills(dims, dtype):
    V = rt.permutation_labels(dims, dtype, 43)
    S = rt.random_image(dims, np.uint16, 44)
    bound = ref.label_spill_bound(V, 0, 2)
    assert bound > 0 and (dims != rt.SPILL_DIMS or bound == 4096 - ref.LABEL_SLOTS)
    with Pass(V) as p:
        p.extract()
        p.set_signal(S)
        debug, _, _ = check_pass(p, S)
        assert debug["spills"] >= bound


def test_the_carry_into_the_high_word():
    dims = (4, 4, 65536)
    V = np.full(dims, 1, dtype=np.uint16)
    S = np.full(dims, 65535, dtype=np.uint16)
    with Pass(V) as p:
        p.extract()
        p.set_signal(S)
        debug, r, plan = check_pass(p, S)
        assert (plan.most, plan.per, plan.groups) == (2, 1, 128)
        m2 = p.ctx.sigmom_rows()[3]
    want = 16 * 65535 * sum(c * c for c in range(65536))
    assert r["m2"][1, 5] == want and want >> 64 == 5
    assert int(m2[1, 5, 1]) == 5 and (int(m2[1, 5, 1]) << 64) | int(m2[1, 5, 0]) == want


def test_the_exactness_cap_binds():
    dims = (1, 12, 98304)
    V = rt.block_labels(dims, np.uint32, 45)
    S = rt.random_image(dims, np.uint16, 46)
    with Pass(V) as p:
        p.extract()
        p.set_signal(S)
        debug, _, plan = check_pass(p, S)
        assert (plan.tiles, plan.uncapped, plan.most, plan.per, plan.groups) == (1152, 2, 1, 1, 1152)
        assert (debug["tiles_per_group"], debug["groups"]) == (1, 1152)
        # a uint8 signal leaves room for the two tiles the plan asks for
        S8 = rt.random_image(dims, np.uint8, 47)
        p.set_signal(S8)
        debug, _, plan = check_pass(p, S8)
        assert (plan.per, plan.groups) == (2, 576)


def test_dims_too_large_for_one_tile_are_refused():
    dims = (1, 1, (1 << 20) + 8)
    V = np.ones(dims, dtype=np.uint16)
    assert ref.plan(dims, 0, 2, 2).most == 0 and ref.plan(dims, 0, 2, 1).most > 0
    with Pass(V) as p:
        p.extract()
        p.set_signal(np.ones(dims, dtype=np.uint16))
        assert code(p.ctx.sigmom_extract) == _capi.TA_EINVAL
        assert code(p.ctx.sigmom_rows) == _capi.TA_EINVAL
        S8 = np.full(dims, 255, dtype=np.uint8)               # ... and taken with a signal whose sums fit
        p.set_signal(S8)
        check_pass(p, S8)


# ---- 6. slabs -------------------------------------------------------------------------------------------------------------------
def test_two_slab_contexts_with_a_halo_merge_to_the_whole():
    V = _c1()
    S = rt.random_image(V.shape, np.uint16, 11)
    L = int(V.max())
    cut = 37
    parts = []
    for lo, hi, halo in ((0, cut, False), (cut - 1, V.shape[0], True)):
        origin = lo + (1 if halo else 0)
        tv, ts = tensor(V[lo:hi]), tensor(S[lo:hi])
        ctx = _capi.Context(0)
        try:
            ctx.set_volume_device(tv.data_ptr(), 2, tv.shape, a0_origin=origin, has_low_halo=halo, keep=tv)
            ctx.set_signal_device(ts.data_ptr(), 2, keep=ts)
            ctx.extract(_capi.F_ALL, L)
            ctx.sigmom_extract()
            n, w, m1, m2 = ctx.sigmom_rows()
            same_integers((n, w, m1, m2), ref.rows(V[lo:hi], S[lo:hi], L + 1, first_owned=1 if halo else 0))      # local rows
            parts.append(SignalMoments(None, n, w, m1, m2, origin0=origin))
        finally:
            ctx.close()
    merged = SignalMoments.merge(parts)
    with Pass(V) as p:
        p.extract()
        p.set_signal(S)
        p.ctx.sigmom_extract()
        whole = p.ctx.sigmom_rows()
    same_integers((merged.n, merged.w, merged.m1, merged.m2), ref.rows(V, S, L + 1))
    for a, b in zip((merged.n, merged.w, merged.m1, merged.m2), whole):
        assert np.array_equal(a, b)


# ---- 7. staleness ---------------------------------------------------------------------------------------------------------------
def test_what_makes_the_rows_stale():
    V = rt.block_labels((24, 20, 70), np.uint16, 31, nlabels=40)
    S = rt.random_image(V.shape, np.uint8, 2)
    getters = lambda ctx: (ctx.sigmom_rows, ctx.sigmom_debug)
    with Pass(V) as p:
        assert code(p.ctx.sigmom_timing) == _capi.TA_EINVAL and code(p.ctx.sigmom_rows) == _capi.TA_EINVAL
        p.set_signal(S)
        assert code(p.ctx.sigmom_extract) == _capi.TA_EINVAL           # no extraction yet
        p.extract()
        check_pass(p, S)
        p.set_signal(S)                                                 # a new signal, even the same voxels
        assert [code(g) for g in getters(p.ctx)] == [_capi.TA_EINVAL] * 2
        check_pass(p, S)
        p.ctx.relabel(np.arange(p.max_label + 1, dtype=np.uint32))      # ta_volume_relabel
        assert [code(g) for g in getters(p.ctx)] == [_capi.TA_EINVAL] * 2
        assert code(p.ctx.sigmom_extract) == _capi.TA_EINVAL
        p.extract()
        check_pass(p, S)
        p.extract()                                                     # a new extraction, even of the same volume
        assert [code(g) for g in getters(p.ctx)] == [_capi.TA_EINVAL] * 2
        check_pass(p, S)
        p.ctx.set_volume(V)                                             # a new volume
        assert [code(g) for g in getters(p.ctx)] == [_capi.TA_EINVAL] * 2


def test_filling_erased_voxels_makes_the_rows_stale():
    V = rt.block_labels((20, 18, 40), np.uint16, 33, nlabels=30)
    V[5:9, 4:9, 10:20] = 0                                              # erased voxels
    S = rt.random_image(V.shape, np.uint16, 3)
    sia = SpatialImageAnalysis(SpatialImage(V.copy(), voxelsize=(1.0, 1.0, 1.0)), return_type=DICT, background=None)
    before = sia.signal_center_of_mass(S, real=False)
    ctx = sia._resident().ctx
    ctx.sigmom_rows()
    assert sum(sia.fill_erased_voxels().values()) == 4 * 5 * 10
    assert code(ctx.sigmom_rows) == _capi.TA_EINVAL and code(ctx.sigmom_debug) == _capi.TA_EINVAL
    filled = np.asarray(sia.image)
    assert not (filled == 0).any()
    after = sia.signal_center_of_mass(S, real=False)                    # the cache went with the labels
    r = ref.rows(filled, S, int(filled.max()) + 1)
    for l in after:
        np.testing.assert_allclose(after[l], r["m1"][l] / r["w"][l], rtol=1e-12)
    assert any(not np.array_equal(before[l], after[l]) for l in after)


def test_a_label_above_max_label_in_an_edited_buffer():
    V = rt.block_labels((24, 20, 70), np.uint16, 31, nlabels=40)
    S = rt.random_image(V.shape, np.uint16, 32)
    with Pass(V, adopted=True) as p:
        p.extract()
        p.set_signal(S)
        check_pass(p, S)
        poke(p.t, (3, 4, 5), p.max_label + 1)
        p.ctx.sigmom_extract()
        for get in (p.ctx.sigmom_rows, p.ctx.sigmom_debug):
            assert code(get) == _capi.TA_ERANGE
        poke(p.t, (3, 4, 5), V[3, 4, 5])
        assert code(p.ctx.sigmom_rows) == _capi.TA_ERANGE              # the results of that pass stay what they are
        p.extract()
        check_pass(p, S)


# ---- 8. the analysis methods and the graph ----------------------------------------------------------------------------------------
def test_analysis_methods_and_graph():
    from scipy import ndimage
    V = _c1()
    S = rt.random_image(V.shape, np.uint16, 12)
    vs = (0.5, 0.25, 2.0)
    img = SpatialImage(V, voxelsize=vs)
    r = ref.rows(V, S, int(V.max()) + 1)
    for rt_ in (DICT, LIST, NPLIST):
        sia = SpatialImageAnalysis(img, ignoredlabels=0, return_type=rt_, background=1)
        labels = sia.labels()
        want = np.asarray(ndimage.center_of_mass(S, V, labels)) * vs
        got = sia.signal_center_of_mass(S)
        vals = np.array([got[l] for l in labels]) if rt_ == DICT else np.asarray(got)
        np.testing.assert_allclose(vals, want, rtol=1e-6)
        m = sia._signal_moments(S)
        same_integers((m.n, m.w, m.m1, m.m2), r)
        pol = sia.signal_polarity(S)
        pvals = np.array([pol[l] for l in labels]) if rt_ == DICT else np.asarray(pol)
        com = sia.center_of_mass()
        cvals = com if rt_ == NPLIST else np.array([com[l] for l in labels])
        np.testing.assert_allclose(pvals, vals - cvals, rtol=1e-6, atol=1e-9)
        assert np.array_equal(pvals, m.polarity()[labels])
        index = sia.signal_polarity(S, normalised=True, real=False)
        ivals = np.array([index[l] for l in labels]) if rt_ == DICT else np.asarray(index)
        assert ivals.shape == (len(labels), 3) and (np.linalg.norm(ivals, axis=1) < 1).all()
        axes, values = sia.signal_inertia_axis(S)
        vecs, evals = m.inertia_axis()
        if rt_ == NPLIST:
            assert np.array_equal(axes, vecs[labels]) and np.array_equal(values, evals[labels])
        else:
            first = labels[0]
            a0 = axes[first] if rt_ == DICT else axes[0]
            assert np.array_equal(np.asarray(a0), vecs[first]) and (np.diff(evals[first]) <= 0).all()
        # a scalar label: a bare vector
        one = sia.signal_center_of_mass(S, labels[3])
        assert isinstance(one, np.ndarray) and one.shape == (3,) and np.array_equal(one, vals[3])
        assert sia.signal_polarity(S, labels[3]).shape == (3,)
        ax1, val1 = sia.signal_inertia_axis(S, labels[3])
        assert len(ax1) == 3 and val1.shape == (3,)
    assert sia._resident().uploads == 1
    # the graph: the columns are the class's; a property list without them does not run the pass
    sia = SpatialImageAnalysis(img, ignoredlabels=0, return_type=DICT, background=1)
    ctx = sia._resident().ctx
    plain = graph_from_image(sia, background=1, spatio_temporal_properties=["volume", "barycenter", "mean_signal"], signal=S,
                             ignore_cells_at_stack_margins=False)
    assert "signal_barycenter" not in plain.vertex_property_names()
    with pytest.raises(_capi.TissueScanError, match="no signal-moment pass has been run"):
        ctx.sigmom_timing()
    g = graph_from_image(sia, background=1, spatio_temporal_properties=["barycenter", "signal_barycenter", "signal_polarity"], signal=S,
                         ignore_cells_at_stack_margins=False)
    assert ctx.sigmom_timing() >= 0
    m = sia._signal_moments(S)
    cen, valid = g.vertex_column("signal_barycenter")
    pol, pvalid = g.vertex_column("signal_polarity")
    bar, _ = g.vertex_column("barycenter")
    ids = np.asarray(g.vertex_ids)
    assert valid.any() and np.array_equal(valid, pvalid)
    assert np.array_equal(cen[valid], m.centroid()[ids[valid]]) and np.array_equal(pol[valid], m.polarity()[ids[valid]])
    np.testing.assert_allclose(pol[valid], cen[valid] - bar[valid], rtol=1e-6, atol=1e-9)
    voxels = graph_from_image(sia, background=1, spatio_temporal_properties=["signal_barycenter"], signal=S, property_as_real=False,
                              ignore_cells_at_stack_margins=False)
    cen_v, valid_v = voxels.vertex_column("signal_barycenter")
    assert np.array_equal(cen_v[valid_v], m.centroid(real=False)[np.asarray(voxels.vertex_ids)[valid_v]])


# ---- 9. device buffers that are not 16-byte aligned ----------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1], ids=["+0B", "+2B"])
def test_unaligned_label_and_signal_buffers(off):
    from test_gpu_unaligned_buffers import SHAPE_A, offset_view
    V = rt.block_labels(SHAPE_A, np.uint16, 51, nlabels=60)
    S = (rt.random_image(SHAPE_A, np.uint16, 52) >> 1).astype(np.uint16)      # (leaves 65535 for the sentinel of the pads)
    assert rt.vector_path(SHAPE_A, 2)                                         # whole strips: the address alone decides
    ctx = _capi.Context(0)
    try:
        lv = offset_view(V, off, 3)
        sv = offset_view(S, off, 3, sentinel=65535)
        assert lv.dev_ptr % 16 == 2 * off and sv.dev_ptr % 16 == 2 * off
        ctx.set_volume_device(lv.dev_ptr, 2, V.shape, keep=lv.flat)
        ctx.set_signal_device(sv.dev_ptr, 2, keep=sv.flat)
        L = int(V.max())
        ctx.extract(_capi.F_ALL, L)
        ctx.sigmom_extract()
        same_integers(ctx.sigmom_rows(), ref.rows(V, S, L + 1))
        assert np.array_equal(lv.read_back().reshape(V.shape), V) and np.array_equal(sv.read_back().reshape(S.shape), S)
    finally:
        ctx.close()
