"""Two-channel statistics on the MI355X (include/tissue_scan_cosignal.h, csrc/kernels_cosignal.hip) against the restatement of
tests/channel_pair_reference.py: the eleven integer columns of every row bit-exact, the floats of `ChannelPairStats` to 1e-12
relative.  The shapes are stated for the pass's tile, which is the signal pass's: 4 rows x 64 * VPL columns x 16 planes, VPL = 8 for
uint16 labels and 4 for uint32; the launch plan the device reports is compared with tests/range_tiles.py's for that pass."""
import functools
import os

import numpy as np
import pytest

import channel_pair_reference as ref
import range_tiles as rt
from feature_passes import Pass, code, tensor
from tissue_analysis_amd import DICT, LIST, NPLIST, ChannelPairStats, SpatialImage, SpatialImageAnalysis, _capi, synth
from tissue_analysis_amd.extraction import ResidentVolume
from tissue_analysis_amd.graph_from_image import graph_from_image

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TYPES = [(np.uint8, np.uint8), (np.uint8, np.uint16), (np.uint16, np.uint8), (np.uint16, np.uint16)]
TYPE_IDS = ["a8b8", "a8b16", "a16b8", "a16b16"]
FLOATS = ("ratio", "covariance", "pearson", "manders_m1", "manders_m2", "overlap_coefficient", "mask_jaccard")


def same_integers(got, want):
    """got: the dict of ctx.cosignal_rows() (or the columns of a ChannelPairStats); want: ref.labels()."""
    for k in ref.COLUMNS:
        assert got[k].dtype == np.uint64 and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def same_floats(stats, want_columns):
    f = ref.floats(want_columns)
    m1, m2 = stats.manders()
    got = dict(ratio=stats.ratio(), covariance=stats.covariance(), pearson=stats.pearson(), manders_m1=m1, manders_m2=m2,
               overlap_coefficient=stats.overlap_coefficient(), mask_jaccard=stats.mask_jaccard())
    for k in FLOATS:
        np.testing.assert_allclose(got[k], f[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)


def mid(dtype):
    return int(np.iinfo(dtype).max) // 2


def check_pair(st, V, A, B, thr):
    """st: the ChannelPairStats of channels A, B over label image V (any dense layout), from a ResidentVolume."""
    x = st.extraction
    perm = x_perm(V)
    V3, A3, B3 = [a if a.ndim == 3 else a[:, :, None] for a in (V, A, B)]
    Vm, Am, Bm = V3.transpose(perm), A3.transpose(perm), B3.transpose(perm)      # (the sums do not depend on the order; the views are cheap)
    rows = None if x.ids is None else np.searchsorted(x.ids, Vm.astype(np.int64))
    want = ref.labels(Vm, Am, Bm, x.nrows, thr[0], thr[1], rows)
    same_integers(st.columns(), want)
    assert np.array_equal(st.n, x.count) and st.thresholds == tuple(thr)
    same_floats(st, want)
    return want


def x_perm(V):
    if V.ndim != 3:
        return (0, 1, 2)
    return tuple(sorted(range(3), key=lambda d: -V.strides[d]))


def _run(V, A, B, thr=(0, 0), **kw):
    rv = ResidentVolume(V)
    try:
        rv.extract(**kw)
        st = rv.signal_pair(A, B, thr)
        debug = rv.ctx.cosignal_debug()
        assert debug["groups"] >= 1 and rv.ctx.cosignal_thresholds() == tuple(thr)
    finally:
        rv.close()
    assert isinstance(st, ChannelPairStats) and st.ms is not None and st.ms >= 0
    return st


@functools.lru_cache(maxsize=None)
def c1():
    c = synth.CONFIGS["C1"]
    V = synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], np.uint16)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def image(dims, dtype, seed):
    a = rt.random_image(dims, dtype, seed)
    a.setflags(write=False)
    return a


def check_pass(p, A, B, thr=(0, 0)):
    """Run the pass on the context of p (a feature_passes.Pass with an extraction, A as its signal and B set): rows against the
    reference, the plan the device reports against the restated one.  Returns (debug, reference columns)."""
    p.ctx.cosignal_extract(*thr)
    debug = p.ctx.cosignal_debug()
    p.check_plan(debug, "signal")                                  # (the same tile, the same 1024 groups, the same 2^31-voxel cap)
    want = ref.labels(p.V, A, B, p.max_label + 1, thr[0], thr[1], first_owned=p.first_owned)
    same_integers(p.ctx.cosignal_rows(), want)
    assert int(want["n"].sum()) == p.V[p.first_owned:].size
    assert p.ctx.cosignal_thresholds() == tuple(thr)
    return debug, want


def set_b(p, B):
    if p.t is None:
        p.ctx.set_cosignal(B)
    else:
        tb = tensor(B)
        p.ctx.set_cosignal_device(tb.data_ptr(), B.dtype.itemsize, keep=tb)


# ---- 1. every golden volume x the four type combinations ---------------------------------------------------------------------------
@pytest.mark.parametrize("adt,bdt", TYPES, ids=TYPE_IDS)
def test_adversarial_golden_volumes(adt, bdt):
    z = np.load(os.path.join(GOLD, "adversarial_small.npz"))
    names = sorted(set(k.split("__")[0] for k in z.files))
    assert names
    for i, name in enumerate(names):
        V = z[name + "__volume"]
        A, B = rt.random_image(V.shape, adt, 2 * i), rt.random_image(V.shape, bdt, 2 * i + 1)
        thr = (mid(adt), mid(bdt))
        check_pair(_run(V, A, B, thr), V, A, B, thr)


# ---- 2. one step past each tile edge ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,ldt", [((17, 5, 260), np.uint32), ((17, 5, 520), np.uint16)], ids=["u32", "u16"])
@pytest.mark.parametrize("adt,bdt", TYPES, ids=TYPE_IDS)
def test_one_step_past_each_tile_edge(dims, ldt, adt, bdt):
    V = rt.block_labels(dims, ldt, 61, nlabels=50)
    A, B = image(dims, adt, 62), image(dims, bdt, 63)
    plan = rt.plan(dims, 0, np.dtype(ldt).itemsize, "signal")
    assert (plan.ncb, plan.nrb, plan.npb) == (2, 2, 2) and rt.vector_path(dims, np.dtype(ldt).itemsize)
    with Pass(V) as p:
        p.extract()
        p.set_signal(A)
        set_b(p, B)
        debug, _ = check_pass(p, A, B, (mid(adt), mid(bdt)))
        assert debug["spills"] == 0


# ---- 3. layouts ------------------------------------------------------------------------------------------------------------------
def test_rows_that_are_no_whole_strips():
    dims = (3, 5, 61)                                              # the element loads
    V = rt.block_labels(dims, np.uint16, 64, nlabels=20)
    assert not rt.vector_path(dims, 2)
    A, B = image(dims, np.uint16, 65), image(dims, np.uint8, 66)
    check_pair(_run(V, A, B, (1000, 100)), V, A, B, (1000, 100))
    V32 = V.astype(np.uint32)
    check_pair(_run(V32, B, A, (100, 1000)), V32, B, A, (100, 1000))


def test_a_two_dimensional_image():
    rng = np.random.default_rng(67)
    V = np.repeat(np.repeat(rng.integers(1, 30, size=(20, 15)), 10, axis=0), 10, axis=1).astype(np.uint16)
    assert V.shape == (200, 150)
    A, B = rt.random_image(V.shape, np.uint16, 68), rt.random_image(V.shape, np.uint16, 69)
    check_pair(_run(V, A, B, (5, 50000)), V, A, B, (5, 50000))


def test_fortran_ordered_labels_with_c_ordered_channels():
    V = np.asfortranarray(rt.block_labels((24, 20, 70), np.uint16, 70, nlabels=40))
    A, B = image(V.shape, np.uint16, 71), image(V.shape, np.uint8, 72)
    assert A.flags.c_contiguous and not V.flags.c_contiguous
    st = _run(V, A, B, (30000, 128))
    check_pair(st, V, A, B, (30000, 128))
    c = _run(np.ascontiguousarray(V), A, B, (30000, 128))
    same_integers(st.columns(), c.columns())


def test_b_is_the_very_array_that_is_a():
    V = rt.block_labels((17, 9, 72), np.uint16, 73, nlabels=30)
    A = image(V.shape, np.uint16, 74)
    st = _run(V, A, A, (20000, 20000))
    want = check_pair(st, V, A, A, (20000, 20000))
    assert np.array_equal(st.sq_aa, st.sq_ab) and np.array_equal(st.sq_bb, st.sq_ab) and np.array_equal(st.n_a, st.n_ab)
    r = st.pearson()
    varies = np.array([n >= 2 and n * q != int(s) ** 2 for n, q, s in zip(want["n"].tolist(), want["sq_aa_int"], want["sum_a"].tolist())])
    assert varies.any() and (r[varies] == 1.0).all() and np.isnan(r[~varies]).all()
    # ... and B = max - A is exactly -1; the device buffer of A adopted as B too
    comp = _run(V, A, (65535 - A).astype(np.uint16))
    assert (comp.pearson()[varies] == -1.0).all()
    with Pass(V, adopted=True) as p:
        p.extract()
        ta = tensor(A)
        p.ctx.set_signal_device(ta.data_ptr(), 2, keep=ta)
        p.ctx.set_cosignal_device(ta.data_ptr(), 2, keep=ta)
        check_pass(p, A, A, (20000, 20000))


# ---- 4. device buffers that are not 16-byte aligned ----------------------------------------------------------------------------------
@pytest.mark.parametrize("off_a,off_b", [(0, 1), (1, 0), (1, 1)], ids=["B+2B", "A+2B", "both+2B"])
def test_unaligned_channel_buffers(off_a, off_b):
    from test_gpu_unaligned_buffers import SHAPE_A, offset_view
    V = rt.block_labels(SHAPE_A, np.uint16, 51, nlabels=60)
    A = (image(SHAPE_A, np.uint16, 52) >> 1).astype(np.uint16)      # (leaves 65535 for the sentinel of the pads)
    B = (image(SHAPE_A, np.uint16, 53) >> 1).astype(np.uint16)
    assert rt.vector_path(SHAPE_A, 2)                               # whole strips: the addresses alone decide
    L = int(V.max())
    results = []
    for oa, ob in ((0, 0), (off_a, off_b)):                         # the aligned run first: the control
        ctx = _capi.Context(0)
        try:
            lv = offset_view(V, 0, 3)
            av, bv = offset_view(A, oa, 3, sentinel=65535), offset_view(B, ob, 3, sentinel=65535)
            assert lv.dev_ptr % 16 == 0 and av.dev_ptr % 16 == 2 * oa and bv.dev_ptr % 16 == 2 * ob
            ctx.set_volume_device(lv.dev_ptr, 2, V.shape, keep=lv.flat)
            ctx.set_signal_device(av.dev_ptr, 2, keep=av.flat)
            ctx.set_cosignal_device(bv.dev_ptr, 2, keep=bv.flat)
            ctx.extract(_capi.F_ALL, L)
            ctx.cosignal_extract(16000, 16000)
            results.append(ctx.cosignal_rows())
            assert np.array_equal(av.read_back().reshape(A.shape), A) and np.array_equal(bv.read_back().reshape(B.shape), B)
        finally:
            ctx.close()
    same_integers(results[0], ref.labels(V, A, B, L + 1, 16000, 16000))
    same_integers(results[1], results[0])


# ---- 5. table spills -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,ldt,per_tile", [((2, 4, 1030), np.uint32, 2048), ((2, 4, 2060), np.uint16, 4096)], ids=["u32", "u16"])
def test_label_table_spills(dims, ldt, per_tile):
    assert _capi.COSIG_SLOTS < per_tile                            # every voxel its own label: a full tile holds more than the table
    V = rt.permutation_labels(dims, ldt, 43)
    A, B = image(dims, np.uint16, 44), image(dims, np.uint8, 45)
    plan = rt.plan(dims, 0, np.dtype(ldt).itemsize, "signal")
    assert plan.per == 1 and plan.groups == 5 and 2 * 4 * rt.columns(np.dtype(ldt).itemsize) == per_tile
    with Pass(V) as p:
        p.extract()
        p.set_signal(A)
        set_b(p, B)
        debug, _ = check_pass(p, A, B, (30000, 100))
        assert debug["spills"] > 0
        assert debug["spills"] >= 4 * (per_tile - _capi.COSIG_SLOTS)      # (what no hash can avoid in the four full tiles)


# ---- 6. more than one tile a workgroup -------------------------------------------------------------------------------------------
def test_two_tiles_a_workgroup():
    dims = (1, 4 * _capi.COSIG_MAX_GROUPS + 4, 8)
    V = rt.block_labels(dims, np.uint16, 46, nlabels=200, block=(1, 7, 3))
    A, B = image(dims, np.uint8, 47), image(dims, np.uint16, 48)
    with Pass(V) as p:
        p.extract()
        p.set_signal(A)
        set_b(p, B)
        debug, _ = check_pass(p, A, B, (100, 30000))
        assert debug["tiles_per_group"] == 2 and p.ctx._debug_words(p.ctx._lib.ta_cosignal_debug)[2] == 2


# ---- 7. thresholds ---------------------------------------------------------------------------------------------------------------
def test_thresholds():
    V = rt.block_labels((18, 6, 40), np.uint16, 49, nlabels=25)
    A, B8 = image(V.shape, np.uint16, 50), image(V.shape, np.uint8, 51)
    B16 = image(V.shape, np.uint16, 52).copy()
    B16[0, 0, :4] = 65535                                          # the largest value is present, and is not over 65535
    thresholded = ("n_a", "n_b", "n_ab", "sum_a_over", "sum_b_over")
    with Pass(V) as p:
        p.extract()
        p.set_signal(A)
        set_b(p, B16)
        _, zero = check_pass(p, A, B16, (0, 0))
        assert np.array_equal(zero["n_b"] + np.bincount(V[B16 == 0], minlength=zero["n"].size).astype(np.uint64), zero["n"])
        _, half = check_pass(p, A, B16, (32767, 40000))
        assert half["n_ab"].any() and (half["n_ab"] <= half["n_a"]).all()
        _, top = check_pass(p, A, B16, (65535, 65535))
        assert all(not top[k].any() for k in thresholded) and top["sum_a"].any()
        set_b(p, B8)
        _, over = check_pass(p, A, B8, (100, 300))                 # 300 on a uint8 channel: nothing is over it
        assert not over["n_b"].any() and not over["n_ab"].any() and not over["sum_a_over"].any() and over["n_a"].any() and over["sum_b_over"].any()
        assert p.ctx.cosignal_thresholds() == (100, 300)


# ---- 8. sparse ids in a compacted context ----------------------------------------------------------------------------------------
def test_sparse_ids_compacted_context():
    rng = np.random.default_rng(5)
    ids = np.array([0, 7, 70000, 2**31 + 5, 2**32 - 2, 2**32 - 1], dtype=np.uint32)
    V = ids[rng.integers(0, ids.size, size=(12, 9, 33))]
    A, B = image(V.shape, np.uint16, 6), image(V.shape, np.uint16, 7)
    st = _run(V, A, B, (1000, 2000), sparse=True)
    assert st.ids is not None and np.array_equal(st.ids, ids.astype(np.int64)) and len(st) == ids.size      # the rows are ranks
    check_pair(st, V, A, B, (1000, 2000))
    got = st.of_labels([2**32 - 1, 7, 12345], "ratio")
    assert got[0] == st.ratio()[5] and got[1] == st.ratio()[1] and np.isnan(got[2])


# ---- 9. slabs --------------------------------------------------------------------------------------------------------------------
def test_two_slab_contexts_with_a_halo_merge_to_the_whole():
    V = c1()
    A, B = image(V.shape, np.uint16, 11), image(V.shape, np.uint8, 12)
    L = int(V.max())
    thr = (30000, 100)
    cut = 37
    parts = []
    for lo, hi, halo in ((0, cut, False), (cut - 1, V.shape[0], True)):
        tv, ta, tb = tensor(V[lo:hi]), tensor(A[lo:hi]), tensor(B[lo:hi])
        ctx = _capi.Context(0)
        try:
            ctx.set_volume_device(tv.data_ptr(), 2, tv.shape, a0_origin=lo + (1 if halo else 0), has_low_halo=halo, keep=tv)
            ctx.set_signal_device(ta.data_ptr(), 2, keep=ta)
            ctx.set_cosignal_device(tb.data_ptr(), 1, keep=tb)
            ctx.extract(_capi.F_ALL, L)
            ctx.cosignal_extract(*thr)
            cols = ctx.cosignal_rows()
            same_integers(cols, ref.labels(V[lo:hi], A[lo:hi], B[lo:hi], L + 1, *thr, first_owned=1 if halo else 0))
            parts.append(ChannelPairStats(None, cols, thr))
        finally:
            ctx.close()
    want = ref.labels(V, A, B, L + 1, *thr)
    for k in ref.COLUMNS:
        assert np.array_equal(parts[0].columns()[k] + parts[1].columns()[k], want[k]), k      # (no carry at this size)
    merged = ChannelPairStats.merge(parts)
    same_integers(merged.columns(), want)
    same_floats(merged, want)


# ---- 10. the carry ---------------------------------------------------------------------------------------------------------------
def test_the_carry_beyond_64_bits():
    """One label, more than 2^32 voxels, both channels 65535 everywhere: every sum of products is n * 65535^2 >= 2^64."""
    import torch
    dims = (1040, 2048, 2048)                                      # 4.36e9 voxels: 8.7 GB of labels + 8.7 GB of the one channel buffer
    n = dims[0] * dims[1] * dims[2]
    assert n > 2**32
    vol = torch.full(dims, 3, dtype=torch.int16, device="cuda")
    sig = torch.full(dims, -1, dtype=torch.int16, device="cuda")      # 0xFFFF; A and B are this one buffer
    torch.cuda.synchronize()
    ctx = _capi.Context(0)
    try:
        ctx.set_volume_device(vol.data_ptr(), 2, dims, keep=vol)
        ctx.set_signal_device(sig.data_ptr(), 2, keep=sig)
        ctx.set_cosignal_device(sig.data_ptr(), 2, keep=sig)
        ctx.extract(_capi.F_VOLUME, 3)
        ctx.cosignal_extract(0, 0)
        cols = ctx.cosignal_rows()
    finally:
        ctx.close()
        del vol, sig
        torch.cuda.empty_cache()
    want = n * 65535 * 65535
    assert want >= 2**64
    st = ChannelPairStats(None, cols)
    for k in ref.WIDE:
        assert int(cols[k][3, 1]) == want >> 64 and st.sq_int(k, 3) == want, k
    assert int(cols["n"][3]) == n and int(cols["n_ab"][3]) == n and int(cols["n_a"][3]) == n and int(cols["n_b"][3]) == n
    assert int(cols["sum_a"][3]) == int(cols["sum_b"][3]) == int(cols["sum_a_over"][3]) == int(cols["sum_b_over"][3]) == n * 65535
    assert all(not cols[k][:3].any() for k in ref.COLUMNS)


# ---- 11. invalidation and errors ---------------------------------------------------------------------------------------------------
def test_what_makes_the_rows_stale():
    V = rt.block_labels((24, 20, 70), np.uint16, 31, nlabels=40)
    A, B = image(V.shape, np.uint8, 2), image(V.shape, np.uint16, 3)
    getters = lambda ctx: (ctx.cosignal_rows, ctx.cosignal_debug, ctx.cosignal_thresholds)
    stale = [_capi.TA_EINVAL] * 3
    with Pass(V) as p:
        assert code(p.ctx.cosignal_timing) == _capi.TA_EINVAL and [code(g) for g in getters(p.ctx)] == stale
        p.extract()
        assert code(p.ctx.cosignal_extract) == _capi.TA_EINVAL         # neither A nor B
        set_b(p, B)
        assert code(p.ctx.cosignal_extract) == _capi.TA_EINVAL         # no A
        p.set_signal(A)
        check_pass(p, A, B, (10, 20))
        p.ctx.relabel(np.arange(p.max_label + 1, dtype=np.uint32))      # ta_volume_relabel
        assert [code(g) for g in getters(p.ctx)] == stale
        assert code(p.ctx.cosignal_extract) == _capi.TA_EINVAL         # no extraction of the current volume
        p.extract()
        check_pass(p, A, B, (10, 20))
        p.extract()                                                     # a new extraction, even of the same volume
        assert [code(g) for g in getters(p.ctx)] == stale
        check_pass(p, A, B)
        p.set_signal(A)                                                 # a new A, even the same voxels
        assert [code(g) for g in getters(p.ctx)] == stale
        check_pass(p, A, B)
        set_b(p, B)                                                     # a new B
        assert [code(g) for g in getters(p.ctx)] == stale
        check_pass(p, A, B, (3, 4))                                     # a fresh pass answers again
        p.ctx.set_volume(V)                                             # a new volume of the same dims: A and B stay
        assert [code(g) for g in getters(p.ctx)] == stale
        p.extract()
        check_pass(p, A, B)
        W = np.ascontiguousarray(V[:, :, :64])                          # a new volume of other dims drops both
        p.ctx.set_volume(W)
        p.V = W
        p.extract()
        assert code(p.ctx.cosignal_extract) == _capi.TA_EINVAL
        p.set_signal(np.ascontiguousarray(A[:, :, :64]))
        assert code(p.ctx.cosignal_extract) == _capi.TA_EINVAL         # A fits again, B is gone
        with pytest.raises(ValueError):
            p.ctx.set_cosignal(B)                                       # a B of other dims
        # ... which the library refuses too, and no B is set by it
        rc = p.ctx._lib.ta_cosignal_set(p.ctx._h, B.ctypes.data, 2, (_capi._i64 * 3)(*B.shape), (_capi._i64 * 3)(*B.strides))
        assert rc == _capi.TA_EINVAL and code(p.ctx.cosignal_extract) == _capi.TA_EINVAL
        set_b(p, np.ascontiguousarray(B[:, :, :64]))
        check_pass(p, np.ascontiguousarray(A[:, :, :64]), np.ascontiguousarray(B[:, :, :64]))


def test_signal_pair_argument_errors():
    V = rt.block_labels((10, 12, 16), np.uint16, 32, nlabels=10)
    A, B = image(V.shape, np.uint8, 4), image(V.shape, np.uint16, 5)
    rv = ResidentVolume(V)
    try:
        rv.extract()
        with pytest.raises(TypeError, match="uint8 or uint16"):
            rv.signal_pair(A, B.astype(np.float32))
        with pytest.raises(TypeError, match="uint8 or uint16"):
            rv.signal_pair(A.astype(np.float32), B)
        with pytest.raises(ValueError):
            rv.signal_pair(A, B[:, :, :-1])
        with pytest.raises(ValueError):
            rv.signal_pair(A[:, :-1], B)
        with pytest.raises(ValueError):
            rv.signal_pair(A, B, (0, -1))
        check_pair(rv.signal_pair(A, B, (1, 2)), V, A, B, (1, 2))
    finally:
        rv.close()


# ---- 12. the analysis methods and the graph ----------------------------------------------------------------------------------------
def test_analysis_methods_and_graph():
    V = np.array(c1())
    A, B = image(V.shape, np.uint16, 12), image(V.shape, np.uint16, 13)
    img = SpatialImage(V, voxelsize=(0.5, 0.25, 2.0))
    thr = (30000, 20000)
    f0 = ref.floats(ref.labels(V, A, B, int(V.max()) + 1))
    ft = ref.floats(ref.labels(V, A, B, int(V.max()) + 1, *thr))
    for rt_ in (DICT, LIST, NPLIST):
        sia = SpatialImageAnalysis(img, ignoredlabels=0, return_type=rt_, background=1)
        labels = sia.labels()
        values = lambda got: np.array([got[l] for l in labels]) if rt_ == DICT else np.asarray(got)
        np.testing.assert_allclose(values(sia.signal_ratio(A, B)), f0["ratio"][labels], rtol=1e-12, atol=0)
        np.testing.assert_allclose(values(sia.signal_correlation(A, B)), f0["pearson"][labels], rtol=1e-12, atol=0)
        assert sia._channel_pair(A, B) is sia._channel_pair(A, B)                      # cached per pair of arrays and thresholds
        coloc = values(sia.signal_colocalisation(A, B, thr))
        assert coloc.shape == (len(labels), 2)
        np.testing.assert_allclose(coloc[:, 0], ft["manders_m1"][labels], rtol=1e-12, atol=0)
        np.testing.assert_allclose(coloc[:, 1], ft["manders_m2"][labels], rtol=1e-12, atol=0)
        assert sia._resident().uploads == 1                                            # exactly one upload of the labels
    # the graph: the columns are the methods' values; without reference_signal the two properties are absent
    sia = SpatialImageAnalysis(img, ignoredlabels=0, return_type=DICT, background=1)
    g = graph_from_image(sia, background=1, spatio_temporal_properties=["volume", "signal_ratio", "signal_correlation"], signal=A,
                         reference_signal=B, ignore_cells_at_stack_margins=False)
    ids = np.asarray(g.vertex_ids)
    ratio, valid = g.vertex_column("signal_ratio")
    corr, cvalid = g.vertex_column("signal_correlation")
    assert valid.any() and np.array_equal(valid, cvalid)
    want_ratio, want_corr = sia.signal_ratio(A, B), sia.signal_correlation(A, B)
    assert np.array_equal(ratio[valid], np.array([want_ratio[l] for l in ids[valid].tolist()]))
    assert np.array_equal(corr[valid], np.array([want_corr[l] for l in ids[valid].tolist()]))
    assert "volume" in g.vertex_property_names()
    plain = graph_from_image(sia, background=1, spatio_temporal_properties=["volume", "signal_ratio", "signal_correlation"], signal=A,
                             ignore_cells_at_stack_margins=False)
    assert "signal_ratio" not in plain.vertex_property_names() and "signal_correlation" not in plain.vertex_property_names()
    assert "volume" in plain.vertex_property_names()
    assert sia._resident().uploads == 1
