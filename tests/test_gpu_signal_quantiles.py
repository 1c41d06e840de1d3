"""Signal histograms and order statistics on the GPU (include/tissue_scan_sighist.h, csrc/kernels_sighist.hip) against
tests/sighist_reference.py: every table bit for bit, the host's float results against numpy.

The shapes are the smallest at which the pass can still go wrong: rows that are whole 16-byte strips of labels and rows that are
not (61, 70 columns), planes that are no whole tiles, several tiles and workgroups, a range of two tiles a workgroup, axes of one
voxel, one voxel, more keys than a workgroup's LDS table has slots, and buffers off a 16-byte boundary."""
import ctypes
import functools
import os

import numpy as np
import pytest

import range_tiles as rt
import sighist_reference as ref
from feature_passes import A0_ORIGIN, Pass, code, poke
from tissue_analysis_amd import DICT, LIST, NPLIST, SignalHistogram, SignalQuantiles, SpatialImageAnalysis, _capi, synth
from tissue_analysis_amd.extraction import ResidentVolume
from tissue_analysis_amd.graph_from_image import graph_from_image

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDTHS = {1: (0, 8), 2: (8, 16)}                             # narrowest and widest log2_width by the signal's item size


@functools.lru_cache(maxsize=None)
def voronoi(shape, cells, seed=3):
    v = synth.voronoi_labels(shape, cells, seed, dtype=np.uint16)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def signal(shape, dtype, seed=8):
    s = rt.random_image(shape, dtype, seed)
    s.setflags(write=False)
    return s


def check(ctx, V, S, nrows, rows=None, first_owned=0, ranks=True, counting=False):
    """Both passes over what the context holds, against the reference of (V, S): the histogram at the narrowest and the widest bins,
    then the ranks 0, floor and ceil of (n - 1) / 2, n - 1 and n of every row.  Returns the diagnostics of the last histogram pass."""
    n = None
    for w in WIDTHS[S.dtype.itemsize]:
        ctx.sighist_extract(w)
        got = ctx.sighist_get()
        want = ref.histogram(V, S, nrows, w, rows, first_owned)
        assert got.shape == want.shape and got.dtype == np.uint64 and np.array_equal(got, want), w
        n = got.sum(axis=1)
    debug = ctx.sighist_debug()
    ms_hist, _ = ctx.sighist_timing()
    assert ms_hist >= 0.0
    assert int(n.sum()) == np.asarray(V)[first_owned:].size
    if ranks:
        wanted = ref.standard_ranks(n)
        ctx.sigrank_extract(wanted)
        got = ctx.sigrank_get()
        order = ref.order_statistics_by_counting if counting else ref.order_statistics
        want = order(V, S, nrows, wanted, rows, first_owned)
        assert got.dtype == np.uint32 and np.array_equal(got, want)
        assert (got[:, 4] == _capi.SIGRANK_NONE).all() and (got[n > 0, :4] != _capi.SIGRANK_NONE).all()
        assert ctx.sighist_timing()[1] >= 0.0
        again = ctx.sighist_debug()
        assert (again["tiles_per_group"], again["groups"]) == (debug["tiles_per_group"], debug["groups"])
    return debug


def run(V, S, adopted=False, **kw):
    with Pass(V, adopted=adopted) as p:
        p.extract(features=_capi.F_VOLUME)
        p.set_signal(S)
        return check(p.ctx, V, S, p.max_label + 1, **kw)


# ---- 1. adversarial and Voronoi volumes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdtype", [np.uint8, np.uint16])
def test_adversarial_golden_volumes(sdtype):
    z = np.load(os.path.join(GOLD, "adversarial_small.npz"))
    for i, name in enumerate(sorted(set(k.split("__")[0] for k in z.files))):
        V = z[name + "__volume"]
        run(V, rt.random_image(V.shape, sdtype, i))


@pytest.mark.parametrize("ldtype", [np.uint16, np.uint32])
@pytest.mark.parametrize("sdtype", [np.uint8, np.uint16])
def test_voronoi_whole_strips_and_ragged_rows(ldtype, sdtype):
    c = synth.CONFIGS["C1"]
    V = voronoi(c["dims"], c["n_cells"], c["seed"]).astype(ldtype)
    run(V, signal(V.shape, sdtype))
    Vo = np.ascontiguousarray(V[:40, :50, :61])                    # rows of 61 columns: the edge path
    run(Vo, signal(Vo.shape, sdtype, 9))


# ---- 2. the ends of the contention range --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 6, 70), (8, 16, 512)])
@pytest.mark.parametrize("sdtype,value", [(np.uint8, 0), (np.uint8, 255), (np.uint16, 0), (np.uint16, 255), (np.uint16, 65535)])
def test_constant_signal_over_a_uniform_volume(shape, sdtype, value):
    """Every lane of every wave on one counter."""
    V = np.full(shape, 2, dtype=np.uint16)
    S = np.full(shape, value, dtype=sdtype)
    with Pass(V) as p:
        p.extract(features=_capi.F_VOLUME)
        p.set_signal(S)
        check(p.ctx, V, S, 3)
        p.ctx.sighist_extract(WIDTHS[S.dtype.itemsize][0])
        counts = p.ctx.sighist_get()
        assert int(counts[2, value >> WIDTHS[S.dtype.itemsize][0]]) == V.size and int(counts.sum()) == V.size
        mid = (V.size - 1) // 2
        p.ctx.sigrank_extract(np.array([[0, 0], [0, 0], [mid, mid + (V.size - 1) % 2]], dtype=np.uint64))
        assert p.ctx.sigrank_get().tolist() == [[_capi.SIGRANK_NONE] * 2] * 2 + [[value, value]]


@pytest.mark.parametrize("axis", [2, 0])
@pytest.mark.parametrize("sdtype", [np.uint8, np.uint16])
def test_ramp_signal(axis, sdtype):
    """Along axis 2 the digit changes with the lane, along axis 0 only with the plane."""
    shape = (40, 9, 600)
    V = voronoi(shape, 25)
    step = 1 if sdtype == np.uint8 else 97
    index = np.arange(shape[axis], dtype=np.int64) * step % (np.iinfo(sdtype).max + 1)
    S = np.broadcast_to(index.reshape([-1 if a == axis else 1 for a in range(3)]), shape).astype(sdtype)
    run(V, S)


# ---- 3. selectors -------------------------------------------------------------------------------------------------------------
def test_selectors_of_the_second_pass():
    """Label 1: every value in high byte 0x42.  Label 2: spread over all 256 high bytes.  Label 3: half its voxels in high byte 0,
    half in 255, and ranks asked on both sides; all eight ranks of label 1 share one selector, label 2's fall into eight."""
    rng = np.random.default_rng(17)
    shape = (12, 10, 128)
    V = rng.integers(1, 3, size=shape, endpoint=True).astype(np.uint16)
    S = np.zeros(shape, dtype=np.uint16)
    m1, m2, m3 = V == 1, V == 2, V == 3
    S[m1] = 0x4200 + rng.integers(0, 255, size=int(m1.sum()), endpoint=True)
    S[m2] = rng.permutation(int(m2.sum())) * 65536 // int(m2.sum())
    side = rng.integers(0, 1, size=int(m3.sum()), endpoint=True)
    S[m3] = np.where(side == 1, 0xFF00, 0) + rng.integers(0, 255, size=int(m3.sum()), endpoint=True)
    n = np.bincount(V.reshape(-1), minlength=4).astype(np.uint64)
    ranks = np.zeros((4, 8), dtype=np.uint64)
    ranks[0] = ref.NO_RANK
    ranks[1] = (np.arange(8, dtype=np.uint64) * (n[1] - np.uint64(1))) // np.uint64(7)
    ranks[2] = (np.arange(8, dtype=np.uint64) * (n[2] - np.uint64(1))) // np.uint64(7)
    zeros, n3 = int((S[m3] < 256).sum()), int(n[3])
    ranks[3] = [0, zeros - 1, zeros, n3 - 1, zeros // 2, zeros + 1, 1, n3 - 2]
    want, selectors = ref.two_pass_select(V, S, 4, ranks)
    assert [len(s) for s in selectors] == [0, 1, 8, 2] and sorted(selectors[3]) == [0, 255]
    assert np.array_equal(want, ref.order_statistics(V, S, 4, ranks))
    with Pass(V) as p:
        p.extract(features=_capi.F_VOLUME)
        p.set_signal(S)
        p.ctx.sigrank_extract(ranks)
        assert np.array_equal(p.ctx.sigrank_get(), want)
        check(p.ctx, V, S, 4)


# ---- 4. thin volumes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 77), (5, 1, 64), (1, 9, 40)])
@pytest.mark.parametrize("sdtype", [np.uint8, np.uint16])
def test_thin_volumes(shape, sdtype):
    V = (np.arange(int(np.prod(shape))).reshape(shape) // 7 % 5).astype(np.uint16)
    run(V, signal(shape, sdtype, 5))


# ---- 5. ranges of tiles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldtype,vector,sdtype", [(np.uint16, True, np.uint8), (np.uint32, False, np.uint16)], ids=["u16-vector-s8", "u32-edge-s16"])
def test_a_range_of_two_tiles_a_workgroup(ldtype, vector, sdtype):
    """The smallest dims at which the plan takes two tiles a workgroup, on both load paths; the order statistics of this many voxels
    come from the full-resolution histogram."""
    dims = ref.two_tile_dims(np.dtype(ldtype).itemsize, vector)
    plan = ref.plan(dims, 0, np.dtype(ldtype).itemsize)
    assert plan.per == 2 and plan.tiles > ref.MAX_GROUPS and rt.vector_path(dims, np.dtype(ldtype).itemsize) == vector
    V = rt.block_labels(dims, ldtype, 23, nlabels=60, block=(37, 29, 3))
    S = rt.random_image(dims, sdtype, 24)
    debug = run(V, S, counting=True)
    assert (debug["tiles_per_group"], debug["groups"]) == (plan.per, plan.groups)


def test_the_plan_of_small_volumes():
    for shape, ldtype in (((40, 9, 600), np.uint16), ((33, 9, 70), np.uint32)):
        V = voronoi(shape, 25).astype(ldtype)
        debug = run(V, signal(shape, np.uint8))
        plan = ref.plan(shape, 0, np.dtype(ldtype).itemsize)
        assert plan.per == 1 and (debug["tiles_per_group"], debug["groups"]) == (1, plan.tiles)


# ---- 6. more keys than slots --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdtype", [np.uint8, np.uint16])
def test_more_keys_than_a_workgroup_has_slots(sdtype):
    """A permutation volume of one tile and one workgroup: 4096 labels.  Whatever the hash does, at least 4096 - slots of them find
    no slot, and each hands over at least one count (pigeonhole, as in test_gpu_feature_table_spills.py)."""
    V = rt.permutation_labels(rt.SPILL_DIMS, np.uint16, 21)
    S = signal(V.shape, sdtype)
    with Pass(V) as p:
        p.extract(features=_capi.F_VOLUME)
        p.set_signal(S)
        debug = check(p.ctx, V, S, p.max_label + 1)
        assert (debug["tiles_per_group"], debug["groups"]) == (1, 1)
        assert debug["spills"] >= 4096 - _capi.SIGHIST_SLOTS > 0
        assert p.ctx.sighist_debug()["spills"] >= (4096 - _capi.SIGHIST_SLOTS if sdtype == np.uint16 else 0)      # the select's last pass


# ---- 7. layouts and buffers ---------------------------------------------------------------------------------------------------
def test_layouts():
    shape = (24, 40, 56)
    V = voronoi(shape, 30)
    S = signal(shape, np.uint16)
    for A, B in ((np.asfortranarray(V), np.asfortranarray(S)),
                 (np.asfortranarray(V), S),
                 (np.ascontiguousarray(V.transpose(1, 2, 0)).transpose(2, 0, 1), np.ascontiguousarray(S.transpose(2, 0, 1)).transpose(1, 2, 0))):
        rv = ResidentVolume(A)
        try:
            x = rv.extract(_capi.F_VOLUME, sparse=False)
            rv.ctx.set_signal(B)                              # (stored in another permutation than the labels: copied into theirs)
            check(rv.ctx, V, S, x.nrows)                      # the tables do not depend on the walk: array axes do for the reference
        finally:
            rv.close()


@pytest.mark.parametrize("dtype,offsets", [(np.uint16, (0, 1, 4)), (np.uint32, (0, 1, 2))], ids=["u16", "u32"])
@pytest.mark.parametrize("sdtype,sbytes", [(np.uint8, 1), (np.uint16, 2), (np.uint16, 8)], ids=["s8+1B", "s16+2B", "s16+8B"])
def test_adopted_buffers_off_a_16_byte_boundary(dtype, offsets, sdtype, sbytes):
    from test_gpu_unaligned_buffers import adopt, offset_view, signal_image
    shape = (19, 7, 528)
    V = voronoi(shape, 60).astype(dtype)
    S = signal_image(shape, sdtype, 7)
    rows = int(V.max()) + 2                                   # a row for the sentinel of the pads too: it must stay empty
    for off in offsets:                                       # offset 0 is the aligned control (of the labels)
        ctx = _capi.Context(0)
        try:
            ov = adopt(ctx, V, off)
            sv = offset_view(S, sbytes // np.dtype(sdtype).itemsize, 5)
            assert sv.dev_ptr % 16 == sbytes
            ctx.set_signal_device(sv.dev_ptr, np.dtype(sdtype).itemsize, keep=sv.flat)
            ctx.extract(_capi.F_VOLUME, rows - 1)
            check(ctx, V, S, rows)
            ov.read_back()
            sv.read_back()
        finally:
            ctx.close()


def test_two_dimensional_image():
    V = synth.voronoi_labels((1, 200, 150), 40, 3, np.uint16)[0]
    S = signal(V.shape, np.uint16, 4)
    rv = ResidentVolume(V)
    try:
        x = rv.extract()
        h = rv.signal_histogram(S)
        assert isinstance(h, SignalHistogram) and np.array_equal(h.counts, ref.histogram(V, S, x.nrows, 8)) and h.bin_width == 256
        check(rv.ctx, V, S, x.nrows)
    finally:
        rv.close()


# ---- 8. sparse ids ------------------------------------------------------------------------------------------------------------
def test_sparse_ids_compacted_context():
    rng = np.random.default_rng(5)
    ids = np.array([0, 7, 70000, 2**31 + 5, 2**32 - 2, 2**32 - 1], dtype=np.uint32)
    V = ids[rng.integers(0, ids.size, size=(12, 9, 33))]
    S = signal(V.shape, np.uint16, 6)
    rows = np.searchsorted(ids, V)
    rv = ResidentVolume(V)
    try:
        x = rv.extract(sparse=True)
        assert rv.ctx.is_compact() and np.array_equal(x.ids, ids.astype(np.int64))
        rv.ctx.set_signal(S)
        check(rv.ctx, V, S, ids.size, rows=rows)
        q = rv.signal_quantiles(S, [0.0, 0.5, 1.0])
        assert isinstance(q, SignalQuantiles) and np.array_equal(q.ids, ids.astype(np.int64))
        for i, l in enumerate(ids.tolist()):
            assert np.array_equal(q.of_labels([l])[0], np.quantile(S[V == l].astype(np.float64), [0.0, 0.5, 1.0]))
        assert np.isnan(q.of_labels([5])).all()
    finally:
        rv.close()


# ---- 9. slabs -----------------------------------------------------------------------------------------------------------------
def test_two_slab_contexts_with_a_halo_sum_to_the_whole():
    c = synth.CONFIGS["C1"]
    V = voronoi(c["dims"], c["n_cells"], c["seed"])
    S = signal(V.shape, np.uint16, 11)
    L = int(V.max())
    cut = 37
    total = 0
    for lo, halo in ((0, 0), (cut - 1, 1)):
        part, spart = np.ascontiguousarray(V[lo:cut] if not halo else V[lo:]), np.ascontiguousarray(S[lo:cut] if not halo else S[lo:])
        with Pass(part, first_owned=halo, adopted=True) as p:
            p.extract(max_label=L, features=_capi.F_VOLUME)
            p.set_signal(spart)
            check(p.ctx, part, spart, L + 1, first_owned=halo, ranks=not halo)
            p.ctx.sighist_extract(8)
            total = total + p.ctx.sighist_get()
            if halo:
                assert p.origin == A0_ORIGIN
                assert code(p.ctx.sigrank_extract, np.zeros((L + 1, 1), dtype=np.uint64)) == _capi.TA_EINVAL
                assert code(p.ctx.sigrank_get) == _capi.TA_EINVAL
    assert np.array_equal(total, ref.histogram(V, S, L + 1, 8))


def test_a_slab_without_a_halo_but_off_the_origin_has_no_order_statistics():
    from feature_passes import tensor
    V = voronoi((20, 12, 64), 9)
    S = signal(V.shape, np.uint8)
    ctx = _capi.Context(0)
    try:
        tv, ts = tensor(V), tensor(S)
        ctx.set_volume_device(tv.data_ptr(), 2, V.shape, a0_origin=5, has_low_halo=False, keep=tv)
        ctx.set_signal_device(ts.data_ptr(), 1, keep=ts)
        ctx.extract(_capi.F_VOLUME, int(V.max()))
        check(ctx, V, S, int(V.max()) + 1, ranks=False)
        assert code(ctx.sigrank_extract, np.zeros((int(V.max()) + 1, 1), dtype=np.uint64)) == _capi.TA_EINVAL
    finally:
        ctx.close()


# ---- 10. invalidation and errors ----------------------------------------------------------------------------------------------
def test_invalidation_and_argument_checks():
    shape = (19, 7, 528)
    V = voronoi(shape, 60)
    S = signal(shape, np.uint16)
    top = int(V.max())
    ctx = _capi.Context(0)
    try:
        getters = (ctx.sighist_get, ctx.sigrank_get, ctx.sighist_debug, ctx.sighist_timing)
        ranks = (ctypes.c_uint64 * (9 * (top + 1)))()                              # room for every row count and nranks below

        def stale():
            return all(code(call) == _capi.TA_EINVAL for call in getters)

        def refused():
            return code(ctx.sighist_extract, 8) == _capi.TA_EINVAL and ctx._lib.ta_sigrank_extract(ctx._h, 1, ranks) == _capi.TA_EINVAL

        def current(labels, rows=None, nrows=top + 1):
            check(ctx, labels, S, nrows, rows)
            assert not any(code(call) != _capi.TA_OK for call in getters)

        assert stale() and refused()                                               # no volume
        ctx.set_volume(V)
        assert refused()                                                           # no signal, no extraction
        ctx.set_signal(S)
        assert stale() and refused()                                               # no extraction
        ctx.extract(_capi.F_VOLUME, top)
        assert stale()
        for bad in (7, 17, -1):
            assert code(ctx.sighist_extract, bad) == _capi.TA_EINVAL, bad
        for bad in (0, 9, -1):
            assert ctx._lib.ta_sigrank_extract(ctx._h, bad, ranks) == _capi.TA_EINVAL, bad
        assert ctx._lib.ta_sigrank_extract(ctx._h, 1, None) == _capi.TA_EINVAL
        assert stale()
        ctx.sighist_extract(8)
        assert code(ctx.sighist_get) == _capi.TA_OK and code(ctx.sigrank_get) == _capi.TA_EINVAL      # each getter its own pass
        assert ctx.sighist_timing()[1] is None
        assert ctx._lib.ta_sighist_get(ctx._h, None) == _capi.TA_OK and ctx._lib.ta_sighist_debug(ctx._h, None) == _capi.TA_OK
        assert ctx._lib.ta_sighist_timing(ctx._h, None, None) == _capi.TA_OK
        current(V)

        ctx.set_signal(S)                                                          # a new signal
        assert stale()
        ctx.set_signal(S.astype(np.uint8))
        for bad in (9, 16):
            assert code(ctx.sighist_extract, bad) == _capi.TA_EINVAL, bad          # the range follows the signal's type
        ctx.set_signal(S)
        current(V)
        ctx.extract(_capi.F_ALL, top)                                              # a new ta_extract
        assert stale()
        current(V)
        lut = np.arange(top + 1, dtype=np.uint32)
        lut[5] = 3
        ctx.relabel(lut)                                                           # ta_volume_relabel
        assert stale() and refused()
        ctx.extract(_capi.F_VOLUME, top)
        W = lut[V].astype(np.uint16)
        current(W)
        ids = ctx.compact_labels()                                                 # compaction
        assert stale() and refused()
        ctx.extract(_capi.F_VOLUME, ids.size - 1)
        current(W, rows=np.searchsorted(ids, W), nrows=ids.size)
        ctx.rerank()                                                               # ta_volume_rerank
        assert stale() and refused()
        ctx.extract(_capi.F_VOLUME, ids.size - 1)
        current(W, rows=np.searchsorted(ids, W), nrows=ids.size)
        ctx.uncompact()                                                            # the end of compaction
        assert stale() and refused()
        ctx.extract(_capi.F_VOLUME, top)
        current(W)
        ctx.components_extract()
        comp = ctx.components_get()
        ctx.components_relabel(np.asarray(comp[0], dtype=np.uint32))               # ta_components_relabel (every blob keeps its label)
        assert stale() and refused()
        ctx.extract(_capi.F_VOLUME, top)
        current(W)
        ctx.set_volume(V)                                                          # a new volume (of the same dims: the signal stays)
        assert stale() and refused()
        ctx.extract(_capi.F_VOLUME, top)
        current(V)
        ctx.set_volume(V[:, :, :64].copy())                                        # ... of other dims: the signal is dropped
        ctx.extract(_capi.F_VOLUME, top)
        assert stale() and refused()
    finally:
        ctx.close()


def test_more_keys_than_the_tables_index():
    V = np.ones((2, 3, 8), dtype=np.uint32)
    S = np.zeros(V.shape, dtype=np.uint8)
    ctx = _capi.Context(0)
    try:
        ctx.set_volume(V)
        ctx.set_signal(S)
        ctx.extract(_capi.F_VOLUME, (1 << 22))                                     # R = 2^22 + 1: R x 256 fits, R x 2 x 256 does not
        ctx.sighist_extract(8)
        assert int(ctx.sighist_get()[1, 0]) == V.size
        ranks = (ctypes.c_uint64 * (2 * ((1 << 22) + 1)))()
        assert ctx._lib.ta_sigrank_extract(ctx._h, 2, ranks) == _capi.TA_EINVAL
        assert ctx._lib.ta_sigrank_extract(ctx._h, 1, ranks) == _capi.TA_OK
        assert code(ctx.sighist_debug) == _capi.TA_OK
        ctx.extract(_capi.F_VOLUME, (1 << 23))                                     # R x 256 > 2^31
        assert code(ctx.sighist_extract, 8) == _capi.TA_EINVAL
        assert ctx._lib.ta_sigrank_extract(ctx._h, 1, ranks) == _capi.TA_EINVAL
    finally:
        ctx.close()


def test_a_label_above_max_label():
    V = rt.block_labels((24, 20, 70), np.uint16, 31, nlabels=40)
    S = signal(V.shape, np.uint16)
    with Pass(V, adopted=True) as p:
        p.extract(features=_capi.F_VOLUME)
        p.set_signal(S)
        check(p.ctx, V, S, p.max_label + 1)
        poke(p.t, (3, 4, 5), 65535)                            # 65535 * 256 + digit is far outside the tables
        p.ctx.sighist_extract(8)
        p.ctx.sigrank_extract(np.zeros((p.max_label + 1, 2), dtype=np.uint64))
        for get in (p.ctx.sighist_get, p.ctx.sigrank_get, p.ctx.sighist_debug):
            assert code(get) == _capi.TA_ERANGE
        poke(p.t, (3, 4, 5), V[3, 4, 5])
        assert code(p.ctx.sighist_get) == _capi.TA_ERANGE      # the results of that pass stay what they are
        check(p.ctx, V, S, p.max_label + 1)                    # the volume as it was: the context works on


# ---- 11. the public API, end to end -------------------------------------------------------------------------------------------
def values_of(V, S, label):
    return S[V == label].astype(np.float64)


@pytest.mark.parametrize("sdtype", [np.uint8, np.uint16])
def test_public_api(sdtype):
    c = synth.CONFIGS["C1"]
    V = voronoi(c["dims"], c["n_cells"], c["seed"])
    S = signal(V.shape, sdtype, 12)
    q = [0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0]                  # 14 ranks a row: two batches
    width = 1 if sdtype == np.uint8 else 256
    for rt_ in (DICT, LIST, NPLIST):
        sia = SpatialImageAnalysis(V, ignoredlabels=0, return_type=rt_, background=1)
        known = sorted(sia.labels())
        pick = [known[3], known[10], known[-1]]
        for labels in (None, pick + [100000]):                     # (an id the image does not hold is dropped, as by volume())
            asked = sia.labels() if labels is None else pick
            med = sia.signal_median(S, labels)
            qs = sia.signal_quantiles(S, q, labels)
            low = sia.signal_quantiles(S, q, labels, method="lower")
            hist = sia.signal_histogram(S, labels)
            assert len(med) == len(asked) and len(qs) == len(asked) and len(hist) == len(asked)
            if rt_ == DICT:
                assert list(med) == asked and list(qs) == asked and list(hist) == asked
            if rt_ == LIST:
                assert isinstance(med, list) and isinstance(qs, list) and isinstance(hist, list)
            for i, l in enumerate(asked):
                at = l if rt_ == DICT else i
                vals = values_of(V, S, l)
                assert med[at] == np.median(vals)
                np.testing.assert_allclose(np.asarray(qs[at]), np.quantile(vals, q), rtol=1e-12, atol=0)
                assert np.array_equal(np.asarray(low[at]), np.quantile(vals, q, method="lower"))
                assert np.array_equal(np.asarray(hist[at]).astype(np.int64), np.bincount(vals.astype(np.int64) // width, minlength=256))
    assert sia._resident().uploads == 1
    with pytest.raises(ValueError):
        sia.signal_quantiles(S, [0.5], method="nearest")
    with pytest.raises(ValueError):
        sia.signal_quantiles(S, [1.5])
    with pytest.raises(ValueError):
        sia.signal_histogram(S, bin_width=3)
    with pytest.raises(TypeError, match="uint8 or uint16"):
        sia.signal_median(S.astype(np.float32))
    wide = sia.signal_histogram(S, pick[:1], bin_width=width * 64)
    assert np.asarray(wide[0]).tolist() == np.bincount(values_of(V, S, pick[0]).astype(np.int64) // (width * 64), minlength=4).tolist()
    h = sia._resident_rows().signal_histogram(S, width * 64)
    assert h.edges.tolist() == [0, width * 64, width * 128, width * 192, width * 256]
    np.testing.assert_array_equal(h.fraction_above_of(pick[:2], width * 128),
                                  [(values_of(V, S, l) >= width * 128).mean() for l in pick[:2]])
    with pytest.raises(ValueError):
        h.fraction_above(width * 128 + 1)


def test_graph_property_median_signal():
    c = synth.CONFIGS["C1"]
    V = voronoi(c["dims"], c["n_cells"], c["seed"])
    S = signal(V.shape, np.uint16, 12)
    sia = SpatialImageAnalysis(V, ignoredlabels=0, return_type=DICT, background=1)
    g = graph_from_image(sia, background=1, spatio_temporal_properties=["volume", "mean_signal", "median_signal"], signal=S,
                         ignore_cells_at_stack_margins=False)
    med, valid = g.vertex_column("median_signal")
    assert valid.any() and "mean_signal" in g.vertex_property_names()
    for vid, v, ok in zip(g.vertex_ids.tolist(), med.tolist(), valid.tolist()):
        if ok:
            assert v == np.median(values_of(V, S, vid))
    plain = graph_from_image(V, background=1, spatio_temporal_properties=["volume", "median_signal"])
    assert "median_signal" not in plain.vertex_property_names()
