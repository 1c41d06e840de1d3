"""Oriented extents on the MI355X (include/tissue_scan_extents.h, csrc/kernels_extents.hip) against the restatement of
tests/extent_reference.py: lo and hi of every row bit for bit -- no tolerance: a minimum does not depend on the order of the voxels
and the arithmetic of one projection is pinned --, the launch plan the device reports equal to the restated one, and the methods of
`SpatialImageAnalysis` on top."""
import functools

import numpy as np
import pytest

import extent_reference as ref
import range_tiles as rt
from feature_passes import Pass, code, poke
from tissue_analysis_amd import DICT, NPLIST, CellExtents, SpatialImage, SpatialImageAnalysis, _capi, synth
from tissue_analysis_amd.extraction import ResidentVolume
from tissue_analysis_amd.graph_from_image import graph_from_image

pytestmark = pytest.mark.gpu


def same_rows(got, want):
    """(lo, hi) of the library against ref.rows(): equal as numbers and as bit patterns (the sign of a zero included)."""
    for name, g, w in zip(("lo", "hi"), got, want):
        assert g.shape == w.shape and g.dtype == np.float64, name
        assert np.array_equal(g, w), name
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), name + " (bits)"


def check_pass(p, w):
    """Run the pass on the context of p (a feature_passes.Pass with an extraction) with the table w: rows against the
    restatement, the plan the device reports against the restated one.  Returns (debug, (lo, hi) of the restatement)."""
    p.ctx.extents_extract(w)
    debug = p.ctx.extents_debug()
    plan = ref.plan(p.V.shape, p.V.dtype.itemsize)
    assert (debug["tiles_per_group"], debug["groups"]) == (plan.per, plan.groups), (debug, plan)
    want = ref.rows(p.V, w)
    same_rows(p.ctx.extents_rows(), want)
    assert p.ctx.extents_timing() >= 0
    return debug, want


def run_case(V, seed, **kw):
    with Pass(V) as p:
        p.extract()
        return check_pass(p, ref.weights(p.max_label + 1, seed, **kw))


# ---- 1. one tile, partial tiles, tile ranges ---------------------------------------------------------------------------------------
def test_one_tile_one_workgroup():
    V = rt.block_labels(rt.SPILL_DIMS, np.uint16, 11)            # (the volume on which a fused evaluation differs: test_cell_extents_cpu)
    debug, (lo, hi) = run_case(V, 12)
    assert (debug["tiles_per_group"], debug["groups"], debug["spills"]) == (1, 1, 0)
    present = np.isfinite(lo[:, 0])
    assert present.sum() > 10 and np.isposinf(lo[~present]).all() and np.isneginf(hi[~present]).all()


def test_partial_tiles_and_scalar_loads():
    V = rt.block_labels(rt.SPILL_DIMS_WIDE, np.uint32, 13)
    assert not rt.vector_path(V.shape, 4)
    debug, _ = run_case(V, 14)
    assert debug["groups"] == 9 and debug["spills"] == 0


@pytest.mark.parametrize("name", ["a_u16", "b_u32_scalar", "c_u16", "c_u32_vector"])
def test_tile_ranges_with_clipped_last_groups(name):
    case = rt.CASE[name]
    V = rt.block_labels(case.dims, case.dtype, 41)
    plan = ref.plan(case.dims, case.dtype.itemsize)
    assert plan.per >= 2
    debug, _ = run_case(V, 42)
    assert debug["spills"] == 0


# ---- 2. load paths by address ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1], ids=["+0B", "+2B"])
def test_unaligned_label_buffer(off):
    from test_gpu_unaligned_buffers import SHAPE_A, offset_view
    V = rt.block_labels(SHAPE_A, np.uint16, 51, nlabels=60)
    assert rt.vector_path(SHAPE_A, 2)                             # whole strips: the address alone decides
    ctx = _capi.Context(0)
    try:
        lv = offset_view(V, off, 3)
        assert lv.dev_ptr % 16 == 2 * off
        ctx.set_volume_device(lv.dev_ptr, 2, V.shape, keep=lv.flat)
        L = int(V.max())
        ctx.extract(_capi.F_ALL, L)
        w = ref.weights(L + 1, 52)
        ctx.extents_extract(w)
        same_rows(ctx.extents_rows(), ref.rows(V, w))
        assert np.array_equal(lv.read_back().reshape(V.shape), V)
    finally:
        ctx.close()


# ---- 3. the key encoding: negatives, mixed signs, zeros -----------------------------------------------------------------------------
def test_negative_and_mixed_sign_projections():
    V = rt.block_labels((24, 20, 70), np.uint16, 31, nlabels=40)
    _, (lo, hi) = run_case(V, 32)                                 # random directions: both signs
    present = np.isfinite(lo[:, 0])
    assert ((lo[present] < 0) & (hi[present] > 0)).any() and (hi[present] < 0).any() and (lo[present] > 0).any()
    _, (lo, hi) = run_case(V, 33, sign=-1)                        # every weight negative: every projection <= 0
    assert (hi[present] <= 0).all() and (hi[present] < 0).sum() >= hi[present].size - 3
    first = int(V[0, 0, 0])                                       # the voxel at the origin projects to -0.0: handed out as +0.0
    assert not hi[first].any() and not np.signbit(hi[first]).any()
    _, (lo, hi) = run_case(V, 34, sign=1)
    assert (lo[present] >= 0).all()


def test_signed_zero_weights():
    V = rt.block_labels((24, 20, 70), np.uint16, 35, nlabels=40)
    with Pass(V) as p:
        p.extract()
        w = ref.weights(p.max_label + 1, 36)
        w[:, 0, :] = [0.0, -0.0, 0.0]                             # direction 0: every projection a zero of either sign
        w[::2, 1, 0] = -0.0                                       # direction 1: one term a signed zero
        w[1::2, 1, 2] = 0.0
        w[3, 2, :] = -0.0
        _, (lo, hi) = check_pass(p, w)
    present = np.isfinite(lo[:, 0])
    assert not lo[present, 0].any() and not hi[present, 0].any()
    assert not np.signbit(lo[present, 0]).any() and not np.signbit(hi[present, 0]).any()


# ---- 4. spills, the range flag, sparse ids -----------------------------------------------------------------------------------------
def test_more_labels_than_slots_in_one_workgroup():
    V = rt.permutation_labels(rt.SPILL_DIMS, np.uint16, 61)       # 4096 labels, one workgroup
    bound = ref.label_spill_bound(V)
    assert bound == 4096 - ref.LABEL_SLOTS
    debug, (lo, hi) = run_case(V, 62)
    assert debug["groups"] == 1 and debug["spills"] >= bound, (debug, bound)
    assert np.array_equal(lo, hi)                                 # one voxel a label


def test_a_label_above_max_label_in_an_edited_buffer():
    V = rt.block_labels((24, 20, 70), np.uint16, 31, nlabels=40)
    with Pass(V, adopted=True) as p:
        p.extract()
        w = ref.weights(p.max_label + 1, 63)
        check_pass(p, w)
        poke(p.t, (3, 4, 5), p.max_label + 1)
        p.ctx.extents_extract(w)
        for get in (p.ctx.extents_rows, p.ctx.extents_debug):
            assert code(get) == _capi.TA_ERANGE
        poke(p.t, (3, 4, 5), V[3, 4, 5])
        assert code(p.ctx.extents_rows) == _capi.TA_ERANGE        # the results of that pass stay what they are
        p.extract()
        check_pass(p, w)


def test_sparse_ids_up_to_the_top_of_uint32():
    rng = np.random.default_rng(5)
    ids = np.array([0, 7, 70000, 2**31 + 5, 2**32 - 2], dtype=np.uint32)
    V = ids[rng.integers(0, ids.size, size=(12, 9, 33))]
    rv = ResidentVolume(V)
    try:
        x = rv.extract(sparse=True)
        assert x.ids is not None and np.array_equal(x.ids, ids.astype(np.int64))
        w = ref.weights(ids.size, 64)
        rv.ctx.extents_extract(w)
        same_rows(rv.ctx.extents_rows(), ref.rows(np.searchsorted(ids, V), w))          # the rows are ranks
        e = rv.cell_extents(np.eye(3))
        assert isinstance(e, CellExtents) and len(e) == ids.size and e.ms is not None and e.ms >= 0
        got = e.of_labels([2**32 - 2, 7, 12345], "lengths")
        assert np.array_equal(got[0], e.lengths()[4]) and np.array_equal(got[1], e.lengths()[1]) and np.isnan(got[2]).all()
    finally:
        rv.close()


# ---- 5. errors and staleness of the C ABI ------------------------------------------------------------------------------------------
def test_errors_and_what_makes_the_rows_stale():
    V = rt.block_labels((24, 20, 70), np.uint16, 31, nlabels=40)
    getters = lambda ctx: (ctx.extents_rows, ctx.extents_debug)
    with Pass(V) as p:
        assert code(p.ctx.extents_timing) == _capi.TA_EINVAL and code(p.ctx.extents_rows) == _capi.TA_EINVAL     # before any extract
        w = ref.weights(int(V.max()) + 1, 65)
        assert code(p.ctx.extents_extract, w) == _capi.TA_EINVAL       # no extraction yet
        p.extract()
        assert code(p.ctx.extents_rows) == _capi.TA_EINVAL
        assert code(p.ctx.extents_extract, w[:-1]) == _capi.TA_EINVAL  # rows that are not the extraction's
        assert code(p.ctx.extents_extract, np.concatenate([w, w[:1]])) == _capi.TA_EINVAL
        for bad in (np.nan, np.inf, -np.inf, 1e306):                   # not finite; a projection could overflow
            wb = w.copy()
            wb[5, 1, 2] = bad
            assert code(p.ctx.extents_extract, wb) == _capi.TA_EINVAL
        assert code(p.ctx.extents_rows) == _capi.TA_EINVAL             # none of these left rows behind
        check_pass(p, w)
        p.ctx.relabel(np.arange(p.max_label + 1, dtype=np.uint32))     # ta_volume_relabel
        assert [code(g) for g in getters(p.ctx)] == [_capi.TA_EINVAL] * 2
        assert code(p.ctx.extents_extract, w) == _capi.TA_EINVAL
        p.extract()
        check_pass(p, w)
        p.extract()                                                    # a new extraction, even of the same volume
        assert [code(g) for g in getters(p.ctx)] == [_capi.TA_EINVAL] * 2
        check_pass(p, w)
        p.ctx.set_volume(V)                                            # a new volume
        assert [code(g) for g in getters(p.ctx)] == [_capi.TA_EINVAL] * 2
    with Pass(np.concatenate([V[:1], V]), first_owned=1) as p:         # a slab
        p.extract(max_label=int(V.max()))
        assert code(p.ctx.extents_extract, w) == _capi.TA_EINVAL


# ---- 6. through the class -----------------------------------------------------------------------------------------------------------
VS = (0.5, 0.25, 2.0)


@functools.lru_cache(maxsize=None)
def tissue():
    """A Voronoi tissue (background 1) with one cuboid cell of distinct sides cut into the background, Fortran-ordered."""
    c = synth.CONFIGS["C1"]
    V = synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], np.uint16)
    cub = int(V.max()) + 1
    V[:14, :11, :9] = 1
    V[2:11, 3:8, 4:7] = cub                                       # 9 x 5 x 3 voxels: 4.5 x 1.25 x 6.0
    V = np.asfortranarray(V)
    V.setflags(write=False)
    return V, cub


def test_lengths_and_fill_through_the_analysis():
    V, cub = tissue()
    sia = SpatialImageAnalysis(SpatialImage(V, voxelsize=VS), ignoredlabels=0, return_type=DICT, background=1)
    assert sia._resident().ctx.memory_axes() == (2, 1, 0)
    e = sia.cell_extents()
    assert isinstance(e, CellExtents) and sia.cell_extents() is e and sia.cell_extents(real=False) is not e
    # the rows of the class are those of the restatement, on the memory-order view and with the table the class made
    from tissue_analysis_amd.cell_extents import extent_weights
    want = ref.rows(np.ascontiguousarray(V.transpose(2, 1, 0)), extent_weights(e.axes, VS, (2, 1, 0)))
    present = np.isfinite(want[0][:, 0])
    assert np.array_equal(e.lo[present], want[0][present]) and np.array_equal(e.hi[present], want[1][present])
    assert np.isnan(e.lo[~present]).all() and np.isnan(e.lengths()[~present]).all()
    # the cuboid: sides times voxel size, sorted by the principal axes (major, middle, minor), and a full box
    sides = np.array([3 * 2.0, 9 * 0.5, 5 * 0.25])
    lengths = sia.cell_lengths()
    np.testing.assert_allclose(lengths[cub], sides, rtol=1e-12, atol=0)
    assert np.array_equal(sia.cell_lengths(cub), lengths[cub])
    fill = sia.box_fill()
    assert fill[cub] == 1.0
    volume = sia.volume(real=False)
    cells = [l for l in sia.labels() if l != cub and volume[l] >= 1000]       # (a sliver of a few voxels in a row is a cuboid too)
    assert len(cells) > 50 and all(0.0 < fill[l] < 1.0 for l in cells) and all(0.0 < f <= 1.0 for f in fill.values())
    np.testing.assert_allclose(sia.cell_lengths(cub, real=False), [9, 5, 3], rtol=1e-12, atol=0)
    # a chosen direction, one frame, a frame per label
    along = sia.cell_extent_along([0, 0, 1])
    np.testing.assert_allclose(along[cub], 6.0, rtol=1e-12)
    np.testing.assert_allclose(sia.cell_extent_along([1, 0, 0], real=False)[cub], 9.0, rtol=1e-12)
    frame = sia.cell_extents(np.eye(3)).of_labels([cub], "lengths")[0]
    np.testing.assert_allclose(frame, [4.5, 1.25, 6.0], rtol=1e-12)
    by_label = sia.cell_extents({cub: np.eye(3)[::-1]}).of_labels([cub], "lengths")[0]
    np.testing.assert_allclose(by_label, [6.0, 1.25, 4.5], rtol=1e-12)
    np.testing.assert_allclose(e.center()[cub], np.array([6.0, 5.0, 5.0]) * VS, rtol=1e-12)
    arr = SpatialImageAnalysis(SpatialImage(V, voxelsize=VS), ignoredlabels=0, return_type=NPLIST, background=1)
    assert np.array_equal(arr.cell_lengths(), np.array([lengths[l] for l in arr.labels()]))
    with pytest.raises(ValueError):
        sia.cell_extents([np.nan, 0.0, 1.0])


def test_extents_go_stale_with_the_image():
    V, cub = tissue()
    sia = SpatialImageAnalysis(SpatialImage(V.copy(order="K"), voxelsize=VS), ignoredlabels=0, return_type=DICT, background=1)
    before = sia.cell_extents()
    ctx = sia._resident().ctx
    ctx.extents_rows()
    victim = [l for l in sia.labels() if l != cub][0]
    sia.remove_labels_from_image([victim], verbose=False)
    assert code(ctx.extents_rows) == _capi.TA_EINVAL and code(ctx.extents_debug) == _capi.TA_EINVAL
    after = sia.cell_extents()
    assert after is not before and np.isnan(after.of_labels([victim], "lengths")).all()
    assert np.isfinite(before.of_labels([victim], "lengths")).all()
    np.testing.assert_allclose(sia.cell_lengths(cub), [6.0, 4.5, 1.25], rtol=1e-12)
    ctx.extents_rows()


def test_graph_properties():
    V, cub = tissue()
    sia = SpatialImageAnalysis(SpatialImage(V, voxelsize=VS), ignoredlabels=0, return_type=DICT, background=1)
    ctx = sia._resident().ctx
    plain = graph_from_image(sia, background=1, spatio_temporal_properties=["volume"], ignore_cells_at_stack_margins=False)
    assert "box_fill" not in plain.vertex_property_names()
    with pytest.raises(_capi.TissueScanError, match="no extent pass has been run"):
        ctx.extents_timing()
    g = graph_from_image(sia, background=1, spatio_temporal_properties=["principal_lengths", "box_fill"], ignore_cells_at_stack_margins=False)
    lengths, fill = sia.cell_lengths(), sia.box_fill()
    got_l, valid_l = g.vertex_column("principal_lengths")
    got_f, valid_f = g.vertex_column("box_fill")
    ids = np.asarray(g.vertex_ids)
    assert valid_l.all() and valid_f.all() and cub in ids.tolist()
    assert np.array_equal(got_l, np.array([lengths[l] for l in ids.tolist()]))
    assert np.array_equal(got_f, np.array([fill[l] for l in ids.tolist()]))
