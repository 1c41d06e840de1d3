"""The distance pass on the MI355X past its launch limits (csrc/kernels_distance.hip): more rows than the row pass has waves, more
voxels than the extremes and pole kernels have threads, more table rows than the initialisation has threads, and runs that begin and
end at every lane of the row pass's 64-voxel chunks.  The volumes and plans come from tests/launch_limits.py (checked without a GPU by
test_launch_limits_cpu.py); image and table are compared bit for bit (every spacing is a power of two) with
tests/distance_reference.py or a closed form, and what the device launched (ta_distance_debug) with the plan."""
import functools

import numpy as np
import pytest

import distance_reference as ref
import launch_limits as ll
from tissue_analysis_amd import _capi, synth
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu

DTYPES = [np.uint16, np.uint32]
OWN, FROM = _capi.DIST_OWN_WALL, _capi.DIST_FROM_LABEL
UNIT, HALF, MIXED = (1.0, 1.0, 1.0), (0.5, 0.5, 1.0), (2.0, 0.25, 1.0)
BG = synth.BACKGROUND


def device(rv, spacing, mode, site, edge):
    """(D2 image with the axes of the volume, (min2, max2, pole), what was launched) of one pass over the volume resident in rv."""
    if rv.last is None:
        rv.extract(_capi.F_VOLUME, sparse=False)
    rv.ctx.distance_extract(mode, site, spacing, _capi.DIST_EDGE_IS_SITE if edge else 0)
    return np.array(rv.distance_image()), rv.ctx.distance_get(), rv.ctx.distance_debug()


def same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def same_plan(debug, memory_dims, table_rows):
    p = ll.distance_plan(memory_dims, table_rows)
    assert debug == dict(row_groups=p.row_groups, voxel_groups=p.voxel_groups, init_groups=p.init_groups,
                         column_launches=ll.distance_column_launches(memory_dims))
    return p


@functools.lru_cache(maxsize=None)
def many_rows():
    V = synth.voronoi_labels(ll.MANY_ROWS_DIMS, 300, 3)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def many_rows_answer(mode, edge):
    V = many_rows()
    d2 = ref.scipy_d2(V, HALF, mode, BG, edge)
    return d2, ll.distance_table(V, d2, int(V.max()) + 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_many_rows(dtype):
    V = many_rows().astype(dtype)
    rv = ResidentVolume(V)
    try:
        for mode in (OWN, FROM):
            for edge in (False, True):
                want_d2, want_table = many_rows_answer(mode, edge)
                d2, table, debug = device(rv, HALF, mode, BG, edge)
                assert np.array_equal(d2, want_d2)
                same(table, want_table)
                p = same_plan(debug, V.shape, int(V.max()) + 1)
                assert p.row_groups == ll.DIST_ROW_MAX_GROUPS < (p.rows + 3) // 4 and p.row_trips == 2      # fewer waves than rows
    finally:
        rv.close()


@pytest.mark.parametrize("permuted", [False, True], ids=["c_order", "permuted"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_many_voxels(dtype, permuted):
    dims, split, w = ll.MANY_VOXELS_DIMS, ll.MANY_VOXELS_SPLIT, MIXED[1]
    V = ll.half_space_axis1(dims, split, dtype)
    memory_dims = dims
    if permuted:                                           # memory axes (1, 2, 0): the pole's array-order key has other strides
        V = np.ascontiguousarray(V.transpose(1, 2, 0)).transpose(2, 0, 1)
        memory_dims = (dims[1], dims[2], dims[0])
    want_d2, want_table = ll.half_space_axis1_answer(dims, split, w)
    rv = ResidentVolume(V)
    try:
        d2, table, debug = device(rv, MIXED, OWN, 0, False)
    finally:
        rv.close()
    assert d2.shape == dims and np.array_equal(d2, want_d2)
    same(table, want_table)
    p = same_plan(debug, memory_dims, 3)
    assert p.voxel_groups == ll.DIST_VOXEL_MAX_GROUPS < (p.voxels + 255) // 256 and p.voxel_trips == 2     # fewer threads than voxels


def test_many_table_rows():
    V = ll.far_label()
    rows = ll.MANY_TABLE_ROWS_LABEL + 1
    want_d2 = ref.scipy_d2(V, HALF)
    want = ref.table(V, want_d2, rows)
    ctx = _capi.Context(0)
    try:
        ctx.set_volume(V)
        ctx.extract(_capi.F_VOLUME, ll.MANY_TABLE_ROWS_LABEL)
        ctx.distance_extract(OWN, 0, HALF, 0)
        d2 = ctx.distance_image().reshape(V.shape)
        table = ctx.distance_get()
        debug = ctx.distance_debug()
    finally:
        ctx.close()
    assert np.array_equal(d2, want_d2)
    same(table, want)
    present = np.zeros(rows, dtype=bool)
    present[[1, ll.MANY_TABLE_ROWS_LABEL]] = True
    min2, max2, pole = table
    assert np.isinf(min2[~present]).all() and np.isinf(max2[~present]).all() and (pole[~present] == -1).all()
    assert np.isfinite(max2[present]).all() and (pole[present] >= 0).all()
    p = same_plan(debug, V.shape, rows)
    assert p.init_groups == ll.DIST_INIT_MAX_GROUPS < (rows + 255) // 256 and p.init_trips == 2            # fewer threads than table rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_run_lengths(dtype):
    V = ll.runs_joined(dtype)
    rv = ResidentVolume(V)
    try:
        for spacing in (UNIT, HALF):
            for mode in (OWN, FROM):
                for edge in (False, True):
                    want = ref.scipy_d2(V, spacing, mode, 2, edge)
                    d2, table, debug = device(rv, spacing, mode, 2, edge)
                    assert np.array_equal(d2, want), (spacing, mode, edge)
                    same(table, ref.table(V, want, 3))
                    p = same_plan(debug, V.shape, 3)
                    assert p.row_trips == 1 and debug["column_launches"] == 2
    finally:
        rv.close()


def test_debug_is_valid_when_the_getters_are():
    V = synth.voronoi_labels((10, 12, 40), 30, 3, dtype=np.uint16)
    ctx = _capi.Context(0)

    def code(call):
        try:
            call()
        except _capi.TissueScanError as e:
            return e.code
        return _capi.TA_OK

    try:
        ctx.set_volume(V)
        ctx.extract(_capi.F_VOLUME, int(V.max()))
        assert code(ctx.distance_debug) == code(ctx.distance_get) == _capi.TA_EINVAL             # no pass yet
        ctx.distance_set_batch(1)                          # a wave of columns a launch: 40 * 10 / 64 and 40 * 12 / 64 launches, rounded up
        ctx.distance_extract(OWN, 0, HALF, 0)
        p = ll.distance_plan(V.shape, int(V.max()) + 1)
        assert ctx.distance_debug() == dict(row_groups=p.row_groups, voxel_groups=p.voxel_groups, init_groups=p.init_groups, column_launches=7 + 8)
        assert ctx._lib.ta_distance_debug(ctx._h, None) == _capi.TA_OK
        ctx.extract(_capi.F_VOLUME, int(V.max()))          # a new extraction
        assert code(ctx.distance_debug) == code(ctx.distance_get) == _capi.TA_EINVAL
    finally:
        ctx.close()
