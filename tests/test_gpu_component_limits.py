"""The component pass on the MI355X past its launch limits (csrc/kernels_components.hip): rows long enough for the second trip of the
seam pass's column loop, more rows than the seam pass has workgroups, runs of every length at every alignment to the 16-byte strips
of the local pass, a halo plane in front of rows long enough for the statistics kernel to keep whole chunks in registers, and more
voxels than the image and relabel kernels have threads.  The volumes and the plan of every launch come from tests/launch_limits.py
(checked without a GPU by test_launch_limits_cpu.py); every case compares the table and the row image bit for bit with
tests/components_reference.py or a closed form, and the launch the device reports (ta_components_debug) with the plan."""
import functools

import numpy as np
import pytest

import components_reference as ref
import launch_limits as ll
from tissue_analysis_amd import _capi, synth

pytestmark = pytest.mark.gpu

DTYPES = [np.uint16, np.uint32]
TORCH_VIEW = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}


def same_rows(got, want):
    """got: the tuple of Context.components_get; want: the rows of ref.table()."""
    for g, w, name in zip(got, want, ("label", "n", "first", "bbox", "sum1")):
        assert g.shape == w.shape, name
        assert np.array_equal(g.astype(w.dtype), w), name


def same_plan(debug, dims, slots, image_voxels):
    p = ll.component_plan(dims)
    assert debug == dict(tiles=p.tiles, seam_groups=p.seam_groups, stream_groups=ll.stream_groups(image_voxels)[0],
                         key_groups=ll.stream_groups(slots)[0])
    return p


def check(V, want):
    """The device's table and row image of the C-ordered V against `want` = (rows, image); returns the plan the device confirmed."""
    ctx = _capi.Context(0)
    try:
        ctx.set_volume(V)
        ctx.components_extract()
        got = ctx.components_get()
        image = ctx.components_image()
        debug = ctx.components_debug()
    finally:
        ctx.close()
    same_rows(got, want[0])
    assert image.dtype == np.uint32 and np.array_equal(image.reshape(V.shape), want[1])
    return same_plan(debug, V.shape, want[0][0].size, V.size)


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref.table() of a named volume, made once (the labels are the same for both label types)."""
    make = {
        "blocks": lambda: ll.long_rows_blocks(np.uint16),
        "speck": lambda: ll.long_rows_speck(np.uint16),
        "voronoi": lambda: synth.voronoi_labels(ll.MANY_ROWS_DIMS, 300, 3),
        "serpentine": lambda: ll.serpentine(ll.MANY_ROWS_DIMS),
    }[name]
    V = make()
    V.setflags(write=False)
    return V, ref.table(V)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["blocks", "speck"])
def test_long_rows(name, dtype):
    V, want = reference(name)
    assert V.shape == ll.LONG_ROW_DIMS and want[0][0].size == (210 if name == "blocks" else 2)
    p = check(V.astype(dtype), want)
    assert p.column_trips == 2 and p.column_seams > ll.THREADS            # the column loop's second trip


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["voronoi", "serpentine"])
def test_many_rows(name, dtype):
    V, want = reference(name)
    label = want[0][0]
    assert V.shape == ll.MANY_ROWS_DIMS
    assert (label.size, np.unique(label).size) == ((708, 687) if name == "voronoi" else (2, 2))
    p = check(V.astype(dtype), want)
    assert p.seam_groups == ll.CC_SEAM_MAX_GROUPS < p.rows and p.seam_row_trips == 2       # fewer workgroups than rows


SCAN_PER_BLOCK = 2048               # counts a workgroup of the scan of the per-wave root counts takes (csrc/ta_counted.h)
# The count has ll.component_waves(dims) waves, four per 1024 voxels: the fewest voxels that give exactly SCAN_PER_BLOCK waves,
# and the fewest that give more -- SCAN_PER_BLOCK + 4, for no volume has SCAN_PER_BLOCK + 1 -- in three factors each (2^19 + 1 =
# 3 x 174763 has no third factor: the second volume is two voxels past the threshold)
SCAN_EDGE_DIMS = {SCAN_PER_BLOCK: (5, 229, 457), SCAN_PER_BLOCK + 4: (37, 109, 130)}


@functools.lru_cache(maxsize=None)
def scan_edge_reference(waves):
    V = synth.voronoi_labels(SCAN_EDGE_DIMS[waves], 200, waves)
    V.setflags(write=False)
    return V, ref.table(V)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("waves", sorted(SCAN_EDGE_DIMS))
def test_a_count_of_one_scan_block_and_of_the_next_size(waves, dtype):
    dims = SCAN_EDGE_DIMS[waves]
    voxels = dims[0] * dims[1] * dims[2]
    assert ll.component_waves(dims) == waves and 4 * ((voxels - 2 + 1023) // 1024) == waves - 4   # two voxels fewer: four waves fewer
    V, want = scan_edge_reference(waves)
    assert want[0][0].size >= 200
    check(V.astype(dtype), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_volume_of_one_label_is_one_row(dtype):
    V = np.full((4, 6, 72), 7, dtype=dtype)
    want = ref.table(V)
    assert want[0][0].tolist() == [7] and want[0][1].tolist() == [V.size]
    check(V, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("make", [ll.runs_isolated, ll.runs_joined])
def test_run_lengths(make, dtype):
    V = make(dtype)
    want = ref.table(V)
    runs = ll.run_rows(V.dtype.itemsize)
    if make is ll.runs_isolated:                                           # a row per run: no run is mended through a neighbour
        assert want[0][0].size == sum(int(np.count_nonzero(r[1:] != r[:-1])) + 1 for r in runs) + runs.shape[0]
    else:
        assert 1000 < want[0][0].size < sum(int(np.count_nonzero(r[1:] != r[:-1])) + 1 for r in runs)
    p = check(V, want)
    assert p.tiles == (V.shape[0] + ll.TP - 1) // ll.TP * ((V.shape[1] + ll.TR - 1) // ll.TR) * 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_halo_on_long_rows(dtype):
    import torch
    V = ll.halo_blocks(dtype)
    slab = np.ascontiguousarray(V[ll.HALO_SLAB])
    want = ref.table(slab, first_owned=1, a0_origin=4)
    assert want[0][0].tolist() == [1, 1, 2, 3, 3] and int((want[1] == ref.NONE).sum()) == 1560
    slots = ref.component_ids(slab)[0]
    assert slots == want[0][0].size + 2                                    # two components lie in the halo plane only
    t = torch.from_numpy(slab.view(TORCH_VIEW[slab.dtype]).copy()).cuda()
    torch.cuda.synchronize()
    ctx = _capi.Context(0)
    try:
        ctx.set_volume_device(t.data_ptr(), slab.dtype.itemsize, t.shape, a0_origin=4, has_low_halo=True, keep=t)
        ctx.components_extract()
        got = ctx.components_get()
        image = ctx.components_image().reshape(slab.shape)
        halo_plane = ctx.components_image(0, 1)
        debug = ctx.components_debug()
    finally:
        ctx.close()
    same_rows(got, want[0])
    assert np.array_equal(image, want[1]) and np.array_equal(halo_plane, want[1][0].reshape(-1))
    p = ll.component_plan(slab.shape)
    assert debug == dict(tiles=p.tiles, seam_groups=p.seam_groups, stream_groups=ll.stream_groups(slab[0].size)[0],
                         key_groups=ll.stream_groups(slots)[0])


def test_more_voxels_than_the_streaming_kernels_have_threads():
    V = ll.split_planes(ll.GRID_DIMS, ll.GRID_SPLIT, ll.GRID_LABELS, np.uint16)
    rows = ll.split_planes_table(ll.GRID_DIMS, ll.GRID_SPLIT, ll.GRID_LABELS)
    ctx = _capi.Context(0)
    try:
        ctx.set_volume(V)
        ctx.components_extract()
        got = ctx.components_get()
        image = ctx.components_image().reshape(V.shape)
        debug = ctx.components_debug()
        same_rows(got, rows)
        assert np.array_equal(image[:ll.GRID_SPLIT], np.zeros_like(image[:ll.GRID_SPLIT])) and (image[ll.GRID_SPLIT:] == 1).all()
        p = same_plan(debug, V.shape, 2, V.size)
        groups, trips = ll.stream_groups(V.size)
        assert debug["stream_groups"] == groups == ll.CC_STREAM_MAX_GROUPS < (V.size + 255) // 256 and trips == 2
        assert p.seam_row_trips == 1 and p.column_trips == 1
        ctx.components_relabel(np.array(ll.GRID_LABELS[::-1], dtype=np.uint32))       # the same grid: every voxel of both trips is rewritten
        with pytest.raises(_capi.TissueScanError) as e:
            ctx.components_debug()                                                    # the tables are gone, as for the other getters
        assert e.value.code == _capi.TA_EINVAL
        back = np.empty_like(V)
        ctx.get_volume(back)
    finally:
        ctx.close()
    assert (back[:ll.GRID_SPLIT] == ll.GRID_LABELS[1]).all() and (back[ll.GRID_SPLIT:] == ll.GRID_LABELS[0]).all()


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
        assert code(ctx.components_debug) == code(ctx.components_size) == _capi.TA_EINVAL         # no pass yet
        ctx.components_extract()
        first = ctx.components_debug()                                                          # settles, as ta_components_size does
        assert first["stream_groups"] == 0 and first["key_groups"] == 1 and ctx.components_timing()[0] > 0.0
        ctx.components_image(2, 3)
        assert ctx.components_debug() == dict(first, stream_groups=ll.stream_groups(3 * 12 * 40)[0])
        assert ctx._lib.ta_components_debug(ctx._h, None) == _capi.TA_OK
        ctx.set_volume(V)                                                                        # a new volume
        assert code(ctx.components_debug) == code(ctx.components_size) == _capi.TA_EINVAL
    finally:
        ctx.close()
