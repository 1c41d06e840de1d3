"""tests/launch_limits.py without a GPU: its constants are those of the kernel headers, every named input crosses the limit it is
named for, and every closed form the GPU tests compare with equals the reference of tests/ at a small shape of the same
construction."""
import os
import re

import numpy as np
import pytest

import components_reference as cref
import distance_reference as dref
import junction_reference as jref
import launch_limits as ll
import nearest_cases
from tissue_analysis_amd import _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(name):
    return open(os.path.join(ROOT, "tissue_analysis_amd", "csrc", name)).read()


def constant(text, name):
    """The value of `NAME = <integer or 1u << k>` in a kernel source."""
    m = re.search(r"\b%s\s*=\s*(?:(\d+)(?:ull|u)?\s*<<\s*(\d+)|(\d+))\s*[,;]" % name, text)
    assert m, name
    return int(m.group(1)) << int(m.group(2)) if m.group(1) else int(m.group(3))


def test_the_constants_are_those_of_the_kernel_sources():
    h = source("ta_components.h")
    assert (constant(h, "CC_TILE_PLANES"), constant(h, "CC_TILE_ROWS"), constant(h, "CC_TILE_COLS")) == (ll.TP, ll.TR, ll.TC)
    assert constant(h, "CC_SEAM_MAX_GROUPS") == ll.CC_SEAM_MAX_GROUPS == 1 << 18
    assert constant(h, "CC_STREAM_MAX_GROUPS") == ll.CC_STREAM_MAX_GROUPS == 65536
    k = source("kernels_components.hip")
    assert constant(k, "CC_THREADS") == ll.THREADS and constant(k, "CC_STATS_CHUNKS") == ll.CC_STATS_CHUNKS
    assert "CC_SEAM_MAX_GROUPS" in k and "CC_STREAM_MAX_GROUPS" in k and "1u << 18" not in k and "65536" not in k
    assert constant(source("ta_junctions.h"), "JN_KEY_MAX_GROUPS") == ll.JN_KEY_MAX_GROUPS == 8192
    k = source("kernels_junctions.hip")
    assert (constant(k, "JN_RPW"), constant(k, "JN_PLANES"), constant(k, "JN_WAVES")) == (ll.JN_RPW, ll.JN_PLANES, ll.JN_WAVES)
    assert "JN_KEY_MAX_GROUPS" in k and "8192" not in k
    h = source("ta_distance.h")
    assert constant(h, "DIST_ROW_MAX_GROUPS") == ll.DIST_ROW_MAX_GROUPS == 1 << 16
    assert constant(h, "DIST_VOXEL_MAX_GROUPS") == ll.DIST_VOXEL_MAX_GROUPS == 1 << 14
    assert constant(h, "DIST_INIT_MAX_GROUPS") == ll.DIST_INIT_MAX_GROUPS == 1 << 12
    k = source("kernels_distance.hip")
    assert all(name in k for name in ("DIST_ROW_MAX_GROUPS", "DIST_VOXEL_MAX_GROUPS", "DIST_INIT_MAX_GROUPS")) and "1u << 1" not in k
    h = source("ta_nearest.h")
    assert constant(h, "NEAR_ROW_MAX_GROUPS") == ll.NEAR_ROW_MAX_GROUPS == 1 << 16
    assert constant(h, "NEAR_VOXEL_MAX_GROUPS") == ll.NEAR_VOXEL_MAX_GROUPS == 1 << 14
    assert constant(h, "NEAR_WORK_CAP") == ll.NEAR_WORK_CAP and constant(h, "NEAR_STACK_ENTRY") == ll.NEAR_STACK_ENTRY
    k = source("kernels_nearest.hip")
    assert "NEAR_ROW_MAX_GROUPS" in k and "NEAR_VOXEL_MAX_GROUPS" in k and "1u << 1" not in k
    assert "blockIdx.x * 4 + (threadIdx.x >> 6)" in k and ll.NEAR_ROWS_PER_GROUP == 4


def test_the_debug_calls_refuse_a_null_context_without_a_gpu():
    lib = _capi.load()
    for name in ("ta_components_debug", "ta_junctions_debug", "ta_distance_debug", "ta_nearest_debug"):
        assert getattr(lib, name)(None, None) == _capi.TA_EINVAL, name
        assert b"NULL" in lib.ta_last_error()


def test_strided_groups():
    assert ll.strided_groups(0, 8) == (1, 0) and ll.strided_groups(256, 8) == (1, 1) and ll.strided_groups(257, 8) == (2, 1)
    assert ll.strided_groups(8 * 256, 8) == (8, 1) and ll.strided_groups(8 * 256 + 1, 8) == (8, 2)
    assert ll.strided_groups(9, 2, 4) == (2, 2) and ll.strided_groups(8, 2, 4) == (2, 1)


# ---- components -------------------------------------------------------------------------------------------------------------------
def test_long_rows_take_the_column_loop_into_its_second_trip():
    p = ll.component_plan(ll.LONG_ROW_DIMS)
    assert p.column_seams == 257 > ll.THREADS and p.column_trips == 2 and p.seam_row_trips == 1
    assert ll.column_seams_of_trip(ll.LONG_ROW_DIMS, 0)[-1] == 65536 and ll.column_seams_of_trip(ll.LONG_ROW_DIMS, 1) == [65792]
    assert ll.component_plan((2, 5, 65792)).column_trips == 1 and ll.component_plan((2, 5, 65793)).column_trips == 2
    for dtype in (np.uint16, np.uint32):
        A = ll.long_rows_blocks(dtype)
        assert A.shape == ll.LONG_ROW_DIMS and A.dtype == dtype and ll.vector_path(A.shape, A.dtype.itemsize)
        # a label goes on across the second trip's column, and across column 65 536 (the last thread of the first trip), in a row
        # behind a tile face and in another row
        for columns in ([65792], [65536]):
            face, other = ll.column_links(A, columns)
            assert face >= 1 and other >= 1
        B = ll.long_rows_speck(dtype)
        assert ll.column_links(B, [65792]) == (2, 8) and ll.column_links(B, [65536]) == (2, 7)
        assert int((B == 9).sum()) == 1 and B[ll.LONG_ROW_SPECK] == 9 and not ll.is_face_row(B.shape, 1 * 5 + 2)
    rows = cref.table(ll.long_rows_blocks(np.uint16))[0]
    assert rows[0].size > 100 and set(rows[0].tolist()) == {1, 2}
    # the speck at a small shape of the same construction: three rows, the uniform label in one piece around it
    rows, image = cref.table(ll.long_rows_speck(np.uint16, (2, 5, 600), (1, 2, 512)))
    assert rows[0].tolist() == [4, 9] and rows[1].tolist() == [5999, 1] and rows[2][1].tolist() == [1, 2, 512]


def test_many_rows_take_the_seam_pass_into_its_second_trip():
    dims = ll.MANY_ROWS_DIMS
    p = ll.component_plan(dims)
    assert p.rows == 265200 > p.seam_groups == ll.CC_SEAM_MAX_GROUPS and p.seam_row_trips == 2 and p.column_seams == 0
    second = ll.seam_rows_of_trip(dims, 1)
    assert (second[0], second[-1]) == (262144, 265199) and any(ll.is_face_row(dims, r) for r in second)
    V = synth.voronoi_labels(dims, 300, 3)
    assert ll.face_links(V, second) > 1000 and ll.face_links(V, ll.seam_rows_of_trip(dims, 0)) > 1000
    S = ll.serpentine(dims)
    assert ll.face_links(S, second) > 1000
    # the snake reaches the second trip's rows through the one voxel that joins the planes 514 and 516: (515, 0, 0)
    assert S[515, 0, 0] == 1 and int((S[515] == 1).sum()) == 1 and ll.is_face_row(dims, 516 * 510) and 516 * 510 >= second[0]
    small = ll.serpentine((9, 11, 4))
    rows = cref.table(small)[0]
    assert rows[0].tolist().count(1) == 1 and int(rows[1][0]) == int((small == 1).sum())


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
def test_run_lengths(dtype):
    itemsize = np.dtype(dtype).itemsize
    v = ll.vpl(itemsize)
    L = ll.run_lengths(itemsize)
    assert set(range(1, 2 * v + 2)) <= set(L) and {63 * v - 1, 63 * v, 64 * v - 1, 64 * v, 64 * v + 1, 255, 256, 257} <= set(L)
    n2 = ll.run_row_length(itemsize)
    assert n2 == 2 * 256 + v + 3 and max(L) < n2 and not ll.vector_path((1, 1, n2), itemsize)
    rows = ll.run_rows(itemsize)
    assert rows.shape == (len(L) * v, n2) and set(np.unique(rows).tolist()) == {1, 2}
    k = L.index(5) * v + 3                                        # L = 5, o = 3: the first run is two voxels
    assert rows[k, :12].tolist() == [1, 1, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1]
    # every run starts at every offset into a strip, for every short L; every lane of the distance row pass begins and ends a run
    starts = set()
    for row in rows[:2 * v * v]:
        starts |= set(((np.flatnonzero(row[1:] != row[:-1]) + 1) % v).tolist())
    assert starts == set(range(v))
    begins, ends = set(), set()
    for row in rows[v:]:                                              # (not L = 1, which has a run at every voxel)
        b, e = ll.run_ends(row)
        begins |= b
        ends |= e
    assert ll.DIST_CHUNK == 64 and {0, 63, 64, 65, 127, 128} <= begins and {0, 62, 63, 64, 127, 128} <= ends
    iso, joined = ll.runs_isolated(dtype), ll.runs_joined(dtype)
    assert iso.shape == (1, 2 * rows.shape[0], n2) and (iso[0, 1::2] == 3).all() and np.array_equal(iso[0, ::2], rows)
    assert joined.shape == (3, rows.shape[0], n2) and np.array_equal(joined[2, :, :-2], rows[:, 2:])
    # isolated: a component per run, and one per row of the third label
    want = sum(int(np.count_nonzero(r[1:] != r[:-1])) + 1 for r in rows) + rows.shape[0]
    assert cref.table(iso)[0][0].size == want


def test_halo_on_long_rows():
    V = ll.halo_blocks(np.uint16)
    slab = V[ll.HALO_SLAB]
    own_begin = slab.shape[1] * slab.shape[2]
    assert V.shape == (9, 6, 520) and own_begin == 3120 and own_begin % ll.CC_STATS_CHUNK != 0
    count, ids = cref.component_ids(slab)
    one, owned, halo = ll.stats_chunks(ids, own_begin)
    assert np.count_nonzero(one & (owned == ll.CC_STATS_CHUNK)) > 10 and np.count_nonzero(one & (owned == 0)) > 3
    # the components of the chunks a wave keeps in registers, in the order it meets them: the same one again (added to what is kept)
    # and another one (what is kept is sent)
    flat = ids.reshape(-1)
    kept = [[int(flat[256 * k]) for k in range(w, min(w + ll.CC_STATS_CHUNKS, one.size)) if one[k] and owned[k] == 256]
            for w in range(0, one.size, ll.CC_STATS_CHUNKS)]
    assert any(a == b for wave in kept for a, b in zip(wave, wave[1:])) and any(a != b for wave in kept for a, b in zip(wave, wave[1:]))
    at = own_begin // ll.CC_STATS_CHUNK
    assert one[at] and owned[at] == 208 and halo[at] == 48                                                    # a halo voxel and owned ones
    assert len(one) > 2 * ll.CC_STATS_CHUNKS                                                                  # more than one wave
    rows, image = cref.table(slab, first_owned=1, a0_origin=4)
    assert rows[0].tolist() == [1, 1, 2, 3, 3] and rows[1].tolist() == [1560, 1560, 12478, 1, 1]
    assert int((image == cref.NONE).sum()) == 1560 and image[0, 1, 100] == cref.NONE and image[0, 5, 0] == 2


def test_grid_for_and_the_closed_form_of_the_split_volume():
    nvox = int(np.prod(ll.GRID_DIMS))
    assert nvox == 16896000 > ll.CC_STREAM_MAX_GROUPS * ll.THREADS == 16777216
    assert ll.stream_groups(nvox) == (65536, 2) and ll.stream_groups(16777216) == (65536, 1)
    for dims, split in (((7, 5, 6), 3), ((4, 3, 9), 1)):
        V = ll.split_planes(dims, split, ll.GRID_LABELS, np.uint16)
        rows, image = cref.table(V)
        for got, want in zip(ll.split_planes_table(dims, split, ll.GRID_LABELS), rows):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        assert np.array_equal(image, np.broadcast_to((np.arange(dims[0]) >= split).reshape(-1, 1, 1), dims))


# ---- junctions --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
def test_corners_meet_every_seam_of_the_walk(dtype):
    itemsize = np.dtype(dtype).itemsize
    v = ll.vpl(itemsize)
    lengths = ll.corner_row_lengths(itemsize)
    assert sorted(set(ll.vector_path((34, 6, n2), itemsize) for n2 in lengths)) == [False, True]
    assert {1100, 1101} <= set(lengths) and not ll.vector_path((34, 6, 1101), itemsize)
    assert ll.corner_columns(itemsize) == (v - 1, v, v + 1, 64 * v - 1, 64 * v, 64 * v + 1) and max(ll.corner_columns(itemsize)) < 1100
    dims = (34, 6, lengths[0])
    sites = dict(((Q, R, C), ll.junction_block_site(dims, itemsize, (Q - 1, R - 1, C - 1)))
                 for Q in ll.CORNER_Q for R in ll.CORNER_R for C in ll.corner_columns(itemsize))
    assert len(sites) == 90
    assert set(s.far for s in sites.values()) == {"strip", "lane", "load"}
    assert sites[(16, 2, 64 * v)].far == "load" and sites[(16, 2, v)].far == "lane" and sites[(16, 2, 64 * v + 1)].lane == 0
    assert sites[(16, 2, 64 * v)].task == (0, 0, 0) and sites[(17, 3, 64 * v + 1)].task == (1, 1, 1)
    assert set(s.last_plane for s in sites.values()) == {False, True} and set(s.last_row for s in sites.values()) == {False, True}
    assert sites[(16, 2, v)].last_plane and sites[(32, 2, v)].last_plane and not sites[(15, 2, v)].last_plane
    assert sites[(17, 2, v)].plane_in_task == 0 and sites[(16, 2, v)].last_row and sites[(16, 3, v)].row_in_task == 0
    p = ll.junction_plan(dims, itemsize)
    assert (p.ncb, p.nrb, p.npb) == (_ceil(lengths[0] - 1, 64 * v), 3, 3) and p.tasks > ll.JN_WAVES


def _ceil(a, b):
    return (a + b - 1) // b


def test_the_corner_the_issue_counts():
    (el, en, es), (vl, vn, vs), degenerate = jref.tables(ll.corner(16, 2, 512, 1100, np.uint16))
    assert el.tolist() == [[1, 2, 3], [1, 2, 4], [1, 3, 4], [2, 3, 4]] and en.tolist() == [15, 511, 1, 17]
    assert vl.tolist() == [[1, 2, 3, 4]] and vn.tolist() == [1] and vs.tolist() == [[31, 3, 1023]] and degenerate == 0
    for Q, R, C in ((15, 1, 3), (32, 3, 513)):                       # the one vertex lies in the block (Q - 1, R - 1, C - 1)
        (_, _, _), (vl, vn, vs), _ = jref.tables(ll.corner(Q, R, C, 1101, np.uint32))
        assert vn.tolist() == [1] and vs.tolist() == [[2 * Q - 1, 2 * R - 1, 2 * C - 1]]


def test_stripes_cross_the_key_kernels_cap_and_their_closed_form():
    B = [d - 1 for d in ll.STRIPES_DIMS]
    records = B[0] * B[1] * B[2]
    assert records == 2171715 > ll.JN_KEY_MAX_GROUPS * ll.THREADS == 2097152
    assert ll.junction_key_groups(records) == (8192, 2) and ll.junction_key_groups(0) == (0, 0)
    for dims in ((6, 7, 9), (2, 2, 5)):
        got, want = ll.stripes_tables(dims), jref.tables(ll.stripes(dims, np.uint16))
        for k in (0, 1):
            for g, w in zip(got[k], want[k]):
                assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
        assert got[2] == want[2] == 0
    edges = ll.stripes_tables(ll.STRIPES_DIMS)[0]
    assert edges[1].tolist() == [records] and edges[2].tolist() == [[65 * records, 129 * records, 259 * records]]


# ---- distance ---------------------------------------------------------------------------------------------------------------------
def test_distance_plans_cross_their_caps():
    p = ll.distance_plan(ll.MANY_ROWS_DIMS, 700)
    assert p.rows == 265200 > ll.DIST_ROW_MAX_GROUPS * ll.DIST_ROWS_PER_GROUP == 262144 and (p.row_groups, p.row_trips) == (65536, 2)
    assert p.voxel_trips == 1 and p.init_trips == 1
    for dims in (ll.MANY_VOXELS_DIMS, (250, 256, 66)):             # the array's dims and those of the permuted layout
        p = ll.distance_plan(dims, 3)
        assert p.voxels == 4224000 > ll.DIST_VOXEL_MAX_GROUPS * ll.THREADS == 4194304 and (p.voxel_groups, p.voxel_trips) == (16384, 2)
        assert p.row_trips == 1
    p = ll.distance_plan(ll.MANY_TABLE_ROWS_DIMS, ll.MANY_TABLE_ROWS_LABEL + 1)
    assert p.table_rows == 1048701 > ll.DIST_INIT_MAX_GROUPS * ll.THREADS == 1048576 and (p.init_groups, p.init_trips) == (4096, 2)
    V = ll.far_label()
    assert V.dtype == np.uint32 and int(V.max()) == ll.MANY_TABLE_ROWS_LABEL and set(np.unique(V).tolist()) == {1, ll.MANY_TABLE_ROWS_LABEL}


def test_distance_table_in_whole_array_operations_is_the_references():
    V = synth.voronoi_labels((12, 20, 33), 25, 3, dtype=np.uint16)
    rows = int(V.max()) + 3                                          # absent rows behind the last label, and some among them
    for d2 in (dref.scipy_d2(V, (0.5, 0.5, 1.0)), dref.scipy_d2(V, (1.0, 1.0, 1.0), dref.FROM_LABEL, 1, True), np.full(V.shape, np.inf)):
        for layout in (V, np.asfortranarray(V)):
            for g, w in zip(ll.distance_table(layout, d2, rows), dref.table(layout, d2, rows)):
                assert g.dtype == w.dtype and np.array_equal(g, w)
    assert ll.distance_column_launches(ll.MANY_ROWS_DIMS) == ll.distance_column_launches(ll.MANY_VOXELS_DIMS) == 2
    assert ll.distance_column_launches((3, 1 << 20, 64)) == 3 + 4    # stacks of 2^20 entries: a wave of 64 columns a launch; of 3: 17 895 680


def test_half_space_closed_form():
    for dims, split, w in (((3, 9, 4), 4, 0.25), ((2, 7, 5), 5, 2.0)):
        V = ll.half_space_axis1(dims, split, np.uint16)
        spacing = (2.0, w, 1.0)
        want = dref.scipy_d2(V, spacing)
        d2, table = ll.half_space_axis1_answer(dims, split, w)
        assert np.array_equal(d2, want)
        for g, t in zip(table, dref.table(V, want, 3)):
            assert g.dtype == t.dtype and np.array_equal(g, t)


# ---- nearest labels ---------------------------------------------------------------------------------------------------------------
def test_nearest_plans_and_the_volume_that_crosses_both_caps():
    assert ll.nearest_plan((7, 9, 11)) == (63, 16, 1, 693, 3, 1) and ll.nearest_second_trip((7, 9, 11)) == (None, None)
    assert ll.nearest_plan((1, 1, 1)) == (1, 1, 1, 1, 1, 1) and ll.nearest_plan((65536, 4, 16))[1:3] == (65536, 1)
    assert ll.nearest_plan((65536, 4, 16))[4:] == (16384, 1) and ll.nearest_plan((65536, 4, 17))[4:] == (16384, 2)
    assert ll.nearest_plan((1, 262145, 1))[1:3] == (65536, 2) and ll.nearest_column_launches((7, 9, 11)) == 2
    assert ll.nearest_column_launches((3, 1 << 20, 64)) == 3 + 6  # stacks of 2^20 entries: a wave of 64 columns a launch; of 3: 12 782 592 of 2^26
    dims = nearest_cases.CAP_DIMS
    for d in (dims, (dims[0], dims[2], dims[1])):                  # (a layout that swaps the two fast axes crosses the voxel cap only)
        p = ll.nearest_plan(d)
        assert p.voxels == 4482594 > ll.NEAR_VOXEL_MAX_GROUPS * ll.THREADS == 4194304 and (p.voxel_groups, p.voxel_trips) == (16384, 2)
    p = ll.nearest_plan(dims)
    assert p.rows == 263682 > ll.NEAR_ROW_MAX_GROUPS * ll.NEAR_ROWS_PER_GROUP == 262144 and (p.row_groups, p.row_trips) == (65536, 2)
    assert p.voxels % 64 == 34                                     # the last wave of the counting kernel is partly past the volume
    row, voxel = ll.nearest_second_trip(dims)
    assert divmod(row, dims[1]) == (1020, 4) and np.unravel_index(voxel, dims) == (960, 3, 13)
    assert nearest_cases.CAP_LATE == 1021 and nearest_cases.CAP_MIDDLE == 960
    assert ll.nearest_column_launches(dims) == 2 and 120e6 < ll.nearest_stack_bytes(dims) < 130e6 < ll.NEAR_WORK_CAP
    V = nearest_cases.cap_sites()
    planes = np.nonzero(V)[0]
    assert V.shape == dims and V.dtype == np.uint16 and sorted(V[V != 0].tolist()) == list(range(1, 17))
    assert (planes >= 1021).sum() >= 3 and ((planes >= 960) & (planes <= 1019)).sum() >= 3 and (planes < 960).sum() >= 3
    # the control: the same sites in a volume under both caps
    p = ll.nearest_plan(nearest_cases.CAP_CONTROL_DIMS)
    assert p.row_groups < ll.NEAR_ROW_MAX_GROUPS and p.voxel_groups < ll.NEAR_VOXEL_MAX_GROUPS and (p.row_trips, p.voxel_trips) == (1, 1)
    assert p.rows > 0.99 * 262144 and p.voxels > 0.99 * 4194304
    C = nearest_cases.cap_sites(nearest_cases.CAP_CONTROL_DIMS)
    assert sorted(C[C != 0].tolist()) == list(range(1, 17))
