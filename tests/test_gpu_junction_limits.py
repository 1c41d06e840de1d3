"""The junction pass on the MI355X at the seams of its walk and past the cap of its key kernel (csrc/kernels_junctions.hip).  A vertex
is placed in the one block whose far column comes from the next lane's registers, or from lane 63's separate load, and in the blocks
on the seam of two 16-plane tasks and of two 2-row tasks, for the vector and for the scalar loads; and a volume whose every block is an
edge of the same three cells gives the key kernel more records than it has threads.  The volumes and plans come from
tests/launch_limits.py (checked without a GPU by test_launch_limits_cpu.py); every table is compared bit for bit with
tests/junction_reference.py or a closed form, and what the device launched (ta_junctions_debug) with the plan."""
import numpy as np
import pytest

import junction_reference as ref
import launch_limits as ll
from tissue_analysis_amd import _capi, synth

pytestmark = pytest.mark.gpu

DTYPES = [np.uint16, np.uint32]


def same_tables(got, want):
    """got: the tuple of Context.junctions_get; want: ref.tables() of the same image."""
    for k, width in ((0, 3), (1, 4)):
        assert got[k][0].shape == want[k][0].shape == (want[k][1].size, width)
        for g, w in zip(got[k], want[k]):
            assert g.shape == w.shape and np.array_equal(g.astype(w.dtype), w)
    assert got[2] == want[2]


def run(ctx, V):
    ctx.set_volume(V)
    ctx.junctions_extract()
    return ctx.junctions_get(), ctx.junctions_debug()


CORNER_CASES = [(dtype, n2) for dtype in DTYPES for n2 in ll.corner_row_lengths(np.dtype(dtype).itemsize)]


@pytest.mark.parametrize("dtype,n2", CORNER_CASES, ids=["%s-%d" % (np.dtype(d).name, n) for d, n in CORNER_CASES])
def test_corners(dtype, n2):
    itemsize = np.dtype(dtype).itemsize
    plan = ll.junction_plan((34, 6, n2), itemsize)
    seen = set()
    ctx = _capi.Context(0)
    try:
        for Q in ll.CORNER_Q:
            for R in ll.CORNER_R:
                for C in ll.corner_columns(itemsize):
                    V = ll.corner(Q, R, C, n2, dtype)
                    want = ref.tables(V)
                    (el, en, es), (vl, vn, vs), degenerate = want
                    assert vl.tolist() == [[1, 2, 3, 4]] and vs.tolist() == [[2 * Q - 1, 2 * R - 1, 2 * C - 1]] and degenerate == 0
                    # the edges {1,2,3}, {1,2,4}, {1,3,4}, {2,3,4} that run into it
                    assert en.tolist() == [n for n in (Q - 1, C - 1, R - 1, 33 - Q) if n]
                    got, debug = run(ctx, V)
                    same_tables(got, want)
                    assert debug == dict(tasks=plan.tasks, edge_key_groups=ll.junction_key_groups(int(en.sum()))[0], vertex_key_groups=1), (Q, R, C)
                    site = ll.junction_block_site(V.shape, itemsize, (Q - 1, R - 1, C - 1))
                    seen.add((site.far, site.last_plane, site.last_row))
    finally:
        ctx.close()
    # every source of the far column met a block on the seam of two plane ranges and of two row pairs, and one that is on neither
    for far in ("strip", "lane", "load"):
        assert (far, True, True) in seen and (far, False, False) in seen
    assert ll.vector_path((34, 6, n2), itemsize) == (n2 == (1100 if itemsize == 4 else 1104))


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_records_than_the_key_kernel_has_threads(dtype):
    V = ll.stripes(ll.STRIPES_DIMS, dtype)
    want = ll.stripes_tables(ll.STRIPES_DIMS)
    records = int(want[0][1][0])
    ctx = _capi.Context(0)
    try:
        got, debug = run(ctx, V)
    finally:
        ctx.close()
    same_tables(got, want)
    groups, trips = ll.junction_key_groups(records)
    assert debug == dict(tasks=ll.junction_plan(V.shape, V.dtype.itemsize).tasks, edge_key_groups=groups, vertex_key_groups=0)
    assert groups == ll.JN_KEY_MAX_GROUPS < (records + 255) // 256 and trips == 2


SCAN_PER_BLOCK = 2048               # counts a workgroup of the scan of the walk's per-task counts takes (csrc/ta_counted.h)
# the smallest volumes with 2 x 2 x 2 blocks whose walk has exactly SCAN_PER_BLOCK tasks, and one more: a task is two rows of blocks
SCAN_EDGE_DIMS = {SCAN_PER_BLOCK: (2, 4096, 2), SCAN_PER_BLOCK + 1: (2, 4098, 2)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tasks", sorted(SCAN_EDGE_DIMS))
def test_a_walk_of_one_scan_block_and_of_one_task_more(tasks, dtype):
    dims = SCAN_EDGE_DIMS[tasks]
    itemsize = np.dtype(dtype).itemsize
    assert ll.junction_plan(dims, itemsize).tasks == tasks
    assert ll.junction_plan((dims[0], dims[1] - 1, dims[2]), itemsize).tasks == tasks - 1     # (thinner: no 2 x 2 x 2 block is left)
    V = np.random.default_rng(tasks).integers(1, 5, size=dims).astype(dtype)         # four labels: edges and vertices in every task
    want = ref.tables(V)
    assert want[0][1].size == 4 and want[1][1].size == 1 and int(want[1][1][0]) > tasks // 2 and want[2] == 0
    ctx = _capi.Context(0)
    try:
        got, debug = run(ctx, V)
    finally:
        ctx.close()
    same_tables(got, want)
    assert debug == dict(tasks=tasks, edge_key_groups=ll.junction_key_groups(int(want[0][1].sum()))[0],
                         vertex_key_groups=ll.junction_key_groups(int(want[1][1].sum()))[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_volume_of_one_label_has_no_rows(dtype):
    ctx = _capi.Context(0)
    try:
        got, debug = run(ctx, np.full((4, 6, 72), 7, dtype=dtype))
    finally:
        ctx.close()
    (el, en, es), (vl, vn, vs), degenerate = got
    assert el.shape == (0, 3) and vl.shape == (0, 4) and en.size == es.size == vn.size == vs.size == 0 and degenerate == 0
    assert debug == dict(tasks=ll.junction_plan((4, 6, 72), np.dtype(dtype).itemsize).tasks, edge_key_groups=0, vertex_key_groups=0)


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
        assert code(ctx.junctions_debug) == code(ctx.junctions_size) == _capi.TA_EINVAL          # no pass yet
        ctx.junctions_extract()
        debug = ctx.junctions_debug()                                                           # settles, as ta_junctions_size does
        (_, en, _), (_, vn, _), _ = ref.tables(V)
        assert ctx.junctions_size()[:2] == (en.size, vn.size) and en.size > 0 and vn.size > 0
        assert debug == dict(tasks=ll.junction_plan(V.shape, 2).tasks, edge_key_groups=ll.junction_key_groups(int(en.sum()))[0],
                             vertex_key_groups=ll.junction_key_groups(int(vn.sum()))[0])
        assert ctx.junctions_timing()[0] > 0.0 and ctx._lib.ta_junctions_debug(ctx._h, None) == _capi.TA_OK
        ctx.set_volume(np.full((4, 4, 40), 7, dtype=np.uint16))                                  # a new volume, without junctions
        assert code(ctx.junctions_debug) == code(ctx.junctions_size) == _capi.TA_EINVAL
        ctx.junctions_extract()
        assert ctx.junctions_debug() == dict(tasks=ll.junction_plan((4, 4, 40), 2).tasks, edge_key_groups=0, vertex_key_groups=0)
    finally:
        ctx.close()
