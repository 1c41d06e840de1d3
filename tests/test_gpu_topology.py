"""Euler numbers on the MI355X (include/tissue_scan_topology.h, csrc/kernels_topology.hip) against the restatement of
tests/topology_reference.py: the twelve block counts of every row bit-exact, n0 equal to the sweep's count, the launch plan the
device reports equal to the restated one -- at the shapes where the blocks beyond the faces and the tile seams go wrong."""
import os

import numpy as np
import pytest

import range_tiles as rt
import topology_reference as tr
from feature_passes import Pass, code, poke, tensor
from tissue_analysis_amd import DICT, NPLIST, CellTopology, SpatialImage, SpatialImageAnalysis, _capi, synth
from tissue_analysis_amd.extraction import ResidentVolume
from tissue_analysis_amd.graph_from_image import graph_from_image

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same_counts(got, want):
    """got: the six arrays as the library gives them (or a CellTopology's); want: tr.counts()."""
    for name, g in zip(tr.COLUMNS, got):
        assert np.array_equal(np.asarray(g).astype(np.uint64), want[name]), name


def check_topology(t, V):
    """t: the CellTopology of label image V (any dense layout, any integer type), from a ResidentVolume."""
    x = t.extraction
    V3 = V if V.ndim == 3 else V[:, :, None]
    Vm = V3.transpose(t.perm)                                 # the memory-order view
    rows = None if x.ids is None else np.searchsorted(x.ids, Vm.astype(np.int64))
    want = tr.counts(Vm, x.nrows, rows)
    same_counts([getattr(t, k) for k in tr.COLUMNS], want)
    assert np.array_equal(t.n0, x.count.astype(np.int64)) and int(t.n0.sum()) == V.size
    assert np.array_equal(t.euler_number(6), tr.euler(want, 6)) and np.array_equal(t.euler_number(26), tr.euler(want, 26))
    return want


def _run(V, **kw):
    rv = ResidentVolume(V)
    try:
        rv.extract(**kw)
        t = rv.topology()
        debug = rv.ctx.topology_debug()
        plan = tr.plan([rv.host.shape[a] for a in t.perm], rv.host.dtype.itemsize)      # (memory-order dims)
        assert (debug["tiles_per_group"], debug["groups"]) == (plan.per, plan.groups), (debug, plan)
    finally:
        rv.close()
    assert isinstance(t, CellTopology) and t.ms is not None and t.ms >= 0
    return t, debug


def _c1(dtype=np.uint16):
    c = synth.CONFIGS["C1"]
    return synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], dtype)


# ---- 1. types and load paths ----------------------------------------------------------------------------------------------------
def test_adversarial_golden_volumes():
    z = np.load(os.path.join(GOLD, "adversarial_small.npz"))
    for name in sorted(set(k.split("__")[0] for k in z.files)):
        V = z[name + "__volume"]
        check_topology(_run(V)[0], V)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_config1(dtype):
    V = _c1().astype(dtype)
    t, debug = _run(V)
    check_topology(t, V)
    assert debug["spills"] == 0 and debug["mixed"] > 0


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.int16, np.int32, np.int64, np.uint64], ids=lambda d: np.dtype(d).name)
def test_the_other_label_types_the_resident_volume_takes(dtype):
    V = rt.block_labels((21, 10, 37), np.uint16, 3, nlabels=90, block=(3, 2, 5)).astype(dtype)
    check_topology(_run(V)[0], V)


@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 7, 9), (5, 1, 300), (6, 5, 1)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_dims_of_one(dims, dtype):
    V = rt.block_labels(dims, dtype, 4, nlabels=5, block=(2, 3, 7))
    check_topology(_run(V)[0], V)
    W = np.full(dims, 3, dtype=dtype)                         # one label: a ball whatever the dims
    t, debug = _run(W)
    check_topology(t, W)
    assert t.euler_number(6)[3] == 1 and t.euler_number(26)[3] == 1 and debug["mixed"] == 0


def test_a_two_dimensional_image_through_the_analysis():
    V = np.zeros((40, 50), dtype=np.uint16)
    V[5:30, 5:40] = 2
    V[10:20, 10:20] = 0                                       # a hole in a 2-D cell is a tunnel of the slab it is
    V[33:38, 3:9] = 3
    sia = SpatialImageAnalysis(SpatialImage(V, voxelsize=(0.5, 2.0)), return_type=DICT, background=0)
    t = sia.cell_topology()
    check_topology(t, V)
    assert sia.euler_number() == {2: 0, 3: 1} and sia.euler_number(connectivity=26) == {2: 0, 3: 1}
    assert sia.mean_breadth(3)[3] == pytest.approx((5 * 0.5 + 6 * 2.0 + 1.0) / 2, rel=1e-12)


@pytest.mark.parametrize("dtype", [np.uint32, np.uint16], ids=["u32", "u16"])
@pytest.mark.parametrize("delta", [0, -1, 1], ids=["tile", "tile-1", "tile+1"])
def test_dims_around_one_tile(dtype, delta):
    cols = rt.columns(np.dtype(dtype).itemsize)
    dims = (rt.PLANES + delta, rt.WAVES + delta, cols + delta)
    assert dims in ((16, 4, 256), (15, 3, 255), (17, 5, 257), (16, 4, 512), (15, 3, 511), (17, 5, 513))
    V = rt.block_labels(dims, dtype, 7 + delta, nlabels=40, block=(3, 2, 9))
    t, debug = _run(V)
    check_topology(t, V)
    assert debug["groups"] == tr.plan(dims, np.dtype(dtype).itemsize).tiles == {0: 4, -1: 1, 1: 8}[delta]
    W = np.full(dims, 1, dtype=dtype)                         # every block beyond a face counted once: v = (n0+1)(n1+1)(n2+1)
    t, debug = _run(W)
    check_topology(t, W)
    assert int(t.v[1]) == int(np.prod([d + 1 for d in dims])) and debug["mixed"] == 0


def test_rows_that_are_no_whole_strips():
    V = np.ascontiguousarray(_c1()[:40, :50, :61])            # the element loads
    assert not rt.vector_path(V.shape, 2)
    check_topology(_run(V)[0], V)
    W = np.ascontiguousarray(V[:, :, :27]).astype(np.uint32)
    check_topology(_run(W)[0], W)


def test_fortran_order():
    V = np.asfortranarray(_c1()[:60, :70, :])
    t, _ = _run(V)
    assert t.perm == (2, 1, 0)
    check_topology(t, V)
    c, _ = _run(np.ascontiguousarray(V))
    assert c.perm == (0, 1, 2)
    assert np.array_equal(t.euler_number(), c.euler_number()) and np.array_equal(t.euler_number(26), c.euler_number(26))
    assert np.array_equal(t.faces(), c.faces()) and np.array_equal(t.face_pairs(), c.face_pairs())
    assert np.array_equal(t.mean_breadth((0.5, 2.0, 1.25)), c.mean_breadth((0.5, 2.0, 1.25)))


@pytest.mark.parametrize("off", [0, 1], ids=["+0B", "+2B"])
def test_unaligned_label_buffer(off):
    from test_gpu_unaligned_buffers import SHAPE_A, offset_view
    V = rt.block_labels(SHAPE_A, np.uint16, 51, nlabels=60)
    assert rt.vector_path(SHAPE_A, 2)                         # whole strips: the address alone decides
    ctx = _capi.Context(0)
    try:
        lv = offset_view(V, off, 3)
        assert lv.dev_ptr % 16 == 2 * off
        ctx.set_volume_device(lv.dev_ptr, 2, V.shape, keep=lv.flat)
        L = int(V.max())
        ctx.extract(_capi.F_ALL, L)
        ctx.topology_extract()
        same_counts(ctx.topology_rows(), tr.counts(V, L + 1))
        assert np.array_equal(lv.read_back().reshape(V.shape), V)
    finally:
        ctx.close()


# ---- 2. mixed blocks, spills, ranges ------------------------------------------------------------------------------------------------
def check_pass(p):
    """Run the pass on the context of p (a feature_passes.Pass with an extraction): rows against the reference, the plan the
    device reports against the restated one.  Returns (debug, reference counts, restated plan)."""
    p.ctx.topology_extract()
    debug = p.ctx.topology_debug()
    plan = tr.plan(p.V.shape, p.V.dtype.itemsize)
    assert (debug["tiles_per_group"], debug["groups"]) == (plan.per, plan.groups), (debug, plan)
    want = tr.counts(p.V, p.max_label + 1)
    same_counts(p.ctx.topology_rows(), want)
    assert int(want["n0"].sum()) == p.V.size
    return debug, want, plan


def test_a_checkerboard_and_all_distinct_labels():
    i, j, k = np.meshgrid(np.arange(9), np.arange(10), np.arange(37), indexing="ij")
    V = (1 + (i + j + k) % 2).astype(np.uint16)
    with Pass(V) as p:
        p.extract()
        debug, want, _ = check_pass(p)
        assert np.array_equal(tr.euler(want, 6), want["n0"].astype(np.int64))        # no two voxels of a label share a face
        assert debug["mixed"] == 10 * 11 * 38 - 8             # every block but the eight at the corners of the volume
    W = rt.permutation_labels((6, 5, 21), np.uint16, 9)
    with Pass(W) as p:
        p.extract()
        debug, want, _ = check_pass(p)
        assert (tr.euler(want, 6) == 1).all() and (tr.euler(want, 26) == 1).all() and debug["mixed"] > 0


@pytest.mark.parametrize("dims,dtype", [(rt.SPILL_DIMS, np.uint16), (rt.SPILL_DIMS_WIDE, np.uint32)], ids=["one_tile_u16", "wide_u32"])
def test_more_labels_than_table_slots(dims, dtype):
    V = rt.permutation_labels(dims, dtype, 43)
    bound = tr.label_spill_bound(V)
    assert bound > 0 and (dims != rt.SPILL_DIMS or bound == 4096 - tr.LABEL_SLOTS)
    with Pass(V) as p:
        p.extract()
        debug, _, _ = check_pass(p)
        assert debug["spills"] >= bound


@pytest.mark.parametrize("name", ["a_u16", "c_u32", "b_u32_scalar"])
def test_tile_ranges(name):
    case = rt.CASE[name]
    V = rt.block_labels(case.dims, case.dtype, 41)
    with Pass(V) as p:
        p.extract()
        debug, _, plan = check_pass(p)
        assert plan.per > 1 and plan.groups > 1 and debug["tiles_per_group"] == plan.per


def test_sparse_ids_compacted_context():
    rng = np.random.default_rng(5)
    ids = np.array([0, 7, 70000, 2**31 + 5, 2**32 - 2, 2**32 - 1], dtype=np.uint32)
    V = ids[rng.integers(0, ids.size, size=(12, 9, 33))]
    t, _ = _run(V, sparse=True)
    assert t.ids is not None and np.array_equal(t.ids, ids.astype(np.int64)) and len(t) == ids.size      # the rows are ranks
    want = check_topology(t, V)
    got = t.of_labels([2**32 - 1, 7, 12345])
    assert got.tolist() == [int(tr.euler(want, 6)[5]), int(tr.euler(want, 6)[1]), 0]


def test_a_label_at_only_the_eight_corners():
    for dtype, dims in ((np.uint16, (17, 6, 513)), (np.uint32, (5, 6, 7))):
        V = tr.eight_corners(dims, 3, dtype)
        t, _ = _run(V)
        check_topology(t, V)
        assert t.euler_number(6)[3] == 8 and t.euler_number(26)[3] == 8 and t.euler_number(6)[0] == 1


# ---- 3. staleness, slabs ------------------------------------------------------------------------------------------------------------
def test_what_makes_the_rows_stale():
    V = rt.block_labels((24, 20, 70), np.uint16, 31, nlabels=40)
    getters = lambda ctx: (ctx.topology_rows, ctx.topology_debug)
    with Pass(V) as p:
        assert code(p.ctx.topology_timing) == _capi.TA_EINVAL and code(p.ctx.topology_rows) == _capi.TA_EINVAL
        assert code(p.ctx.topology_extract) == _capi.TA_EINVAL          # no extraction yet
        p.extract()
        check_pass(p)
        p.ctx.set_signal(rt.random_image(V.shape, np.uint8, 2))         # a new signal: this pass does not read it
        check_pass(p)
        p.ctx.relabel(np.arange(p.max_label + 1, dtype=np.uint32))      # ta_volume_relabel
        assert [code(g) for g in getters(p.ctx)] == [_capi.TA_EINVAL] * 2
        assert code(p.ctx.topology_extract) == _capi.TA_EINVAL
        p.extract()
        check_pass(p)
        p.extract()                                                     # a new extraction, even of the same volume
        assert [code(g) for g in getters(p.ctx)] == [_capi.TA_EINVAL] * 2
        check_pass(p)
        p.ctx.set_volume(V)                                             # a new volume
        assert [code(g) for g in getters(p.ctx)] == [_capi.TA_EINVAL] * 2


def test_a_label_above_max_label_in_an_edited_buffer():
    V = rt.block_labels((24, 20, 70), np.uint16, 31, nlabels=40)
    with Pass(V, adopted=True) as p:
        p.extract()
        check_pass(p)
        poke(p.t, (3, 4, 5), p.max_label + 1)
        p.ctx.topology_extract()
        for get in (p.ctx.topology_rows, p.ctx.topology_debug):
            assert code(get) == _capi.TA_ERANGE
        poke(p.t, (3, 4, 5), V[3, 4, 5])
        p.extract()
        check_pass(p)


def test_a_slab_context_is_refused():
    V = rt.block_labels((12, 10, 40), np.uint16, 35, nlabels=20)
    for first_owned, origin in ((1, 40), (0, 8)):
        t = tensor(V)
        ctx = _capi.Context(0)
        try:
            ctx.set_volume_device(t.data_ptr(), 2, V.shape, a0_origin=origin, has_low_halo=bool(first_owned), keep=t)
            ctx.extract(_capi.F_ALL, int(V.max()))
            assert code(ctx.topology_extract) == _capi.TA_EINVAL
            assert code(ctx.topology_rows) == _capi.TA_EINVAL
        finally:
            ctx.close()


# ---- 4. the analysis methods and the graph ----------------------------------------------------------------------------------------
def test_tunnel_cavity_box_through_the_analysis():
    vs = (0.5, 0.25, 2.0)
    V, info = tr.drilled_voronoi(tr.voronoi((48, 40, 56), 30, 3))
    want = tr.counts(V, int(V.max()) + 1)
    sia = SpatialImageAnalysis(SpatialImage(V, voxelsize=vs), return_type=DICT, background=None)
    t = sia.cell_topology()
    same_counts([getattr(t, k) for k in tr.COLUMNS], want)
    assert sia.cell_topology() is t                           # cached
    found = sia.topological_defects()
    assert found == {info["tunnel"]: {'blobs': 1, 'euler': 0, 'tunnels_minus_cavities': 1},
                     info["cavity"]: {'blobs': 1, 'euler': 2, 'tunnels_minus_cavities': -1}}
    assert sia.topological_defects(exclude=[info["tunnel"]]) == {info["cavity"]: found[info["cavity"]]}
    blobs = sia.label_components().per_label()
    chi = sia.euler_number()
    assert sorted(chi) == sorted(blobs) == sia.labels()
    for l in chi:
        assert isinstance(chi[l], (int, np.integer))
        assert (chi[l] == blobs[l]) == (l not in found), l
    assert chi[info["box"]] == 1 and chi[info["speck"]] == 1
    a, b, c = info["box_dims"]
    assert sia.mean_breadth(info["box"])[info["box"]] == pytest.approx((a * vs[0] + b * vs[1] + c * vs[2]) / 2, rel=1e-12)
    assert sia.mean_breadth([info["box"]], real=False)[info["box"]] == pytest.approx((a + b + c) / 2, rel=1e-12)
    assert sia._resident().uploads == 1
    listed = SpatialImageAnalysis(SpatialImage(V, voxelsize=vs), return_type=NPLIST, background=None)
    assert np.array_equal(listed.euler_number(connectivity=26), tr.euler(want, 26)[listed.labels()])
    # the graph: the column is the class's; a property list without it does not run the pass
    fresh = SpatialImageAnalysis(SpatialImage(V, voxelsize=vs), return_type=DICT, background=1)
    ctx = fresh._resident().ctx
    graph_from_image(fresh, background=1, spatio_temporal_properties=["volume"], ignore_cells_at_stack_margins=False)
    with pytest.raises(_capi.TissueScanError, match="no Euler-number pass has been run"):
        ctx.topology_timing()
    g = graph_from_image(fresh, background=1, spatio_temporal_properties=["volume", "euler_number"], ignore_cells_at_stack_margins=False)
    assert ctx.topology_timing() >= 0
    col, valid = g.vertex_column("euler_number")
    ids = np.asarray(g.vertex_ids)
    assert valid.all() and sorted(ids.tolist()) == fresh.labels() and info["tunnel"] in ids and info["cavity"] in ids
    assert col.tolist() == [fresh.euler_number(l)[l] for l in ids.tolist()] == [chi[l] for l in ids.tolist()]
