"""Cell junctions on the MI355X (include/tissue_scan_junctions.h, csrc/kernels_junctions.hip) against the NumPy restatement of
tests/junction_reference.py: every number is an integer and must be bit-exact."""
import numpy as np
import pytest

import junction_reference as ref
from tissue_analysis_amd import DICT, CellJunctions, SpatialImageAnalysis, _capi, cell_junctions, synth
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu


def check_tables(J, want, nonempty=False):
    """J: CellJunctions (or the tuple of Context.junctions_get); want: ref.tables(...) of the same image."""
    if isinstance(J, CellJunctions):
        assert J.edge_labels.dtype == np.int64 and J.edge_n.dtype == np.uint64 and J.edge_sum.dtype == np.uint64
        got = ((J.edge_labels, J.edge_n, J.edge_sum), (J.vertex_labels, J.vertex_n, J.vertex_sum), J.degenerate)
    else:
        got = J
    (el, en, es), (vl, vn, vs), deg = want
    if nonempty:                                   # (from the reference's table: no case passes on empty tables)
        assert en.size > 0 and vn.size > 0 and deg > 0
    for k, width in ((0, 3), (1, 4)):
        assert got[k][0].shape == want[k][0].shape == (want[k][1].size, width)
        assert np.array_equal(got[k][0], want[k][0])
        assert np.array_equal(got[k][1], want[k][1])
        assert got[k][2].shape == want[k][2].shape and np.array_equal(got[k][2], want[k][2])
    assert got[2] == deg


def _run(V):
    rv = ResidentVolume(V)
    try:
        J = rv.junctions()
        assert J.ms is not None and J.ms[0] > 0.0 and J.ms[1] >= 0.0
    finally:
        rv.close()
    return J


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
def test_label_types_and_edge_tiles(dtype):
    # a task is 2 block rows x 512 (uint16) or 256 (uint32) block columns x 16 block planes: partial tasks on every axis; rows of
    # 531 voxels are not whole 16-byte strips (the scalar path), rows of 528 and 264 are (the vector path)
    for dims in ((19, 7, 531), (19, 7, 528), (33, 10, 264)):
        V = synth.voronoi_labels(dims, 60, 3, dtype=np.uint16).astype(dtype)
        check_tables(_run(V), ref.tables(V), nonempty=True)


def test_thin_and_tiny_volumes():
    for dims in ((1, 9, 40), (5, 1, 64), (1, 1, 77), (1, 1, 1)):
        V = synth.voronoi_labels(dims, 6, 3, dtype=np.uint16)
        want = ref.tables(V)
        check_tables(_run(V), want)
        check_tables(_run(V.astype(np.uint32)), want)
    J = _run(synth.voronoi_labels((1, 1, 77), 6, 3, dtype=np.uint16))          # blocks of two voxels: no rows, and no failure
    assert J.edge_labels.shape == (0, 3) and J.vertex_labels.shape == (0, 4) and J.degenerate == 0
    V = np.arange(1, 9, dtype=np.uint16).reshape(2, 2, 2)
    J = _run(V)
    check_tables(J, ref.tables(V))
    assert J.degenerate == 1 and len(J.edge_n) == 0 and len(J.vertex_n) == 0
    A = synth.voronoi_labels((1, 200, 150), 40, 3, dtype=np.uint16)[0]          # a 2-D image through the public function
    want = ref.tables(A)
    assert want[0][1].size > 0 and want[1][1].size > 0 and want[2] == 0
    J = cell_junctions(A.astype(np.int64), voxelsize=(0.5, 0.25))
    check_tables(J, want)
    assert not J.edge_sum[:, 2].any() and J.voxelsize == (0.5, 0.25, 1.0)


def test_dense_layouts_other_than_c_order():
    V = synth.voronoi_labels((24, 40, 56), 60, 3, dtype=np.uint16)
    want = ref.tables(V)
    assert want[1][1].size > 0
    check_tables(_run(np.asfortranarray(V)), want)                              # positions come back in array axes
    VT = V.transpose(1, 2, 0)
    check_tables(_run(VT), ref.tables(VT))
    check_tables(_run(np.asfortranarray(V.astype(np.uint32))), want)


def test_noise_and_sizing():
    rng = np.random.default_rng(7)
    V = rng.integers(0, 6, size=(24, 24, 40)).astype(np.uint16)                 # every triple and quadruple of six labels
    want = ref.tables(V)
    assert want[0][1].size == 20 and want[1][1].size == 15 and want[2] > 0.4 * 23 * 23 * 39
    check_tables(_run(V), want)
    V = rng.integers(0, 3, size=(24, 24, 40)).astype(np.uint32)                 # one triple holds most blocks: one huge segment
    want = ref.tables(V)
    assert want[0][1].tolist()[0] > 0.8 * 23 * 23 * 39 and want[0][1].size == 1 and want[1][1].size == 0
    check_tables(_run(V), want)
    V = rng.integers(0, 4000, size=(16, 16, 16)).astype(np.uint16)              # every block degenerate
    want = ref.tables(V)
    assert want[2] > 0.99 * 15 ** 3
    check_tables(_run(V), want)


def test_sparse_ids_and_a_compacted_context():
    rng = np.random.default_rng(5)
    ids = np.array([0, 7, 70000, 2**31 + 5, 2**32 - 2, 2**32 - 1], dtype=np.uint32)
    V = ids[rng.integers(0, ids.size, size=(12, 9, 33))]
    want = ref.tables(V)
    assert want[0][1].size == 20 and want[1][1].size == 15 and want[1][0].max() == 2**32 - 1
    rv = ResidentVolume(V)
    try:
        check_tables(rv.junctions(), want)
        x = rv.extract(sparse=True)
        assert rv.ctx.is_compact() and x.ids is not None
        check_tables(rv.junctions(), want)                                       # rows of the sweep are ranks, the tables speak in ids
        rv.ctx.uncompact()
        check_tables(rv.junctions(), want)
    finally:
        rv.close()


@pytest.fixture(scope="module")
def c1():
    c = synth.CONFIGS["C1"]
    V = synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], np.uint16)
    return V, ref.tables(V)


@pytest.mark.parametrize("cuts", [(37,), (20, 41)])
def test_slabs_with_a_low_halo_merge_to_the_whole(c1, cuts):
    import torch
    V, whole = c1
    edges = (0,) + tuple(cuts) + (V.shape[0],)
    parts = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        halo = lo > 0
        lo_ = lo - 1 if halo else lo
        t = torch.from_numpy(V[lo_:hi].view(np.int16).copy()).cuda()
        torch.cuda.synchronize()
        ctx = _capi.Context(0)
        try:
            ctx.set_volume_device(t.data_ptr(), 2, t.shape, a0_origin=lo, has_low_halo=halo, keep=t)
            ctx.junctions_extract()
            got = ctx.junctions_get()
        finally:
            ctx.close()
        check_tables(got, ref.tables(V[lo_:hi], first_owned=1 if halo else 0, a0_origin=lo))
        parts.append(tuple((g[0].astype(np.int64), g[1], g[2]) for g in got[:2]) + (got[2],))
    check_tables(ref.merge(parts), whole, nonempty=True)
    J = CellJunctions.merge([CellJunctions(p[0][0], p[0][1], p[0][2], p[1][0], p[1][1], p[1][2], p[2]) for p in parts])
    check_tables(J, whole)


def _einval(call, *args):
    with pytest.raises(_capi.TissueScanError) as e:
        call(*args)
    assert e.value.code == _capi.TA_EINVAL


def test_argument_checks_and_invalidation():
    V = synth.voronoi_labels((10, 12, 40), 30, 3, dtype=np.uint16)
    ctx = _capi.Context(0)
    try:
        _einval(ctx.junctions_extract)                              # no volume
        ctx.set_volume(V)
        _einval(ctx.junctions_size)                                 # no pass yet
        _einval(ctx.junctions_get)
        _einval(ctx.junctions_timing)
        lib, h = ctx._lib, ctx._h
        assert lib.ta_junctions_get_edges(h, None, None, None) == _capi.TA_EINVAL
        ctx.junctions_extract()
        check_tables(ctx.junctions_get(), ref.tables(V))
        assert lib.ta_junctions_get_edges(h, None, None, None) == _capi.TA_OK            # any pointer may be NULL
        assert lib.ta_junctions_get_vertices(h, None, None, None) == _capi.TA_OK
        assert lib.ta_junctions_size(h, None, None, None) == _capi.TA_OK
        ms_pass, ms_after = ctx.junctions_timing()
        assert ms_pass > 0.0 and ms_after > 0.0
        lut = np.arange(int(V.max()) + 1, dtype=np.uint32)
        lut[2:] += 100
        lut[5] = 3                                                  # two cells fused
        ctx.relabel(lut)                                            # ta_volume_relabel
        _einval(ctx.junctions_size)
        _einval(ctx.junctions_get)
        ctx.junctions_extract()
        check_tables(ctx.junctions_get(), ref.tables(lut[V]))
        ctx.set_volume(V)                                           # a new volume
        _einval(ctx.junctions_size)
        assert lib.ta_junctions_get_vertices(h, None, None, None) == _capi.TA_EINVAL
        ctx.junctions_extract()
        ctx.set_volume(np.ascontiguousarray(V[:, :, :32]))          # a new volume while the counting walk is the only thing done
        _einval(ctx.junctions_get)
        ctx.junctions_extract()
        check_tables(ctx.junctions_get(), ref.tables(V[:, :, :32]))
    finally:
        ctx.close()


def test_analysis_cross_check_and_invalidation_by_an_image_edit(c1):
    V, whole = c1
    vs = (0.5, 0.25, 2.0)
    from tissue_analysis_amd import SpatialImage
    sia = SpatialImageAnalysis(SpatialImage(V.copy(), voxelsize=vs), background=1, return_type=DICT)
    J = sia.cell_junctions()
    check_tables(J, whole, nonempty=True)
    assert sia.cell_junctions() is J                                # cached
    assert J.voxelsize == vs
    known = set(sia.labels()) | set(sia.ignoredlabels()) | {sia.background()}
    assert set(np.unique(J.edge_labels).tolist()) <= known and set(np.unique(J.vertex_labels).tolist()) <= known
    verts = sia.cell_vertices()
    assert len(verts) == whole[1][1].size
    for labels, n, s in zip(whole[1][0].tolist(), whole[1][1].tolist(), whole[1][2].tolist()):
        want = np.array(s, dtype=np.float64) / (2.0 * n) * np.array(vs)
        assert np.abs(verts[tuple(labels)] - want).max() <= 1e-12
    vox = sia.cell_vertices(real=False)
    k = tuple(whole[1][0][0].tolist())
    assert np.array_equal(vox[k], whole[1][2][0] / (2.0 * float(whole[1][1][0])))
    # an edit of the labels: the cached tables go, the tables on the context are invalid, the next ones describe the new image
    gone = [int(l) for l in whole[1][0][0][-2:] if int(l) != 1]
    sia.remove_labels_from_image(list(gone), verbose=False)
    _einval(sia._resident().ctx.junctions_size)
    J2 = sia.cell_junctions()
    assert J2 is not J
    W = V.copy()
    W[np.isin(W, gone)] = 0
    check_tables(J2, ref.tables(W))
    assert not np.isin(J2.vertex_labels, gone).any()
    sia.image[0, :, :] = 1                                          # in place, then refresh()
    sia.refresh()
    W[0, :, :] = 1
    check_tables(sia.cell_junctions(), ref.tables(W))


def test_full_size_512_cubed_against_the_reference_by_plane_pairs():
    import torch
    from tissue_analysis_amd import device as dev
    c = synth.CONFIGS["C2"]
    dtype = np.dtype("uint16")
    ctx = dev.torch_context(0)
    try:
        v, _ = dev.synth_slab(ctx, c["dims"], dtype, c["n_cells"], c["seed"])
        torch.cuda.synchronize()
        ctx.set_volume_device(v.data_ptr(), 2, v.shape, keep=v)
        ctx.junctions_extract()
        got = ctx.junctions_get()
        V = v.cpu().numpy().view(dtype)
    finally:
        ctx.close()
    check_tables(got, ref.tables_by_plane_pairs(V, planes=2), nonempty=True)
