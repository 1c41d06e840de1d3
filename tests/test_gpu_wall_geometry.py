"""Wall geometry on the MI355X (include/tissue_scan_wallgeo.h, csrc/kernels_wallgeo.hip) against the NumPy restatement of
tests/wall_geometry_reference.py: every number is an integer and must be bit-exact.

The shapes assume the pass's tiling, which is the signal pass's: 4 rows x 64 * VPL columns x 16 planes, VPL = 8 for uint16 and 4
for uint32."""
import numpy as np
import pytest

import wall_geometry_reference as ref
from tissue_analysis_amd import DICT, SpatialImage, SpatialImageAnalysis, WallGeometry, _capi, graph_from_image, synth, wall_geometry
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu

FIELDS = ("fwd", "rev", "sum1", "sum2")


def check_rows(G, want, faces=None, nonempty=False):
    """G: WallGeometry, or (lo, hi, fwd, rev, sum1, sum2); want: ref.rows(...) of the same image; faces: pair_faces of the same
    extraction."""
    if isinstance(G, WallGeometry):
        assert G.fwd.dtype == np.uint64 and G.sum2.dtype == np.uint64 and G.pair_lo.dtype == np.int64
        got = dict(lo=G.pair_lo, hi=G.pair_hi, fwd=G.fwd, rev=G.rev, sum1=G.sum1, sum2=G.sum2)
    else:
        got = dict(zip(("lo", "hi") + FIELDS, G))
    if nonempty:                                   # (from the reference's table: no case passes on empty tables)
        assert want["lo"].size > 0 and want["sum2"].any()
    assert np.array_equal(np.asarray(got["lo"]).astype(np.int64), want["lo"])
    assert np.array_equal(np.asarray(got["hi"]).astype(np.int64), want["hi"])
    for name in FIELDS:
        assert got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), name
    if faces is not None:
        assert np.array_equal(got["fwd"] + got["rev"], np.asarray(faces).reshape(-1, 3))


def _run(V, sparse=None, nonempty=False, want=None):
    rv = ResidentVolume(V)
    try:
        x = rv.extract(sparse=sparse)
        G = rv.wall_geometry()
        assert G.ms is not None and G.ms >= 0.0
        check_rows(G, ref.rows(V) if want is None else want, x.as_arrays()["pair_faces"], nonempty)
        spills = rv.ctx.wallgeo_spills()
    finally:
        rv.close()
    return G, spills


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
def test_vector_and_scalar_paths_and_partial_tiles(dtype):
    # rows of 531 voxels are not whole 16-byte strips (the scalar path), rows of 528 and 264 are (the vector path); more than one
    # tile and a partial tile along every axis
    for dims in ((19, 7, 531), (19, 7, 528), (33, 10, 264)):
        V = synth.voronoi_labels(dims, 60, 3, dtype=np.uint16).astype(dtype)
        _run(V, nonempty=True)


def test_thin_and_tiny_volumes():
    for dims in ((1, 9, 40), (5, 1, 64), (1, 1, 77), (1, 1, 1)):
        V = synth.voronoi_labels(dims, 6, 3, dtype=np.uint16)
        want = ref.rows(V)
        _run(V, want=want)
        _run(V.astype(np.uint32), want=want)
    G, _ = _run(np.full((5, 6, 7), 3, dtype=np.uint16))                         # one label: no rows, and no failure
    assert len(G) == 0 and G.fwd.shape == (0, 3) and G.sum2.shape == (0, 6)
    A = synth.voronoi_labels((1, 200, 150), 40, 3, dtype=np.uint16)[0]          # a 2-D image through the public function
    want = ref.rows(A)
    assert want["lo"].size > 40
    G = wall_geometry(A.astype(np.int64), voxelsize=(0.5, 0.25))
    check_rows(G, want)
    assert G.voxelsize == (0.5, 0.25, 1.0) and not G.fwd[:, 2].any() and not G.sum1[:, 2].any()
    sia = SpatialImageAnalysis(SpatialImage(A.copy(), voxelsize=(0.5, 0.25)), background=1, return_type=DICT)
    check_rows(sia.wall_geometry(), want)


def test_dense_layouts_other_than_c_order():
    V = synth.voronoi_labels((24, 40, 56), 60, 3, dtype=np.uint16)
    want = ref.rows(V)
    _run(np.asfortranarray(V), want=want, nonempty=True)                        # rows come back in array axes
    VT = V.transpose(1, 2, 0)
    _run(VT, want=ref.rows(VT), nonempty=True)
    _run(np.asfortranarray(V.astype(np.uint32)), want=want)


def test_table_pressure():
    rng = np.random.default_rng(7)
    V = rng.integers(0, 4000, size=(16, 16, 16)).astype(np.uint16)              # more pairs in one workgroup's range than any LDS table holds
    want = ref.rows(V)
    assert want["lo"].size > 10000
    _, spills = _run(V, want=want)
    assert spills > 0
    V = rng.integers(0, 2, size=(24, 24, 40)).astype(np.uint32)                 # one pair owns every face
    want = ref.rows(V)
    assert want["lo"].size == 1 and want["fwd"].sum() + want["rev"].sum() > 0.4 * 3 * 23 * 23 * 39
    _, spills = _run(V, want=want)
    assert spills == 0


def _slab(V, lo, hi):
    """The rows of planes lo .. hi - 1 of V on the device, adopted as a slab (a low halo plane when lo > 0): lo, hi, fwd, rev, sum1,
    sum2 and the pair faces of the extraction."""
    import torch
    halo = lo > 0
    lo_ = lo - 1 if halo else lo
    sub = np.ascontiguousarray(V[lo_:hi])
    t = torch.from_numpy(sub.view(np.int16 if V.dtype == np.uint16 else np.int32).copy()).cuda()
    torch.cuda.synchronize()
    ctx = _capi.Context(0)
    try:
        ctx.set_volume_device(t.data_ptr(), V.dtype.itemsize, t.shape, a0_origin=lo, has_low_halo=halo, keep=t)
        ctx.extract(_capi.F_ALL, int(V.max()))
        plo, phi, faces = ctx.adjacency()
        ctx.wallgeo_extract()
        got = (plo, phi) + ctx.wallgeo_get()
    finally:
        ctx.close()
    want = ref.rows(sub, first_owned=1 if halo else 0, a0_origin=lo)
    check_rows(got, want, faces)
    return got, want


def test_sums_beyond_32_bits():
    V = synth.voronoi_labels((6, 40, 300), 40, 3, dtype=np.uint16)
    import torch
    t = torch.from_numpy(V.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    ctx = _capi.Context(0)
    try:
        ctx.set_volume_device(t.data_ptr(), 2, t.shape, a0_origin=2040, has_low_halo=False, keep=t)
        ctx.extract(_capi.F_ALL, int(V.max()))
        plo, phi, faces = ctx.adjacency()
        ctx.wallgeo_extract()
        got = (plo, phi) + ctx.wallgeo_get()
    finally:
        ctx.close()
    want = ref.rows(V, a0_origin=2040)
    assert (want["sum2"][:, 0] > 2 ** 32).any()
    check_rows(got, want, faces, nonempty=True)


def test_sparse_ids_and_a_compacted_context():
    rng = np.random.default_rng(5)
    ids = np.array([0, 7, 70000, 2**31 + 5, 2**32 - 2, 2**32 - 1], dtype=np.uint32)
    V = ids[rng.integers(0, ids.size, size=(12, 9, 33))]
    want = ref.rows(V)
    assert want["lo"].size == 15 and want["hi"].max() == 2**32 - 1
    rv = ResidentVolume(V)
    try:
        x = rv.extract(sparse=True)
        assert rv.ctx.is_compact() and x.ids is not None
        G = rv.wall_geometry()
        check_rows(G, want, x.as_arrays()["pair_faces"])                         # the Python table answers in ids
        raw = rv.ctx.wallgeo_get()                                              # the raw getter: the extraction's rows
        plo, phi, faces = rv.ctx.adjacency()
        assert len(raw[0]) == rv.ctx.adjacency_size() == 15
        check_rows((plo, phi) + raw, want, faces)
    finally:
        rv.close()


@pytest.fixture(scope="module")
def c1():
    c = synth.CONFIGS["C1"]
    V = synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], np.uint16)
    return V, ref.rows(V)


@pytest.mark.parametrize("cuts", [(37,), (20, 41)])
def test_slabs_with_a_low_halo_merge_to_the_whole(c1, cuts):
    V, whole = c1
    edges = (0,) + tuple(cuts) + (V.shape[0],)
    parts, wants = [], []
    for lo, hi in zip(edges[:-1], edges[1:]):
        got, want = _slab(V, lo, hi)
        parts.append(WallGeometry(*got))
        wants.append(want)
    check_rows(WallGeometry.merge(parts), whole, nonempty=True)
    check_rows(tuple(ref.merge(wants)[k] for k in ("lo", "hi") + FIELDS), whole)


def test_several_ranges_meet_in_the_same_rows():
    # 3 x 50 x 6 tiles, a workgroup range each: the flushes of hundreds of workgroups meet in the rows of 3 000 cells' walls
    import torch
    from tissue_analysis_amd import device as dev
    ctx = dev.torch_context(0)
    try:
        v, top = dev.synth_slab(ctx, (96, 200, 600), np.dtype("uint32"), 3000, 3)           # (made on the device: seconds on the host)
        torch.cuda.synchronize()
        ctx.set_volume_device(v.data_ptr(), 4, v.shape, keep=v)
        ctx.extract(_capi.F_ALL, top)
        plo, phi, faces = ctx.adjacency()
        ctx.wallgeo_extract()
        got = (plo, phi) + ctx.wallgeo_get()
        V = v.cpu().numpy().view(np.uint32)
    finally:
        ctx.close()
    want = ref.rows(V)
    assert want["lo"].size > 5000
    check_rows(got, want, faces, nonempty=True)


def _einval(call, *args):
    with pytest.raises(_capi.TissueScanError) as e:
        call(*args)
    assert e.value.code == _capi.TA_EINVAL


def test_argument_checks_and_invalidation():
    V = synth.voronoi_labels((10, 12, 40), 30, 3, dtype=np.uint16)
    want = ref.rows(V)
    ctx = _capi.Context(0)
    try:
        _einval(ctx.wallgeo_extract)                                # no volume
        ctx.set_volume(V)
        _einval(ctx.wallgeo_extract)                                # no extraction
        ctx.extract(_capi.F_ALL & ~_capi.F_ADJACENCY, int(V.max()))
        _einval(ctx.wallgeo_extract)                                # an extraction without adjacency
        ctx.extract(_capi.F_ALL, int(V.max()))
        lib, h = ctx._lib, ctx._h
        assert lib.ta_wallgeo_get(h, None, None, None, None) == _capi.TA_EINVAL      # a getter before the pass
        _einval(ctx.wallgeo_timing)
        _einval(ctx.wallgeo_spills)
        ctx.wallgeo_extract()
        plo, phi, faces = ctx.adjacency()
        check_rows((plo, phi) + ctx.wallgeo_get(), want, faces, nonempty=True)
        assert lib.ta_wallgeo_get(h, None, None, None, None) == _capi.TA_OK          # any pointer may be NULL
        s2 = np.zeros((len(plo), 6), dtype=np.uint64)
        assert lib.ta_wallgeo_get(h, None, None, None, s2.ctypes.data) == _capi.TA_OK
        assert np.array_equal(s2, want["sum2"])
        assert lib.ta_wallgeo_spills(h, None) == _capi.TA_OK
        assert ctx.wallgeo_timing() > 0.0
        ctx.extract(_capi.F_ALL, int(V.max()))                      # a new ta_extract: stale until the pass is re-run
        assert lib.ta_wallgeo_get(h, None, None, None, None) == _capi.TA_EINVAL
        ctx.wallgeo_extract()
        check_rows((plo, phi) + ctx.wallgeo_get(), want)
        lut = np.arange(int(V.max()) + 1, dtype=np.uint32)
        lut[5] = 3                                                  # two cells fused
        ctx.relabel(lut)                                            # ta_volume_relabel
        assert lib.ta_wallgeo_get(h, None, None, None, None) == _capi.TA_EINVAL
        _einval(ctx.wallgeo_extract)                                # ... and the extraction is gone too
        ctx.extract(_capi.F_ALL, int(V.max()))
        ctx.wallgeo_extract()
        plo, phi, faces = ctx.adjacency()
        check_rows((plo, phi) + ctx.wallgeo_get(), ref.rows(lut[V]), faces)
        ctx.set_volume(np.ascontiguousarray(V[:, :, :32]))          # a new volume
        assert lib.ta_wallgeo_get(h, None, None, None, None) == _capi.TA_EINVAL
        _einval(ctx.wallgeo_extract)
    finally:
        ctx.close()


def test_through_the_analysis_class(c1):
    V, whole = c1
    vs = (0.5, 0.25, 2.0)
    sia = SpatialImageAnalysis(SpatialImage(V.copy(), voxelsize=vs), background=1, return_type=DICT)
    plain = graph_from_image(sia, spatio_temporal_properties=['barycenter', 'wall_surface'], ignore_cells_at_stack_margins=False)
    assert getattr(sia, "_wall_geometry", None) is None                         # no geometry property: the pass has not run
    _einval(sia._resident().ctx.wallgeo_timing)
    G = sia.wall_geometry()
    check_rows(G, whole, sia.extraction.as_arrays()["pair_faces"], nonempty=True)
    assert sia.wall_geometry() is G and G.voxelsize == vs                       # cached
    areas, proj = sia.wall_areas(), sia.wall_projected_areas()
    assert list(proj.keys()) == list(areas.keys()) and len(proj) > 100
    assert all(proj[k] <= areas[k] * (1 + 1e-12) for k in proj)
    normals = sia.wall_normals()
    assert list(normals.keys()) == list(areas.keys())
    k = next(iter(normals))
    r = int(G.wall_rows([k[0]], [k[1]])[0])
    assert np.array_equal(normals[k], G.normal()[r]) and proj[k] == G.projected_area()[r]
    assert sia.wall_projected_areas(real=False)[k] == G.projected_area(real=False)[r]
    some = {k[0]: [k[1]]}
    assert list(sia.wall_normals(some).keys()) == [k]
    # the graph: the same vectors on its edges; without the properties the identical graph
    g = graph_from_image(sia, spatio_temporal_properties=['barycenter', 'wall_surface', 'wall_normal', 'wall_centroid', 'wall_projected_area'],
                         ignore_cells_at_stack_margins=False)
    assert np.array_equal(g.edge_sources, plain.edge_sources) and np.array_equal(g.edge_targets, plain.edge_targets)
    assert sorted(plain.edge_property_names()) == sorted(n for n in g.edge_property_names() if not n.startswith('wall_')
                                                          or n == 'wall_surface')
    rows = G.wall_rows(g.edge_sources, g.edge_targets)
    assert (rows >= 0).all() and rows.size > 100
    assert np.array_equal(g.edge_column('wall_normal')[0], G.normal()[rows], equal_nan=True)
    assert np.array_equal(g.edge_column('wall_centroid')[0], G.centroid()[rows])
    assert np.array_equal(g.edge_column('wall_projected_area')[0], G.projected_area()[rows])
    assert all(g.edge_column(n)[1].all() for n in ('wall_normal', 'wall_centroid', 'wall_projected_area'))
    assert np.array_equal(g.edge_column('wall_surface')[0], plain.edge_column('wall_surface')[0])
    # an edit of the labels: the cached table goes, the rows on the context are invalid, the next ones describe the new image
    gone = sorted(set(int(l) for l in whole["hi"][-2:] if int(l) != 1))
    sia.remove_labels_from_image(list(gone), verbose=False)
    assert sia._resident().ctx._lib.ta_wallgeo_get(sia._resident().ctx._h, None, None, None, None) == _capi.TA_EINVAL
    G2 = sia.wall_geometry()
    assert G2 is not G
    W = V.copy()
    W[np.isin(W, gone)] = 0
    check_rows(G2, ref.rows(W))
    sia.image[0, :, :] = 1                                          # in place, then refresh()
    sia.refresh()
    W[0, :, :] = 1
    check_rows(sia.wall_geometry(), ref.rows(W), sia.extraction.as_arrays()["pair_faces"])
