"""Cell meshes on the MI355X (include/tissue_scan_mesh.h, csrc/kernels_mesh.hip) against the NumPy restatement of
tests/mesh_reference.py -- bit-identical, array for array, order included -- and, at 512^3, against the sweep's own per-cell
results (voxel counts, faces per wall, centres of mass)."""
import numpy as np
import pytest

import mesh_reference as ref
from tissue_analysis_amd import CellMeshes, SpatialImageAnalysis, _capi, synth
from tissue_analysis_amd import device as dev
from tissue_analysis_amd.cell_meshes import (spatial_image_analysis_to_cell_triangular_meshes,
                                             spatial_image_analysis_to_triangular_mesh)
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu

A = np.array([[1, 2, 7, 7, 1, 1],
              [1, 6, 5, 7, 3, 3],
              [2, 2, 1, 7, 3, 3],
              [1, 1, 1, 4, 1, 1]], dtype=np.uint16)
FIELDS = ("labels", "points", "triangles", "triangle_cell", "triangle_neighbor", "vertex_offsets", "triangle_offsets")


def device_meshes(V, labels=None, sub_factor=1, voxelsize=(1.0, 1.0, 1.0), sparse=None):
    rv = ResidentVolume(V)
    try:
        rv.extract(sparse=sparse)
        m = rv.meshes(labels, sub_factor, voxelsize)
    finally:
        rv.close()
    assert isinstance(m, CellMeshes)
    return m


def assert_identical(m, r):
    for k in FIELDS:
        got, want = getattr(m, k), r[k]
        assert got.shape == want.shape, (k, got.shape, want.shape)
        assert np.array_equal(got, want.astype(got.dtype)), k
    assert m.points.dtype == np.float64 and m.triangles.dtype == np.uint32


def check(V, labels=None, sub_factor=1, voxelsize=(1.0, 1.0, 1.0), sparse=None):
    m = device_meshes(V, labels, sub_factor, voxelsize, sparse)
    assert_identical(m, ref.mesh(V, labels, sub_factor, voxelsize))
    return m


def tri_set(m):
    """{(cell, neighbour, corner triple as points)}: the triangles of a mesh as a set, independent of order."""
    p = m.points[m.triangles.astype(np.int64)]
    return set(zip(m.triangle_cell.tolist(), m.triangle_neighbor.tolist(), map(lambda x: x.tobytes(), p)))


def test_docstring_image():
    check(A)
    check(A, labels=[1, 2, 3, 4, 5, 6, 7], voxelsize=(0.5, 0.25, 1.0))


def test_voronoi_tissue_uint16_and_uint32():
    for dims, n, seed in (((64, 64, 64), 60, 3), ((96, 80, 128), 150, 4)):
        V16 = synth.voronoi_labels(dims, n, seed, np.uint16)
        for dt in (np.uint16, np.uint32):
            V = V16.astype(dt)
            check(V)
            check(V, labels=np.unique(V)[1:].tolist())


def test_sparse_ids_above_2_16():
    V16 = synth.voronoi_labels((48, 40, 56), 40, 5, np.uint16)
    V = (V16.astype(np.uint32) * 70001 + (V16 > 0) * 3).astype(np.uint32)
    ids = np.unique(V)
    assert ids[-1] > (1 << 16)
    m = check(V, sparse=True)
    assert m.labels[-1] > (1 << 16)
    check(V, labels=ids[1::3].tolist(), sparse=True)


def test_sub_factor_on_dims_not_divisible():
    V = synth.voronoi_labels((37, 41, 50), 30, 6, np.uint16)
    for s in (2, 3):
        check(V, sub_factor=s, voxelsize=(0.7, 1.1, 0.3))
        check(V.astype(np.uint32), labels=[1, 2, 5, 9], sub_factor=s)


def test_labels_subset_and_explicit_background():
    V = synth.voronoi_labels((40, 44, 36), 35, 7, np.uint16)
    labs = np.unique(V)
    check(V, labels=labs[1::5].tolist())
    check(V, labels=[0])
    check(V, labels=[0] + labs[2::7].tolist())
    check(V, labels=[])


def test_borders_single_voxels_cavity_and_edge_contacts():
    V = np.zeros((7, 8, 9), dtype=np.uint16)
    V[:, :, :] = 1                    # one cell touching all six stack borders...
    V[2:5, 2:6, 3:7] = 2              # ...around a cell with a cavity
    V[3, 3:5, 4:6] = 3
    V[0, 0, 0] = 4                    # single-voxel cells
    V[6, 7, 8] = 5
    V[1, 1, 1] = 6                    # cells touching only along an edge
    V[2, 2, 1] = 7
    V[6, 0, 4] = 8                    # ... and only at a corner
    V[5, 1, 5] = 9
    check(V)
    check(V.astype(np.uint32), labels=[2, 3, 6, 7])


def test_2d_image():
    V = synth.voronoi_labels((60, 50, 1), 20, 8, np.uint16)[:, :, 0]
    check(V)
    check(A.astype(np.uint32), labels=[1, 7], sub_factor=2)


def test_f_ordered_input_gives_the_same_sets_and_calls_repeat():
    V = synth.voronoi_labels((30, 34, 26), 25, 9, np.uint16)
    F = np.asfortranarray(V)
    for s in (1, 2):
        c, f = device_meshes(V, sub_factor=s), device_meshes(F, sub_factor=s)
        assert np.array_equal(c.labels, f.labels)
        assert np.array_equal(c.vertex_offsets, f.vertex_offsets) and np.array_equal(c.triangle_offsets, f.triangle_offsets)
        for i in range(c.labels.size):
            v0, v1 = int(c.vertex_offsets[i]), int(c.vertex_offsets[i + 1])
            a = c.points[v0:v1]
            b = f.points[v0:v1]
            assert sorted(map(tuple, a.tolist())) == sorted(map(tuple, b.tolist()))
        assert tri_set(c) == tri_set(f)
    rv = ResidentVolume(V)
    try:
        rv.extract()
        a, b = rv.meshes(), rv.meshes()
    finally:
        rv.close()
    for k in FIELDS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_512_cube_against_the_sweep():
    c = synth.CONFIGS["C2"]
    dims = c["dims"]
    ctx = dev.torch_context(0)
    try:
        vol, L = dev.synth_slab(ctx, dims, np.uint16, c["n_cells"], c["seed"])
        ctx.set_volume_device(vol.data_ptr(), 2, vol.shape, keep=vol)
        ctx.extract(_capi.F_ALL, L)
        count, _, sum1, _ = ctx.labels()
        lo, hi, faces = ctx.adjacency()
        cells, voff, toff, corners, tri, tcell, tnb, ms = ctx.mesh(1)
    finally:
        ctx.close()
    R = L + 1
    present = np.flatnonzero(count)
    assert np.array_equal(cells.astype(np.int64), present)
    g = tuple(int(d) + 1 for d in dims)
    K = np.stack(np.unravel_index(corners.astype(np.int64), g), axis=1).astype(np.int64)
    t = tri.astype(np.int64)
    cell = tcell.astype(np.int64)
    a, b, cc = K[t[:, 0]], K[t[:, 1]], K[t[:, 2]]
    det = np.einsum("ij,ij->i", a, np.cross(b, cc))
    # enclosed volume, in integers
    six = np.zeros(R, dtype=np.int64)
    np.add.at(six, cell, det)
    assert np.array_equal(six, 6 * count.astype(np.int64))
    # faces per axis and per neighbour (one face = two triangles; the axis is the one the first triangle's normal is along)
    f = slice(0, None, 2)
    normal = np.cross(b[f] - a[f], cc[f] - a[f])
    axis = np.argmax(np.abs(normal), axis=1)
    nb = tnb[f].astype(np.int64)
    inner = tnb[f] != _capi.MESH_OUTSIDE
    got = np.zeros((R, 3), dtype=np.int64)
    np.add.at(got, (cell[f][inner], axis[inner]), 1)
    want = np.zeros((R, 3), dtype=np.int64)
    fa = faces.astype(np.int64)
    np.add.at(want, lo.astype(np.int64), fa)
    np.add.at(want, hi.astype(np.int64), fa)
    assert np.array_equal(got, want)
    key = cell[f][inner] * R + nb[inner]
    uk, n = np.unique(key, return_counts=True)
    pk = np.concatenate([lo.astype(np.int64) * R + hi, hi.astype(np.int64) * R + lo])
    pf = np.concatenate([fa.sum(axis=1), fa.sum(axis=1)])
    order = np.argsort(pk)
    assert np.array_equal(uk, pk[order]) and np.array_equal(n, pf[order])
    # divergence-theorem centroid == center of mass (voxel units; corner K sits at K - 1/2)
    mom = np.zeros((R, 3))
    for k in range(3):
        np.add.at(mom[:, k], cell, (det * (a[:, k] + b[:, k] + cc[:, k])).astype(np.float64))
    cen = mom[present] / (4.0 * six[present, None]) - 0.5
    com = sum1.astype(np.float64).reshape(R, -1)[present, :3] / count[present, None].astype(np.float64)
    np.testing.assert_allclose(cen, com, rtol=1e-9, atol=1e-9)
    assert ms > 0


def test_sia_cell_meshes_and_reference_functions():
    sia = SpatialImageAnalysis(A, background=1)
    m = sia.cell_meshes()
    assert m.labels.tolist() == sia.labels() and 1 not in m
    assert sia.cell_meshes() is m
    pts, tri = m[7]
    assert pts.shape[1] == 3 and tri.shape[1] == 3 and tri.max() < len(pts)
    assert_identical(m, ref.mesh(A, sia.labels()))
    sub = sia.cell_meshes([2, 7], sub_factor=2)
    assert set(sub) <= {2, 7}
    cm = spatial_image_analysis_to_cell_triangular_meshes(sia, labels=[2, 3])
    assert sorted(cm) == [2, 3]
    mesh, matching = spatial_image_analysis_to_triangular_mesh(sia, 'volume')
    assert mesh.points.shape == m.points.shape and mesh.triangles.shape == m.triangles.shape
    assert len(matching) == len(mesh.triangle_data) == len(m.triangles)
    vol = sia.volume()
    assert all(mesh.triangle_data[t] == vol[c] for t, c in matching.items())
    _, matching = spatial_image_analysis_to_triangular_mesh(sia, None, labels=[2])
    mesh, _ = spatial_image_analysis_to_triangular_mesh(sia, {2: 5.0, 3: 6.0}, labels=[2, 3])
    assert set(mesh.triangle_data.values()) == {5.0, 6.0}
    mesh, matching = spatial_image_analysis_to_triangular_mesh(sia, 'neighborhood_size')
    assert len(matching) == len(m.triangles)
    sia.refresh()
    assert sia.cell_meshes() is not m


def as_meshes(r):
    """The reference's dict as a CellMeshes (for comparisons that go through tri_set)."""
    return CellMeshes(r["labels"], r["points"], r["triangles"], r["triangle_cell"], r["triangle_neighbor"], r["vertex_offsets"],
                      r["triangle_offsets"])


def assert_same_sets(m, r):
    """Cells, offsets and each cell's vertices identical (the vertex order holds in every layout); the faces as a set."""
    w = as_meshes(r)
    assert np.array_equal(m.labels, w.labels)
    assert np.array_equal(m.vertex_offsets, w.vertex_offsets) and np.array_equal(m.triangle_offsets, w.triangle_offsets)
    for i in range(w.labels.size):
        v0, v1 = int(w.vertex_offsets[i]), int(w.vertex_offsets[i + 1])
        assert sorted(map(tuple, m.points[v0:v1].tolist())) == sorted(map(tuple, w.points[v0:v1].tolist()))
    assert np.array_equal(m.points, w.points)
    assert tri_set(m) == tri_set(w)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 77), (1, 9, 40), (5, 1, 64), (3, 5, 1031), (2, 2, 2100)])
def test_thin_and_tiny_volumes_and_rows_longer_than_a_wave(shape):
    """(3, 5, 1031), (2, 2, 2100): a wave's 1024 voxels end inside a row, and the rows of the corner grid (1032, 2101) wrap
    inside a step of 64 lanes."""
    rng = np.random.default_rng(sum(shape))
    for dt in (np.uint16, np.uint32):
        V = synth.voronoi_labels(shape, max(1, int(np.prod(shape)) // 60), 3, dt, ellipsoid=False)
        m = check(V)
        assert len(m.triangles) >= 12
        check(rng.integers(1, 4, size=shape).astype(dt))
        check(V, sub_factor=2)
    if int(np.prod(shape)) > 1:
        assert np.unique(V).size > 1


def test_noise_and_a_uniform_volume():
    rng = np.random.default_rng(12)
    V = rng.integers(0, 6, size=(12, 14, 40)).astype(np.uint16)           # nearly every face a boundary, corners with many cells
    m = check(V)
    assert len(m.triangles) > 2 * 2.4 * V.size                            # (5/6 of the inner faces, counted from both sides)
    check(V.astype(np.uint32), labels=[0, 3, 5])
    V = rng.integers(0, 4000, size=(10, 10, 16)).astype(np.uint16)        # every face a boundary, up to eight cells a corner
    m = check(V)
    assert len(m.triangles) >= 2 * 5.99 * V.size and len(m.labels) > 1200
    check(V.astype(np.uint32))
    for dt in (np.uint16, np.uint32):
        V = np.full((9, 6, 70), 5, dtype=dt)                              # one cell: only border faces
        m = check(V)
        assert m.labels.tolist() == [5] and (m.triangle_neighbor == -1).all()
        assert len(m.triangles) == 4 * (9 * 6 + 9 * 70 + 6 * 70)


def test_sub_factors_of_the_reference_and_beyond_the_dims():
    V = synth.voronoi_labels((37, 41, 50), 30, 6, np.uint16)
    for s in (4, 6):                                                      # what the reference subsamples by
        check(V, sub_factor=s, voxelsize=(0.7, 1.1, 0.3))
        check(V.astype(np.uint32), labels=[1, 2, 5, 9], sub_factor=s)
    for s in (50, 64):                                                    # W is the single voxel V[0, 0, 0]
        m = check(V, sub_factor=s)
        assert m.labels.tolist() == [int(V[0, 0, 0])] and len(m.points) == 8 and len(m.triangles) == 12
    check(V, sub_factor=41)                                               # W = V[::41, 0:1, ::41]: (1, 1, 2)
    for X in (np.asfortranarray(V), np.transpose(V, (1, 0, 2)), np.transpose(V.astype(np.uint32), (2, 0, 1))):
        assert not X.flags.c_contiguous
        for s in (1, 3):
            assert_same_sets(device_meshes(X, sub_factor=s), ref.mesh(X, sub_factor=s))


def _code(code, call, *args):
    with pytest.raises(_capi.TissueScanError) as e:
        call(*args)
    assert e.value.code == code


def _einval(call, *args):
    _code(_capi.TA_EINVAL, call, *args)


def context_meshes(ctx, sub_factor=1, wanted_rows=None, ids=None):
    """Context.mesh as a CellMeshes of unit voxels (rows are ids unless `ids` maps them)."""
    cells, voff, toff, corners, tri, tcell, tnb, ms = ctx.mesh(sub_factor, wanted_rows)
    assert ms > 0.0
    name = (lambda r: r.astype(np.int64)) if ids is None else (lambda r: ids[r.astype(np.int64)].astype(np.int64))
    nb = np.full(tnb.shape, -1, dtype=np.int64)
    nb[tnb != _capi.MESH_OUTSIDE] = name(tnb[tnb != _capi.MESH_OUTSIDE])
    g = tuple(-(-int(n) // sub_factor) + 1 for n in ctx._vol_layout[0])
    K = np.stack(np.unravel_index(corners.astype(np.int64), g), axis=1).astype(np.float64)
    return CellMeshes(name(cells), (K - 0.5) * sub_factor, tri, name(tcell), nb, voff, toff, sub_factor=sub_factor, ms=ms)


def test_argument_checks_and_invalidation():
    import torch
    V = synth.voronoi_labels((10, 12, 40), 30, 3, dtype=np.uint16)
    top = int(V.max())
    ctx = _capi.Context(0)
    try:
        lib, h = ctx._lib, ctx._h
        _einval(ctx.mesh)                                           # no volume
        _einval(ctx.mesh_timing)                                    # no pass has ever run
        ctx.set_volume(V)
        _einval(ctx.mesh)                                           # a volume, but no ta_extract yet
        assert lib.ta_mesh_size(h, None, None, None) == _capi.TA_EINVAL
        assert lib.ta_mesh_get(h, None, None, None, None, None, None, None) == _capi.TA_EINVAL
        _einval(ctx.mesh_timing)
        ctx.extract(_capi.F_ALL, top)
        _einval(ctx.mesh, 0)                                        # sub_factor 0
        _einval(ctx.mesh, -2)
        assert lib.ta_mesh_size(h, None, None, None) == _capi.TA_EINVAL           # an extraction, but no mesh pass yet
        assert lib.ta_mesh_get(h, None, None, None, None, None, None, None) == _capi.TA_EINVAL
        _einval(ctx.mesh_timing)
        with pytest.raises(ValueError):
            ctx.mesh(1, np.ones(top, dtype=np.uint8))               # wanted_rows: one byte per row, top + 1 of them
        with pytest.raises(ValueError):
            ctx.mesh(1, np.ones(top + 2, dtype=np.uint8))
        assert_identical(context_meshes(ctx), ref.mesh(V))
        assert lib.ta_mesh_size(h, None, None, None) == _capi.TA_OK               # any pointer may be NULL
        assert lib.ta_mesh_get(h, None, None, None, None, None, None, None) == _capi.TA_OK
        assert ctx.mesh_timing() > 0.0

        def getters_refuse():
            assert lib.ta_mesh_size(h, None, None, None) == _capi.TA_EINVAL
            assert lib.ta_mesh_get(h, None, None, None, None, None, None, None) == _capi.TA_EINVAL

        ctx.extract(_capi.F_VOLUME, top + 3)                        # a new ta_extract: other rows
        getters_refuse()
        wanted = np.zeros(top + 4, dtype=np.uint8)
        wanted[[1, 4, top, top + 2]] = 1
        assert_identical(context_meshes(ctx, 1, wanted), ref.mesh(V, [1, 4, top, top + 2]))
        lut = np.arange(top + 1, dtype=np.uint32)
        lut[2:] += 100
        lut[5] = 3                                                  # two cells fused
        ctx.relabel(lut)                                            # ta_volume_relabel
        getters_refuse()
        _einval(ctx.mesh)                                           # ... and the extraction went with the volume
        ctx.extract(_capi.F_ALL, top + 100)
        assert_identical(context_meshes(ctx, 2), ref.mesh(lut[V], sub_factor=2))
        ctx.set_volume(np.ascontiguousarray(V[:, :, :32]))          # a new volume
        getters_refuse()
        _einval(ctx.mesh)
        ctx.extract(_capi.F_ALL, top)
        assert_identical(context_meshes(ctx), ref.mesh(V[:, :, :32]))
        ids = ctx.compact_labels()                                  # compaction: rows become ranks
        getters_refuse()
        _einval(ctx.mesh)
        ctx.extract(_capi.F_ALL, ids.size - 1)
        assert_identical(context_meshes(ctx, ids=ids), ref.mesh(V[:, :, :32]))
        ctx.uncompact()                                             # ... and its end
        getters_refuse()
        _einval(ctx.mesh)
        ctx.extract(_capi.F_ALL, top)
        assert_identical(context_meshes(ctx), ref.mesh(V[:, :, :32]))
        t = torch.from_numpy(V.view(np.int16).copy()).cuda()        # a slab adopted with a halo plane
        torch.cuda.synchronize()
        ctx.set_volume_device(t.data_ptr(), 2, t.shape, a0_origin=4, has_low_halo=True, keep=t)
        ctx.extract(_capi.F_ALL, top)
        _einval(ctx.mesh)
        getters_refuse()
        ctx.set_volume_device(t.data_ptr(), 2, t.shape, keep=t)     # the same planes without one
        ctx.extract(_capi.F_ALL, top)
        assert_identical(context_meshes(ctx), ref.mesh(V))
    finally:
        ctx.close()


def test_a_volume_changed_behind_the_extraction_is_an_error_not_a_fault():
    """A label above the rows of the extraction: the count kernels see it (they guard the read of the wanted table) and
    ta_mesh_extract answers TA_ERANGE; the context goes on working."""
    import torch
    V = synth.voronoi_labels((12, 20, 70), 30, 5, np.uint32)
    top = int(V.max())
    for patch in ((slice(3, 6), slice(4, 9), slice(10, 50)), (slice(11, 12), slice(19, 20), slice(69, 70))):
        t = torch.from_numpy(V.view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        ctx = _capi.Context(0)
        try:
            ctx.set_volume_device(t.data_ptr(), 4, t.shape, keep=t)
            ctx.extract(_capi.F_ALL, top)
            assert_identical(context_meshes(ctx), ref.mesh(V))
            t[patch] = top + 1 + 70000
            torch.cuda.synchronize()
            _code(_capi.TA_ERANGE, ctx.mesh)
            assert ctx._lib.ta_mesh_size(ctx._h, None, None, None) == _capi.TA_EINVAL          # no result is held
            wanted = np.zeros(top + 1, dtype=np.uint8)
            wanted[2] = 1
            _code(_capi.TA_ERANGE, ctx.mesh, 1, wanted)
            W = V.copy()
            W[patch] = top + 1 + 70000
            ctx.extract(_capi.F_ALL, int(W.max()))                  # a new extraction of the volume as it is now
            assert_identical(context_meshes(ctx), ref.mesh(W))
        finally:
            ctx.close()
