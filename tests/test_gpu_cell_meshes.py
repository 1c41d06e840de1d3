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
