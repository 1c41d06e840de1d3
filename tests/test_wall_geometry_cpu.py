"""The host side of the wall geometry (tissue_analysis_amd/wall_geometry.py) without a GPU: the tables come from the NumPy
restatement of tests/wall_geometry_reference.py and are injected into WallGeometry; the C ABI's symbols and its argument check."""
import os
import re

import numpy as np
import pytest

import wall_geometry_reference as ref
from tissue_analysis_amd import WallGeometry, _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def geometry(V, voxelsize=(1.0, 1.0, 1.0), **kw):
    r = ref.rows(V, **kw)
    return WallGeometry(r["lo"], r["hi"], r["fwd"], r["rev"], r["sum1"], r["sum2"], voxelsize)


def row_of(G, lo, hi):
    r = G.wall_rows([lo], [hi])
    assert r[0] >= 0
    return int(r[0])


# -- symbols
def declared_symbols():
    text = open(os.path.join(ROOT, "include", "tissue_scan_wallgeo.h")).read()
    return sorted(set(re.findall(r"TA_API\s+(?:const\s+char\s*\*|int)\s+(ta_\w+)\s*\(", text)))


def test_header_and_binding_agree():
    assert declared_symbols() == sorted(_capi.WALLGEO_SYMBOLS)
    assert not set(_capi.WALLGEO_SYMBOLS) & set(_capi.SYMBOLS)


def test_library_exports_the_symbols_and_rejects_a_null_context():
    lib = _capi.load()
    for name in declared_symbols():
        assert hasattr(lib, name), name
    assert lib.ta_wallgeo_extract(None) == _capi.TA_EINVAL
    assert b"NULL" in lib.ta_last_error()
    assert lib.ta_wallgeo_get(None, None, None, None, None) == _capi.TA_EINVAL
    assert lib.ta_wallgeo_debug(None, None) == _capi.TA_EINVAL
    assert b"NULL" in lib.ta_last_error()
    assert lib.ta_version() == 5


# -- a {111} wall: its staircase has 3 F faces for an area of sqrt(3) F
def test_a_111_wall():
    i, j, k = np.indices((24, 24, 24))
    V = np.where(i + j + k < 36, 2, 3).astype(np.uint16)
    G = geometry(V)
    assert len(G) == 1 and G.pair_lo[0] == 2 and G.pair_hi[0] == 3
    assert not G.rev.any()
    assert G.fwd[0, 0] == G.fwd[0, 1] == G.fwd[0, 2] > 0
    assert np.abs(G.normal()[0] - np.ones(3) / np.sqrt(3.0)).max() <= 1e-15
    assert abs(G.projected_area()[0] / G.voxel_area()[0] - 1.0 / np.sqrt(3.0)) <= 1e-15
    n, thickness, extents = G.plane_fit()
    assert np.abs(np.abs(n[0]) - 1.0 / np.sqrt(3.0)).max() <= 1e-6 and (n[0] > 0).all()
    assert thickness[0] < 0.6 and (extents[0] > 5.0).all()            # a staircase of half-steps about a plane of 24 voxels across


# -- a ball in a background, cut at a plane
def test_a_cut_ball_and_a_closed_wall():
    i, j, k = np.indices((32, 32, 32))
    ball = (i - 16) ** 2 + (j - 15) ** 2 + (k - 14) ** 2 <= 81
    V = np.ones((32, 32, 32), dtype=np.uint16)
    V[ball] = 2
    V[ball & (j >= 17)] = 3                                            # the cut: between j = 16 and j = 17
    G = geometry(V)
    r = row_of(G, 2, 3)
    assert np.array_equal(G.normal()[r], [0.0, 1.0, 0.0])              # +e_1 points from 2 to 3
    n, thickness, extents = G.plane_fit()
    assert np.abs(np.abs(n[r]) - [0.0, 1.0, 0.0]).max() <= 1e-12 and n[r, 1] > 0
    assert thickness[r] == 0.0 and (extents[r] > 1.0).all()
    assert G.projected_area()[r] == G.voxel_area()[r] > 0
    assert np.array_equal(G.centroid(real=False)[r, 1:2], [16.5])
    # the uncut ball: a closed wall
    U = np.ones((32, 32, 32), dtype=np.uint16)
    U[ball] = 2
    G = geometry(U)
    assert len(G) == 1
    assert not G.vector_area()[0].any() and G.projected_area()[0] == 0.0
    assert np.isnan(G.normal()[0]).all()
    assert np.abs(G.centroid(real=False)[0] - [16.0, 15.0, 14.0]).max() <= 1e-12
    assert G.voxel_area()[0] > 0


# -- closure: the outward signed face counts of an interior cell add up to zero
def test_closure_on_c1():
    c = synth.CONFIGS["C1"]
    V = synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], np.uint16)
    G = geometry(V)
    assert len(G) > 100
    signed = G.fwd.astype(np.int64) - G.rev.astype(np.int64)           # from lo to hi
    top = int(V.max())
    out = np.zeros((top + 1, 3), dtype=np.int64)
    np.add.at(out, G.pair_lo, signed)                                  # outward for lo
    np.add.at(out, G.pair_hi, -signed)                                 # outward for hi
    interior = 0
    for l in np.unique(V).tolist():
        w = np.argwhere(V == l)
        if (w.min(axis=0) > 0).all() and (w.max(axis=0) < np.array(V.shape) - 1).all():
            interior += 1
            assert not out[l].any(), l
    assert interior > 10


# -- moments of a flat wall against the closed form
def test_moments_of_a_flat_rectangle():
    V = np.ones((12, 20, 30), dtype=np.uint16)
    V[5:, 3:12, 4:25] = 7                      # its low face along axis 0: a 9 x 21 rectangle between planes 4 and 5
    V[6:] = 1
    G = geometry(V)
    # (1, 7) also has the top face and the sides: take the single plane of faces by cutting the volume under it
    G = geometry(V[:6])
    assert len(G) == 1
    faces = G.faces()[0]
    assert faces[0] == 9 * 21 and faces[1] == 2 * 21 and faces[2] == 2 * 9
    W = np.ones((6, 20, 30), dtype=np.uint16)
    W[5:, :, :] = 7                            # a whole plane: only axis-0 faces, a 20 x 30 rectangle
    G = geometry(W)
    cov = G.covariance(real=False)[0]
    want = np.diag([0.0, (20 ** 2 - 1) / 12.0, (30 ** 2 - 1) / 12.0])
    assert np.abs(cov - want).max() <= 1e-12
    assert np.array_equal(G.centroid(real=False)[0], [4.5, 9.5, 14.5])
    vs = (2.0, 0.5, 0.25)
    G = geometry(W, vs)
    assert np.abs(G.covariance()[0] - want * np.outer(vs, vs)).max() <= 1e-12
    n, thickness, extents = G.plane_fit()
    assert np.array_equal(np.abs(n[0]), [1.0, 0.0, 0.0]) and n[0, 0] > 0 and thickness[0] == 0.0
    assert np.abs(np.sort(extents[0]) - np.sort([np.sqrt(want[1, 1]) * 0.5, np.sqrt(want[2, 2]) * 0.25])).max() <= 1e-12


# -- host forms
def test_anisotropic_voxels_merge_and_dictionaries():
    V = synth.voronoi_labels((30, 24, 40), 25, 5, np.uint16)
    vs = (0.5, 0.25, 2.0)
    G = geometry(V, vs)
    assert len(G) > 20 and G.voxelsize == vs
    face = np.array([vs[1] * vs[2], vs[2] * vs[0], vs[0] * vs[1]])
    assert np.allclose(G.voxel_area(), (G.faces() * face).sum(axis=1), rtol=1e-15, atol=0)
    assert np.array_equal(G.voxel_area(real=False), G.n())
    assert np.array_equal(G.vector_area(), (G.fwd.astype(np.int64) - G.rev.astype(np.int64)) * face)
    assert (G.projected_area() <= G.voxel_area() * (1 + 1e-15)).all()
    assert np.allclose(G.centroid(), G.centroid(real=False) * np.array(vs), rtol=1e-15, atol=0)
    ok = ~np.isnan(G.normal()).any(axis=1)
    assert ok.sum() > 20 and np.abs(np.linalg.norm(G.normal()[ok], axis=1) - 1.0).max() <= 1e-15
    # covariance against the definition, wall by wall, from the restatement's own faces
    cov = G.covariance(real=False)
    c = G.sum1.astype(np.float64) / G.n()[:, None]
    for k, (x, y) in enumerate(ref.PAIRS):
        assert np.abs(cov[:, x, y] - (G.sum2[:, k] / G.n() - c[:, x] * c[:, y]) / 4.0).max() <= 1e-9
    # two slabs with a low halo merge to the whole
    cut = 13
    low = geometry(V[:cut], vs)
    high = geometry(V[cut - 1:], vs, first_owned=1, a0_origin=cut)
    M = WallGeometry.merge([low, high])
    for name in ("pair_lo", "pair_hi", "fwd", "rev", "sum1", "sum2"):
        assert np.array_equal(getattr(M, name), getattr(G, name)), name
    assert M.voxelsize == vs
    r = ref.merge([ref.rows(V[:cut]), ref.rows(V[cut - 1:], first_owned=1, a0_origin=cut)])
    assert np.array_equal(r["sum2"], G.sum2) and np.array_equal(r["fwd"], G.fwd)
    d = G.as_dict("projected_area")
    assert len(d) == len(G) and all(lo < hi for lo, hi in d)
    d = G.as_dict("normal", exclude=(1,))
    assert 0 < len(d) < len(G) and all(1 not in k for k in d) and all(np.shape(v) == (3,) for v in d.values())
    assert np.array_equal(G.wall_rows(G.pair_hi, G.pair_lo), np.arange(len(G)))
    assert G.wall_rows([70000], [70001])[0] == -1
    with pytest.raises(ValueError):
        WallGeometry([3], [2], np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 6)))
    empty = geometry(np.ones((3, 3, 3), dtype=np.uint16))
    assert len(empty) == 0 and empty.normal().shape == (0, 3) and empty.plane_fit()[2].shape == (0, 2) and empty.as_dict("n") == {}


# -- through the analysis class and the graph, with the sweep's tables from the CPU restatement and the geometry injected
def test_analysis_methods_and_graph_columns_from_injected_tables():
    from oracle import onepass
    from tissue_analysis_amd import DICT, SpatialImage, SpatialImageAnalysis3D, graph_from_image
    from tissue_analysis_amd.extraction import Extraction
    V = synth.voronoi_labels((30, 24, 40), 25, 5, np.uint16)
    vs = (0.5, 0.25, 2.0)
    sia = SpatialImageAnalysis3D(SpatialImage(V, voxelsize=vs), ignoredlabels=0, return_type=DICT, background=1,
                                 extraction=Extraction.from_arrays(V.shape, onepass.extract(V)))
    G = sia._wall_geometry = geometry(V, vs)
    assert np.array_equal(G.faces(), sia.extraction.as_arrays()["pair_faces"])
    areas, proj, normals = sia.wall_areas(), sia.wall_projected_areas(), sia.wall_normals()
    assert list(proj.keys()) == list(areas.keys()) == list(normals.keys()) and len(proj) > 20
    assert all(proj[k] <= areas[k] * (1 + 1e-12) for k in proj)
    k = next(iter(normals))
    r = row_of(G, k[0], k[1])
    assert np.array_equal(normals[k], G.normal()[r]) and proj[k] == G.projected_area()[r]
    assert sia.wall_projected_areas(real=False)[k] == G.projected_area(real=False)[r]
    assert list(sia.wall_normals({k[0]: [k[1]]}).keys()) == [k]
    plain = graph_from_image(sia, spatio_temporal_properties=['barycenter', 'wall_surface'], ignore_cells_at_stack_margins=False)
    g = graph_from_image(sia, spatio_temporal_properties=['barycenter', 'wall_surface', 'wall_normal', 'wall_centroid', 'wall_projected_area'],
                         ignore_cells_at_stack_margins=False)
    assert np.array_equal(g.edge_sources, plain.edge_sources) and np.array_equal(g.edge_targets, plain.edge_targets)
    assert sorted(g.edge_property_names()) == sorted(list(plain.edge_property_names()) + ['wall_normal', 'wall_centroid', 'wall_projected_area'])
    rows = G.wall_rows(g.edge_sources, g.edge_targets)
    assert (rows >= 0).all() and rows.size > 20
    assert np.array_equal(g.edge_column('wall_normal')[0], G.normal()[rows], equal_nan=True)
    assert np.array_equal(g.edge_column('wall_centroid')[0], G.centroid()[rows])
    assert np.array_equal(g.edge_column('wall_projected_area')[0], G.projected_area()[rows])
    assert all(g.edge_column(n)[1].all() for n in ('wall_normal', 'wall_centroid', 'wall_projected_area'))
    assert np.array_equal(g.edge_column('wall_surface')[0], plain.edge_column('wall_surface')[0])
    e = next(iter(g.edges()))
    assert len(g.edge_property('wall_normal')[e]) == 3
