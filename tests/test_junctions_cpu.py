"""Cell junctions without a GPU: the NumPy restatement of tests/junction_reference.py against closed forms, and the host logic of
CellJunctions on tables from that restatement."""
import itertools

import numpy as np
import pytest

import junction_reference as ref
from tissue_analysis_amd import CellJunctions, synth


def _junctions(V, voxelsize=(1.0, 1.0, 1.0), **kw):
    e, v, deg = ref.tables(V, **kw)
    return CellJunctions(e[0], e[1], e[2], v[0], v[1], v[2], deg, voxelsize)


def _octants(n, labels):
    V = np.zeros((n, n, n), dtype=np.uint16)
    h = n // 2
    for q, (i, j, k) in enumerate(itertools.product((0, 1), repeat=3)):
        V[i * h:(i + 1) * h, j * h:(j + 1) * h, k * h:(k + 1) * h] = labels[q]
    return V


# ---- the reference against closed forms ----------------------------------------------------------------------------------------

def test_three_cells_along_one_line():
    a, b, c = 3, 7, 9
    V = np.full((6, 8, 10), a, dtype=np.uint16)
    V[:, 4:, :5] = b
    V[:, 4:, 5:] = c
    (el, en, es), (vl, vn, vs), deg = ref.tables(V)
    # the line runs along axis 0 at (j, k) = (3.5, 4.5): five blocks, origins (i, 3, 4), centres 2 o + 1 = (2 i + 1, 7, 9)
    assert el.tolist() == [[a, b, c]] and en.tolist() == [5] and es.tolist() == [[25, 35, 45]]
    assert vl.shape == (0, 4) and vn.size == 0 and vs.shape == (0, 3) and deg == 0


def test_four_quadrant_columns_meet_in_one_vertex_row():
    n0 = 7
    V = np.zeros((n0, 6, 6), dtype=np.uint32)
    V[:, :3, :3], V[:, :3, 3:], V[:, 3:, :3], V[:, 3:, 3:] = 11, 12, 13, 70000
    (el, en, es), (vl, vn, vs), deg = ref.tables(V)
    assert el.shape == (0, 3) and deg == 0
    assert vl.tolist() == [[11, 12, 13, 70000]] and vn.tolist() == [n0 - 1]
    assert vs.tolist() == [[sum(2 * i + 1 for i in range(n0 - 1)), 5 * (n0 - 1), 5 * (n0 - 1)]]


def test_eight_octants():
    labels = [1, 2, 3, 4, 5, 6, 7, 8]
    (el, en, es), (vl, vn, vs), deg = ref.tables(_octants(2, labels))
    assert deg == 1 and el.shape == (0, 3) and vl.shape == (0, 4)
    V = _octants(6, labels)
    (el, en, es), (vl, vn, vs), deg = ref.tables(V)
    # the centre block sees all eight; along each of the six half-axes two blocks see the four octants around it
    assert deg == 1 and el.shape == (0, 3)
    assert vl.shape == (6, 4) and vn.tolist() == [2] * 6
    want = set()
    for axis in range(3):
        for side in (0, 1):
            quad = []
            for q, ijk in enumerate(itertools.product((0, 1), repeat=3)):
                if ijk[axis] == side:
                    quad.append(labels[q])
            want.add(tuple(sorted(quad)))
    assert set(map(tuple, vl.tolist())) == want
    row = vl.tolist().index([1, 2, 3, 4])                  # octants with i = 0: the half-axis 0, low side; origins (0, 2, 2), (1, 2, 2)
    assert vs[row].tolist() == [1 + 3, 5 + 5, 5 + 5]


def test_flat_axes_and_slab_cuts_of_the_reference():
    V = synth.voronoi_labels((1, 40, 30), 25, 2, dtype=np.uint16)
    e3, v3, d3 = ref.tables(V)
    e2, v2, d2 = ref.tables(V[0])                          # the 2-D image (40, 30) is the volume (40, 30, 1)
    assert e3[1].sum() > 0 and np.array_equal(e3[0], e2[0]) and np.array_equal(e3[1], e2[1])
    assert np.array_equal(e3[2][:, 1:], e2[2][:, :2]) and not e3[2][:, 0].any() and not e2[2][:, 2].any()
    assert d2 == 0                                         # four voxels hold at most four labels
    W = synth.voronoi_labels((20, 18, 22), 30, 4, dtype=np.uint16)
    whole = ref.tables(W)
    parts = [ref.tables(W[:8]), ref.tables(W[7:13], first_owned=1, a0_origin=8), ref.tables(W[12:], first_owned=1, a0_origin=13)]
    merged = ref.merge(parts)
    pairs = ref.tables_by_plane_pairs(W)
    for got in (merged, pairs, ref.tables_by_plane_pairs(W, planes=4)):
        for k in (0, 1):
            for x, y in zip(got[k], whole[k]):
                assert np.array_equal(x, y)
        assert got[2] == whole[2]
    assert whole[0][1].size > 50 and whole[1][1].size > 20


# ---- CellJunctions on tables from the reference ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tissue():
    V = synth.voronoi_labels((24, 28, 32), 40, 6, dtype=np.uint16)
    return V, _junctions(V, voxelsize=(0.5, 0.25, 2.0))


def test_positions_and_real_scaling(tissue):
    V, J = tissue
    assert J.edge_labels.dtype == np.int64 and J.edge_n.dtype == np.uint64 and J.edge_sum.dtype == np.uint64
    assert J.vertex_labels.shape[1] == 4 and J.vertex_labels.shape[0] > 10
    vox = J.vertex_positions(real=False)
    assert vox.dtype == np.float64 and np.array_equal(vox, J.vertex_sum / (2.0 * J.vertex_n[:, None].astype(np.float64)))
    assert np.allclose(J.vertex_positions(real=True), vox * np.array([0.5, 0.25, 2.0]), rtol=0, atol=1e-12)
    assert np.allclose(J.edge_centroids(), J.edge_centroids(real=False) * np.array([0.5, 0.25, 2.0]), rtol=0, atol=1e-12)
    assert (vox > 0).all() and (vox < np.array(V.shape) - 1).all()
    # a vertex of one block: the position is that block's centre, and the block holds exactly the row's labels
    i = int(np.flatnonzero(J.vertex_n == 1)[0])
    o = (vox[i] - 0.5).astype(int)
    assert np.array_equal(o + 0.5, vox[i])
    assert np.unique(V[o[0]:o[0] + 2, o[1]:o[1] + 2, o[2]:o[2] + 2]).tolist() == J.vertex_labels[i].tolist()


def test_exclude_and_lookups(tissue):
    V, J = tissue
    every = J.cell_vertices(real=False)
    assert len(every) == J.vertex_labels.shape[0]
    k0 = tuple(J.vertex_labels[0].tolist())
    assert np.array_equal(every[k0], J.vertex_positions(real=False)[0])
    gone = int(J.vertex_labels[0, 1])
    kept = J.cell_vertices(real=False, exclude=(gone,))
    assert set(kept) == set(k for k in every if gone not in k) and len(kept) < len(every)
    edges = J.wall_edges(exclude=(gone,))
    assert set(edges) == set(tuple(l) for l in J.edge_labels.tolist() if gone not in l)
    k = next(iter(edges))
    r = J.edge_labels.tolist().index(list(k))
    assert edges[k][0] == int(J.edge_n[r]) and np.array_equal(edges[k][1], J.edge_centroids(True)[r])
    a, b, c = J.edge_labels[3].tolist()
    assert 3 in J.edges_of_wall(a, b).tolist() and 3 in J.edges_of_wall(c, a).tolist()
    assert J.edges_of_wall(a, b).tolist() == [i for i, l in enumerate(J.edge_labels.tolist()) if a in l and b in l]
    assert J.edges_of_cell(a).tolist() == [i for i, l in enumerate(J.edge_labels.tolist()) if a in l]
    assert J.vertices_of_cell(gone).tolist() == [i for i, l in enumerate(J.vertex_labels.tolist()) if gone in l]
    assert J.edges_of_wall(a, a).size == 0 and J.edges_of_cell(10 ** 6).size == 0


def test_incidence_against_a_brute_force_set_test(tissue):
    _, J = tissue
    inc = J.incidence()
    assert inc.shape == (J.vertex_labels.shape[0], 4) and inc.dtype == np.int64
    rows = dict((tuple(l), i) for i, l in enumerate(J.edge_labels.tolist()))
    found = 0
    for v, quad in enumerate(J.vertex_labels.tolist()):
        for k in range(4):
            want = rows.get(tuple(quad[:k] + quad[k + 1:]), -1)
            assert inc[v, k] == want
            found += want >= 0
    assert found > 0 and (inc == -1).sum() + found == inc.size
    # ids beyond 2^31 and a table without edges
    big = CellJunctions([[5, 2 ** 31 + 1, 2 ** 32 - 1]], [2], [[4, 4, 4]], [[5, 7, 2 ** 31 + 1, 2 ** 32 - 1], [1, 2, 3, 4]], [1, 1],
                        [[1, 1, 1], [3, 3, 3]])
    assert big.incidence().tolist() == [[-1, 0, -1, -1], [-1, -1, -1, -1]]
    none = CellJunctions(np.zeros((0, 3)), [], np.zeros((0, 3)), [[1, 2, 3, 4]], [1], [[1, 1, 1]])
    assert none.incidence().tolist() == [[-1, -1, -1, -1]]


def test_merge_of_two_cuts_equals_the_whole(tissue):
    V, J = tissue
    for cut in (9, 17):
        lowp = _junctions(V[:cut], J.voxelsize)
        high = _junctions(V[cut - 1:], J.voxelsize, first_owned=1, a0_origin=cut)
        M = CellJunctions.merge([lowp, high])
        for name in ("edge_labels", "edge_n", "edge_sum", "vertex_labels", "vertex_n", "vertex_sum"):
            assert np.array_equal(getattr(M, name), getattr(J, name)), name
        assert M.degenerate == J.degenerate and M.voxelsize == J.voxelsize
    with pytest.raises(ValueError):
        CellJunctions.merge([])


def test_shape_validation_and_empty_tables():
    E = CellJunctions([], [], [], [], [], [])
    assert E.edge_labels.shape == (0, 3) and E.vertex_labels.shape == (0, 4) and E.edge_sum.shape == (0, 3)
    assert E.vertex_positions().shape == (0, 3) and E.cell_vertices() == {} and E.wall_edges() == {} and E.incidence().shape == (0, 4)
    assert CellJunctions([], [], [], [], [], [], voxelsize=(2.0, 3.0)).voxelsize == (2.0, 3.0, 1.0)
    with pytest.raises(ValueError):
        CellJunctions([[1, 2]], [1], [[1, 1, 1]], [], [], [])                  # two labels in an edge row
    with pytest.raises(ValueError):
        CellJunctions([[1, 2, 3]], [1, 1], [[1, 1, 1]], [], [], [])            # n of another length
    with pytest.raises(ValueError):
        CellJunctions([], [], [], [[1, 2, 3, 4]], [1], [[1, 1]])               # sums of two columns
    with pytest.raises(ValueError):
        CellJunctions([[1, 2, -3]], [1], [[1, 1, 1]], [], [], [])
    with pytest.raises(ValueError):
        CellJunctions([], [], [], [], [], [], voxelsize=(1.0,))
