"""The references of the distance maps against each other, and the host side of the feature (DistanceMap, the analysis methods with
an injected table): no GPU."""
import functools

import numpy as np
import pytest

import distance_reference as ref
from oracle import onepass
from tissue_analysis_amd import DICT, NPLIST, DistanceMap, Extraction, SpatialImage, SpatialImageAnalysis3D
from tissue_analysis_amd.distance_map import FROM_LABEL, OWN_WALL

DYADIC = [(1.0, 1.0, 1.0), (0.5, 0.5, 1.0), (2.0, 0.25, 1.0)]
OTHER = (0.2, 0.3, 0.7)


@functools.lru_cache(maxsize=None)
def small_volumes():
    rng = np.random.default_rng(11)
    blocks = np.repeat(np.repeat(np.repeat(rng.integers(0, 4, (3, 3, 4)), 3, 0), 2, 1), 5, 2)      # (9, 6, 20)
    out = {
        "noise": rng.integers(0, 3, (6, 7, 9)),
        "blocks": blocks,
        "plane": rng.integers(0, 3, (1, 9, 40)),
        "thin": rng.integers(0, 2, (5, 1, 64)),
        "row": np.repeat(rng.integers(0, 3, 11), 7)[None, None, :],                                  # (1, 1, 77)
        "voxel": np.zeros((1, 1, 1), dtype=np.int64),
        "uniform": np.full((3, 3, 20), 2),
    }
    for v in out.values():
        v.setflags(write=False)
    return out


def close(a, b, rel=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(invalid="ignore"):
        return bool(np.all((a == b) | (np.abs(a - b) <= rel * np.abs(b))))


CASES = [(name, mode, edge) for name in ("noise", "blocks", "plane", "thin", "row", "voxel", "uniform")
         for mode in (OWN_WALL, FROM_LABEL) for edge in (False, True)]


@pytest.mark.parametrize("name,mode,edge", CASES)
def test_references_agree(name, mode, edge):
    V = small_volumes()[name]
    for spacing in DYADIC:
        a, b = ref.brute_d2(V, spacing, mode, 0, edge), ref.scipy_d2(V, spacing, mode, 0, edge)
        assert a.shape == V.shape and np.array_equal(a, b), spacing
    assert close(ref.brute_d2(V, OTHER, mode, 0, edge), ref.scipy_d2(V, OTHER, mode, 0, edge))


def test_reference_known_values():
    V = np.zeros((1, 1, 7), dtype=np.int64)
    V[0, 0, 3:] = 5
    assert ref.brute_d2(V, (1, 1, 0.5))[0, 0].tolist() == [2.25, 1.0, 0.25, 0.25, 1.0, 2.25, 4.0]
    assert ref.brute_d2(V, (1, 1, 1), FROM_LABEL, 5)[0, 0].tolist() == [9, 4, 1, 0, 0, 0, 0]
    assert ref.brute_d2(V, (1, 1, 1), edge=True)[0, 0].tolist() == [1, 1, 1, 1, 1, 1, 1]          # the margin along the other axes
    assert np.isinf(ref.brute_d2(np.full((2, 2, 2), 3))).all()
    assert np.isinf(ref.scipy_d2(V, (1, 1, 1), FROM_LABEL, 9)).all()                                # an absent site label


@pytest.mark.parametrize("mode", [OWN_WALL, FROM_LABEL])
def test_edge_is_the_padded_image(mode):
    """EDGE_IS_SITE equals the transform, without the flag, of the image padded by one voxel of a label it does not hold (mode 1: of
    the site label)."""
    V = small_volumes()["blocks"]
    for spacing in DYADIC:
        padded = np.pad(V, 1, mode="constant", constant_values=99 if mode == OWN_WALL else 0)
        want = ref.scipy_d2(padded, spacing, mode, 0, False)[1:-1, 1:-1, 1:-1]
        assert np.array_equal(ref.scipy_d2(V, spacing, mode, 0, True), want)
        assert np.array_equal(ref.brute_d2(V, spacing, mode, 0, True), want)


def test_table_reductions():
    V = np.array([[[1, 1, 1, 1, 1, 3, 3]]])
    d2 = ref.brute_d2(V, (1, 1, 1), edge=True)
    min2, max2, pole = ref.table(V, d2, 5)
    assert min2.tolist() == [np.inf, 1, np.inf, 1, np.inf] and max2.tolist() == [np.inf, 1, np.inf, 1, np.inf]
    assert pole.tolist() == [[-1] * 3, [0, 0, 0], [-1] * 3, [0, 0, 5], [-1] * 3]
    ids, min2, max2, pole = ref.table_by_id(V * 1000003, d2)
    assert ids.tolist() == [1000003, 3000009] and pole.tolist() == [[0, 0, 0], [0, 0, 5]]
    # a pole tie: the first in C order of the array axes, for every memory layout
    B = np.zeros((5, 6, 6), dtype=np.int64)
    B[1:4, 1:5, 1:5] = 7
    for layout in (B, np.asfortranarray(B), np.ascontiguousarray(B.transpose(1, 2, 0)).transpose(2, 0, 1)):
        assert ref.table(layout, ref.scipy_d2(layout), 8)[2][7].tolist() == [2, 2, 2]


# ---- DistanceMap on host arrays ---------------------------------------------------------------------------------------------
def host_map(**kw):
    inf = np.inf
    return DistanceMap([0, 1, 2, 5], [inf, 0.25, 1.0, inf], [inf, 9.0, 6.25, inf], [[-1, -1, -1], [4, 5, 6], [1, 0, 2], [-1, -1, -1]],
                       voxelsize=(0.5, 0.25, 2.0), **kw)


def test_distance_map_lookups():
    dm = host_map()
    assert len(dm) == 4 and dm.present.tolist() == [False, True, True, False] and dm.mode == OWN_WALL and dm.ms is None
    assert dm.radius() == {1: 3.0, 2: 2.5} and dm.max_distance() == dm.radius()
    assert dm.min_distance() == {1: 0.5, 2: 1.0}
    assert dm.radius(exclude=(1,)) == {2: 2.5} and dm.radius(labels=[2, 5, 77]) == {2: 2.5}
    assert dm.of_labels([1, 5, 0, 77, 2], "min2").tolist() == [0.5, np.inf, np.inf, np.inf, 1.0]
    real, voxels = dm.pole(), dm.pole(real=False, exclude=(2,))
    assert sorted(real) == [1, 2] and real[1].tolist() == [2.0, 1.25, 12.0] and real[2].tolist() == [0.5, 0.0, 4.0]
    assert list(voxels) == [1] and voxels[1].tolist() == [4.0, 5.0, 6.0]
    assert dm.rows_of([5, 3, 0]).tolist() == [3, -1, 0]
    with pytest.raises(ValueError):
        dm.image()
    with pytest.raises(ValueError):
        dm.of_labels([1], "mean")
    empty = DistanceMap([], [], [], [])
    assert len(empty) == 0 and empty.radius() == {} and empty.of_labels([3]).tolist() == [np.inf]
    two = DistanceMap([4], [1.0], [4.0], [[1, 2, 0]], voxelsize=(0.5, 0.25), mode=FROM_LABEL, site_label=1)
    assert two.voxelsize == (0.5, 0.25, 1.0) and two.pole()[4].tolist() == [0.5, 0.5, 0.0] and two.site_label == 1


def test_distance_map_shape_errors():
    with pytest.raises(ValueError):
        DistanceMap([1, 2], [1.0], [1.0, 2.0], [[0, 0, 0], [1, 1, 1]])
    with pytest.raises(ValueError):
        DistanceMap([1, 2], [1.0, 1.0], [1.0, 2.0], [[0, 0], [1, 1]])
    with pytest.raises(ValueError):
        DistanceMap([2, 1], [1.0, 1.0], [1.0, 2.0], [[0, 0, 0], [1, 1, 1]])
    with pytest.raises(ValueError):
        DistanceMap([1], [1.0], [1.0], [[0, 0, 0]], voxelsize=(1.0,))
    with pytest.raises(ValueError):
        DistanceMap([1], [1.0], [1.0], [[0, 0, 0]], mode=2)


# ---- the analysis methods, with the table injected -----------------------------------------------------------------------------
def analysis_with_tables(return_type):
    rng = np.random.default_rng(3)
    V = np.repeat(np.repeat(rng.integers(1, 5, (3, 3, 3)), 3, 0), 3, 1).astype(np.uint16)          # (9, 9, 3), labels 1 .. 4
    vs = (0.5, 0.5, 1.0)
    sia = SpatialImageAnalysis3D(SpatialImage(V, voxelsize=vs), return_type=return_type, background=1,
                                 extraction=Extraction.from_arrays(V.shape, onepass.extract(V)))
    for real in (True, False):
        spacing = vs if real else (1.0, 1.0, 1.0)
        wall = ref.scipy_d2(V, spacing)
        depth = ref.scipy_d2(V, spacing, FROM_LABEL, 1)
        sia._distance_cache[(OWN_WALL, None, False, real)] = DistanceMap(np.arange(5), *ref.table(V, wall, 5), voxelsize=spacing)
        sia._distance_cache[(FROM_LABEL, 1, False, real)] = DistanceMap(np.arange(5), *ref.table(V, depth, 5), voxelsize=spacing,
                                                                        mode=FROM_LABEL, site_label=1)
    return sia, V, vs


def test_inscribed_radius_and_depth_through_convert_return():
    sia, V, vs = analysis_with_tables(DICT)
    labels = sia.labels()
    assert 1 not in labels and set(labels) <= {2, 3, 4}
    for real in (True, False):
        spacing = vs if real else (1.0, 1.0, 1.0)
        wall, depth = ref.scipy_d2(V, spacing), ref.scipy_d2(V, spacing, FROM_LABEL, 1)
        radius = sia.inscribed_radius(real=real)
        assert radius == dict((l, float(np.sqrt(wall[V == l].max()))) for l in labels)
        assert sia.cell_depth(real=real) == dict((l, float(np.sqrt(depth[V == l].min()))) for l in labels)
        assert sia.inscribed_radius(labels[0], real=real) == {labels[0]: radius[labels[0]]}          # (as volume(label) answers)
    assert sia.wall_distance() is sia.wall_distance(edge_is_wall=False, real=True)
    assert sia.distance_from().site_label == 1 and sia.distance_from(1) is sia.distance_from()
    arrays, _, _ = analysis_with_tables(NPLIST)
    assert arrays.cell_depth().tolist() == [sia.cell_depth()[l] for l in labels]
    sia._forget()
    assert sia._distance_cache == {}


def test_distance_from_needs_a_label():
    V = np.ones((2, 2, 2), dtype=np.uint16)
    with pytest.warns(UserWarning):
        sia = SpatialImageAnalysis3D(V, extraction=Extraction.from_arrays(V.shape, onepass.extract(V)))
    with pytest.raises(ValueError):
        sia.distance_from()


def test_slab_jobs_name_the_pass():
    from tissue_analysis_amd.distributed import PipelinedSlabJob, SlabJob
    for cls in (SlabJob, PipelinedSlabJob):
        with pytest.raises(NotImplementedError, match="distance"):
            cls.distance_map(object.__new__(cls))
