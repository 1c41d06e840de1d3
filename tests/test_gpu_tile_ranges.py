"""The signal, overlap and wall-geometry passes on the MI355X where a workgroup takes MORE THAN ONE tile (csrc/kernels_signal.hip,
kernels_overlap.hip, kernels_wallgeo.hip), against tests/signal_reference.py, overlap_reference.py and
wall_geometry_reference.py: every number is an integer and must be bit-exact.

tiles_per_group = ceil(tiles / MAX_GROUPS), so a range of several tiles needs more than 1024 tiles (wall geometry: 4096).  The
shapes of tests/range_tiles.py get there with thin volumes -- few columns, many row and plane blocks -- of 1.6 to 4.5 million
voxels: 2 tiles a group with a clipped last group, 2 tiles that are the two column blocks of one row block, and 5 tiles (wall
geometry: 2).  Every case asserts the plan the device reports (ta_signal_debug, ta_overlap_debug, ta_wallgeo_debug) against the
restatement, so that a retuned group count cannot turn these into one-tile tests unnoticed; test_range_tiles_cpu.py states what
each shape is for (partial tiles and the row skip inside a range, ranges that straddle plane blocks, both load paths).

The labels are a coarse random grid repeated in blocks of 5 x 7 x 3 voxels: label runs cross tiles, column blocks and ranges,
a lane's running record is carried from tile to tile, and a group's LDS tables hold several tiles' labels."""
import functools

import numpy as np
import pytest

import range_tiles as rt
from feature_passes import Pass
from tissue_analysis_amd import _capi

pytestmark = pytest.mark.gpu

# signal and B types by case: every (label, signal) and (label, B) combination on the vector-load and on the scalar-load path
SIGNAL_DTYPE = {"a_u16": np.uint8, "a_u32": np.uint16, "a_u16_scalar": np.uint8, "b_u32": np.uint8, "b_u32_scalar": np.uint16,
                "c_u16": np.uint16, "c_u32": np.uint8, "c_u16_vector": np.uint8, "c_u32_vector": np.uint16, "a_u16_halo": np.uint16,
                "c_u32_halo": np.uint8}
B_DTYPE = {"a_u16": np.uint16, "a_u32": np.uint32, "a_u16_scalar": np.uint32, "b_u32": np.uint16, "b_u32_scalar": np.uint32,
           "c_u16": np.uint16, "c_u32": np.uint16, "c_u16_vector": np.uint32, "c_u32_vector": np.uint32, "a_u16_halo": np.uint32,
           "c_u32_halo": np.uint16}
NAMES = [c.name for c in rt.CASES]
DEGENERATE = rt.CASE["c_u16"]          # 5 tiles a group (wall geometry: 2)


@functools.lru_cache(maxsize=None)
def labels_of(name):
    c = rt.CASE[name]
    v = rt.block_labels(c.dims, c.dtype, 11)
    v.setflags(write=False)
    return v


def test_the_type_tables_cover_every_combination_on_both_load_paths():
    for table, kinds in ((SIGNAL_DTYPE, (np.uint8, np.uint16)), (B_DTYPE, (np.uint16, np.uint32))):
        assert sorted(table) == sorted(NAMES)
        seen = set((c.dtype.itemsize, np.dtype(table[c.name]).itemsize, rt.vector_path(c.dims, c.dtype.itemsize)) for c in rt.CASES)
        assert seen == set((l, np.dtype(k).itemsize, v) for l in (2, 4) for k in kinds for v in (False, True))


@pytest.mark.parametrize("name", NAMES)
def test_signal(name):
    c, V = rt.CASE[name], labels_of(name)
    S = rt.random_image(c.dims, SIGNAL_DTYPE[name], 12)
    with Pass(V, c.first_owned) as p:
        assert p.plan("signal").per > 1
        p.extract()
        p.set_signal(S)
        p.check_signal(S)


@pytest.mark.parametrize("name", NAMES)
def test_overlap(name):
    c, V = rt.CASE[name], labels_of(name)
    B = rt.block_labels(c.dims, B_DTYPE[name], 13, nlabels=200, block=(3, 5, 7))
    with Pass(V, c.first_owned) as p:
        assert p.plan("overlap").per > 1
        p.set_overlap(B)
        p.check_overlap(B)


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("c_")] + ["a_u16", "b_u32_scalar", "a_u16_halo"])
def test_wall_geometry(name):
    c, V = rt.CASE[name], labels_of(name)
    with Pass(V, c.first_owned) as p:
        assert p.plan("wallgeo").per == (2 if name.startswith("c_") else 1)
        p.extract()
        _, want = p.check_wallgeo()
        assert want["lo"].size > 20000 and want["rev"].any() and want["sum2"].any()


# ---- degenerate contents at one multi-tile shape ----------------------------------------------------------------------------------
def test_one_label_with_the_largest_signal_everywhere():
    """A lane's record and the group's one LDS row hold a whole range of 5 tiles: n, sum and sumsq of the groups add up."""
    c = DEGENERATE
    V = np.full(c.dims, 3, dtype=c.dtype)
    S = np.full(c.dims, 65535, dtype=np.uint16)
    with Pass(V) as p:
        p.extract()
        assert p.ctx.adjacency_size() == 0
        p.set_signal(S)
        d = p.check_signal(S)
        assert d == dict(label_spills=0, pair_spills=0, tiles_per_group=5, groups=874)
        n, s, q, mn, mx = p.ctx.signal_labels()
        assert int(n[3]) == V.size and int(s[3]) == V.size * 65535 and int(q[3, 0]) == V.size * 65535 ** 2 < 2 ** 64
        assert (int(mn[3]), int(mx[3])) == (65535, 65535) and not n[:3].any()
        p.set_overlap(V)
        assert p.check_overlap(V)["spills"] == 0
        assert [x.tolist() for x in p.ctx.overlap_get()] == [[3], [3], [V.size]]
        d, want = p.check_wallgeo()                                  # no pair: nothing is launched, and nothing fails
        assert want["lo"].size == 0


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_two_half_spaces(axis, swap):
    """Exactly one pair, whose faces all lie in one plane and on one side: every group that meets the plane adds to the same row."""
    c = DEGENERATE
    V = rt.half_space(c.dims, c.dtype, axis, swap=swap)
    S = rt.random_image(c.dims, np.uint16, 14)
    with Pass(V) as p:
        p.extract()
        assert p.ctx.adjacency_size() == 1
        p.set_signal(S)
        assert p.check_signal(S)["pair_spills"] == 0
        d, want = p.check_wallgeo()
        assert d["spills"] == 0 and want["lo"].tolist() == [2] and want["hi"].tolist() == [5]
        side, other = (want["rev"], want["fwd"]) if swap else (want["fwd"], want["rev"])
        assert not other.any() and side[0].tolist() == [V.size // c.dims[axis] if a == axis else 0 for a in range(3)]


def test_a_volume_against_itself_is_the_diagonal():
    c, V = DEGENERATE, labels_of(DEGENERATE.name)
    with Pass(V) as p:
        p.set_overlap(V)
        p.check_overlap(V)
        a, b, n = p.ctx.overlap_get()
        ids, counts = np.unique(V, return_counts=True)
        assert np.array_equal(a, ids) and np.array_equal(b, ids) and np.array_equal(n, counts.astype(np.uint64))
