"""The LDS tables of the signal, overlap and wall-geometry passes when they are full, and the guards of the feature passes against
a volume that changed after ta_extract (csrc/kernels_signal.hip, kernels_overlap.hip, kernels_wallgeo.hip, kernels_distance.hip).

Spills.  A record that finds no slot in a workgroup's LDS table within 32 probes goes to the global rows directly.  In a volume
that is a permutation of 0 .. nvox - 1 every voxel is its own label and every face its own pair: at (16, 4, 64) uint16, exactly
one tile and one workgroup, that is 4096 labels, 10944 wall pairs and 4096 overlap pairs against any B for tables of 512, 2048 (or
512) and 2048 slots.  By pigeonhole, whatever the hash does, at least (distinct keys of a workgroup - slots) records spill: the
bounds come from tests/range_tiles.py, that is from the volume alone, and every case asserts the spill counter of the device
against them (ta_signal_debug, ta_overlap_debug, ta_wallgeo_debug) and bit-exact results.

Stale volumes.  The passes index their rows by the labels and pairs of the last ta_extract.  A caller who edits an adopted device
buffer afterwards must get TA_ERANGE from the getters, never a write outside the rows, and the context must go on working."""
import functools

import numpy as np
import pytest

import distance_reference
import range_tiles as rt
import signal_reference
from feature_passes import Pass, code, poke
from tissue_analysis_amd import _capi

pytestmark = pytest.mark.gpu

LABELS, WALLS = _capi.SIG_LABELS, _capi.SIG_WALLS


@functools.lru_cache(maxsize=None)
def permutation(dims, dtype):
    v = rt.permutation_labels(dims, dtype, 21)
    v.setflags(write=False)
    return v


SMALL = (rt.SPILL_DIMS, np.uint16)
WIDE = (rt.SPILL_DIMS_WIDE, np.uint32)


# ---- spills ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", [LABELS | WALLS, LABELS, WALLS])
@pytest.mark.parametrize("sdtype", [np.uint8, np.uint16])
def test_signal_one_workgroup(sdtype, what):
    """The three instantiations of the kernel: both tables, the label table alone (no pair table in LDS), the pair table alone."""
    V = permutation(*SMALL)
    S = rt.random_image(V.shape, sdtype, 22)
    with Pass(V) as p:
        p.extract()
        assert p.ctx.adjacency_size() == 10944
        p.set_signal(S)
        d = p.check_signal(S, what)
        assert (d["tiles_per_group"], d["groups"]) == (1, 1)
        if what & LABELS:
            assert d["label_spills"] >= rt.label_spill_bound(V, 0) == 4096 - 512
        if what & WALLS:
            assert d["pair_spills"] >= rt.wall_spill_bound(V, 0, "signal") == 10944 - 2048


@pytest.mark.parametrize("bdtype", [np.uint16, np.uint32])
def test_overlap_one_workgroup(bdtype):
    V = permutation(*SMALL)
    B = rt.block_labels(V.shape, bdtype, 23)
    with Pass(V) as p:
        p.set_overlap(B)
        d = p.check_overlap(B)
        assert d["passes"] == 1 and p.ctx.overlap_size() == 4096
        assert d["spills"] >= rt.overlap_spill_bound(V, B, 0) == 4096 - 2048


def test_overlap_spills_into_a_device_table_that_overflows_and_regrows():
    V = permutation(*SMALL)
    B = np.zeros(V.shape, dtype=np.uint16)
    with Pass(V) as p:
        p.ctx.set_overlap_capacity(4)                  # 16 slots for 4096 pairs: the LDS spills and the flush meet a full table
        p.set_overlap(B)
        d = p.check_overlap(B)
        assert d["passes"] > 1
        assert d["spills"] >= 4096 - 2048              # of the LAST run, whose table was large enough
        p.ctx.set_overlap_capacity(0)
        assert p.check_overlap(B)["passes"] == 1


def test_wall_geometry_one_workgroup():
    V = permutation(*SMALL)
    with Pass(V) as p:
        p.extract()
        d, want = p.check_wallgeo()
        assert want["lo"].size == 10944
        assert d["spills"] >= rt.wall_spill_bound(V, 0, "wallgeo") == 10944 - 512


def test_several_workgroups_partial_tiles_and_the_scalar_path():
    V = permutation(*WIDE)
    S = rt.random_image(V.shape, np.uint16, 24)
    B = rt.block_labels(V.shape, np.uint32, 25)
    assert V.size == 20790 and not rt.vector_path(V.shape, 4)
    with Pass(V) as p:
        p.extract()
        assert p.ctx.adjacency_size() == 59133
        p.set_signal(S)
        d = p.check_signal(S)
        assert d["groups"] == 9
        assert d["label_spills"] >= rt.label_spill_bound(V, 0) > 10000
        assert d["pair_spills"] >= rt.wall_spill_bound(V, 0, "signal") > 40000
        p.set_overlap(B)
        assert p.check_overlap(B)["spills"] >= rt.overlap_spill_bound(V, B, 0) > 5000
        d, _ = p.check_wallgeo()
        assert d["spills"] >= rt.wall_spill_bound(V, 0, "wallgeo") > 50000


def test_spills_inside_ranges_of_several_tiles():
    """Spill and range meet: a box of noise in the volume with 5 tiles a group (wall geometry: 2).  The box spans two plane blocks and
    16 row blocks, so the groups that walk it also walk quiet tiles before and after, with their tables already full."""
    c = rt.CASE["c_u16"]
    V = rt.noise_box(rt.block_labels(c.dims, c.dtype, 11), (slice(16, 48), slice(200, 262), slice(None)), 26, 60000)
    S = rt.random_image(c.dims, np.uint8, 27)
    B = rt.block_labels(c.dims, np.uint16, 13, nlabels=200, block=(3, 5, 7))
    with Pass(V) as p:
        p.extract()
        p.set_signal(S)
        d = p.check_signal(S)
        assert d["tiles_per_group"] == 5
        assert d["label_spills"] >= rt.label_spill_bound(V, 0) > 5000
        assert d["pair_spills"] >= rt.wall_spill_bound(V, 0, "signal") > 5000
        p.set_overlap(B)
        assert p.check_overlap(B)["spills"] >= rt.overlap_spill_bound(V, B, 0) > 1000
        d, _ = p.check_wallgeo()
        assert d["tiles_per_group"] == 2
        assert d["spills"] >= rt.wall_spill_bound(V, 0, "wallgeo") > 5000


# ---- a volume edited after ta_extract ---------------------------------------------------------------------------------------------
def _quiet_volume(dtype=np.uint16):
    return rt.block_labels((24, 20, 70), dtype, 31, nlabels=40)


def _a_pair_that_is_not_adjacent(V):
    """(index of a voxel deep inside a block, a label that is no neighbour of that voxel's label): from the reference's pair list."""
    w = signal_reference.walls(V, np.zeros(V.shape, np.uint8))
    pairs = set(w["keys"].tolist())
    at = (7, 10, 34)                                    # the middle of the block (5 .. 9, 7 .. 13, 33 .. 35)
    a = int(V[at])
    assert all(int(V[at[0] + d[0], at[1] + d[1], at[2] + d[2]]) == a
               for d in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)))
    for b in np.unique(V).tolist():
        if b != a and ((min(a, b) << 32) | max(a, b)) not in pairs:
            return at, a, b
    raise AssertionError("every label touches label %d" % a)


def test_signal_meets_a_label_above_max_label():
    V = _quiet_volume()
    S = rt.random_image(V.shape, np.uint16, 32)
    with Pass(V, adopted=True) as p:
        p.extract()
        p.set_signal(S)
        p.check_signal(S)
        poke(p.t, (3, 4, 5), p.max_label + 1)
        p.ctx.signal_extract()
        for get in (p.ctx.signal_labels, p.ctx.signal_walls, p.ctx.signal_debug):
            assert code(get) == _capi.TA_ERANGE
        poke(p.t, (3, 4, 5), V[3, 4, 5])
        assert code(p.ctx.signal_labels) == _capi.TA_ERANGE            # the results of that pass stay what they are
        p.extract()
        p.check_signal(S)


def test_signal_meets_a_pair_the_extraction_does_not_hold():
    V = _quiet_volume(np.uint32)
    S = rt.random_image(V.shape, np.uint8, 33)
    at, a, b = _a_pair_that_is_not_adjacent(V)
    with Pass(V, adopted=True) as p:
        p.extract()
        p.set_signal(S)
        poke(p.t, at, b)
        p.ctx.signal_extract()
        assert code(p.ctx.signal_walls) == _capi.TA_ERANGE
        assert code(p.ctx.signal_debug) == _capi.TA_ERANGE
        p.ctx.signal_extract(WALLS)                                    # the kernel without the label table
        assert code(p.ctx.signal_walls) == _capi.TA_ERANGE
        poke(p.t, at, a)
        p.extract()
        p.check_signal(S)


def test_signal_walls_when_the_extraction_has_no_pair_at_all():
    """No pair, no pair index: the face of a stale volume must raise the flag, not read the index."""
    V = np.full((24, 20, 70), 1, dtype=np.uint16)
    S = rt.random_image(V.shape, np.uint16, 34)
    with Pass(V, adopted=True) as p:
        p.extract(max_label=2)
        assert p.ctx.adjacency_size() == 0
        p.set_signal(S)
        poke(p.t, (7, 10, 34), 2)
        p.ctx.signal_extract(WALLS)
        assert code(p.ctx.signal_walls) == _capi.TA_ERANGE
        assert code(p.ctx.signal_debug) == _capi.TA_ERANGE
        p.ctx.signal_extract(LABELS | WALLS)
        assert code(p.ctx.signal_walls) == _capi.TA_ERANGE
        poke(p.t, (7, 10, 34), 1)
        p.extract(max_label=2)
        p.check_signal(S, WALLS)
        assert [x.size for x in p.ctx.signal_walls()] == [0, 0]
        p.check_signal(S)


def test_wall_geometry_meets_a_pair_the_extraction_does_not_hold():
    V = _quiet_volume()
    at, a, b = _a_pair_that_is_not_adjacent(V)
    with Pass(V, adopted=True) as p:
        p.extract()
        poke(p.t, at, b)
        p.ctx.wallgeo_extract()
        for get in (p.ctx.wallgeo_get, p.ctx.wallgeo_spills, p.ctx.wallgeo_debug):
            assert code(get) == _capi.TA_ERANGE
        poke(p.t, at, a)
        p.extract()
        p.check_wallgeo()


def test_wall_geometry_when_the_extraction_has_no_pair_at_all():
    """Pinned, not praised: without a pair there is no row and the pass is not launched, so a stale volume goes unnoticed here
    (include/tissue_scan_wallgeo.h says so)."""
    V = np.full((24, 20, 70), 1, dtype=np.uint16)
    with Pass(V, adopted=True) as p:
        p.extract(max_label=2)
        poke(p.t, (7, 10, 34), 2)
        p.ctx.wallgeo_extract()
        assert [x.shape for x in p.ctx.wallgeo_get()] == [(0, 3), (0, 3), (0, 3), (0, 6)]
        assert p.ctx.wallgeo_debug() == dict(spills=0, tiles_per_group=0, groups=0)
        W = V.copy()
        W[7, 10, 34] = 2
        p.extract(max_label=2)                                         # the sweep sees the voxel: six faces of one pair
        _, want = p.check_wallgeo(V=W)
        assert int(want["fwd"].sum() + want["rev"].sum()) == 6


def test_distance_meets_a_label_above_max_label():
    V = _quiet_volume()
    with Pass(V, adopted=True) as p:
        p.extract()
        poke(p.t, (3, 4, 5), p.max_label + 1)
        p.ctx.distance_extract()
        assert code(p.ctx.distance_get) == _capi.TA_ERANGE
        poke(p.t, (3, 4, 5), V[3, 4, 5])
        p.extract()
        p.ctx.distance_extract()
        d2 = distance_reference.scipy_d2(V)
        want = distance_reference.table(V, d2, p.max_label + 1)
        for got, w in zip(p.ctx.distance_get(), want):
            assert np.array_equal(got, w)
        assert np.array_equal(p.ctx.distance_image().reshape(V.shape), d2)
