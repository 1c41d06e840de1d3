"""range_tiles.py does what it claims, with no GPU: the restated launch plan gives the recorded numbers, every shape of
test_gpu_tile_ranges.py and test_gpu_feature_table_spills.py has the property it is used for, and the restated constants are
the ones the kernels are compiled with today."""
import os
import re

import numpy as np
import pytest

import overlap_reference
import range_tiles as rt
import signal_reference
import wall_geometry_reference

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tissue_analysis_amd", "csrc")


def _constant(source, name):
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*\d+\s*,\s*)*%s\s*=\s*(\d+)" % name, open(os.path.join(CSRC, source)).read())
    assert m, name
    return int(m.group(1))


def test_restated_constants_are_the_sources():
    """A retuned tile, table or group count must change range_tiles.py (and the shapes below) deliberately."""
    for which, src, pre in (("signal", "kernels_signal.hip", "SIG"), ("overlap", "kernels_overlap.hip", "OV"),
                            ("wallgeo", "kernels_wallgeo.hip", "WG")):
        assert _constant(src, pre + "_WAVES") == rt.WAVES and _constant(src, pre + "_PLANES") == rt.PLANES
        assert _constant(src, pre + "_MAX_GROUPS") == rt.MAX_GROUPS[which]
        assert re.search(r"\(int64_t\)1 << %d\) / \(%s_WAVES \* cols \* %s_PLANES\)" % (rt.VOXEL_CAP_LOG2[which], pre, pre),
                         open(os.path.join(CSRC, src)).read())
    assert _constant("kernels_signal.hip", "SIG_LSLOTS") == rt.LABEL_SLOTS["signal"]
    assert _constant("kernels_signal.hip", "SIG_PSLOTS") == rt.PAIR_SLOTS["signal"]
    assert _constant("kernels_overlap.hip", "OV_SLOTS") == rt.PAIR_SLOTS["overlap"]
    assert _constant("kernels_wallgeo.hip", "WG_SLOTS") == rt.PAIR_SLOTS["wallgeo"]


# (ncb, nrb, npb, tiles, per, groups, tiles in the last group): computed by hand from the launch code
RECORDED = [
    ((257, 259, 24), 0, 2, "signal", (1, 65, 17, 1105, 2, 553, 1)),
    ((257, 259, 24), 0, 4, "overlap", (1, 65, 17, 1105, 2, 553, 1)),
    ((257, 259, 24), 0, 2, "wallgeo", (1, 65, 17, 1105, 1, 1105, 1)),
    ((258, 259, 24), 1, 2, "signal", (1, 65, 17, 1105, 2, 553, 1)),
    ((17, 1025, 260), 0, 4, "signal", (2, 257, 2, 1028, 2, 514, 2)),
    ((17, 1025, 260), 0, 4, "wallgeo", (2, 257, 2, 1028, 1, 1028, 1)),
    ((17, 1025, 260), 0, 2, "signal", (1, 257, 2, 514, 1, 514, 1)),
    ((257, 1025, 9), 0, 2, "signal", (1, 257, 17, 4369, 5, 874, 4)),
    ((257, 1025, 9), 0, 4, "overlap", (1, 257, 17, 4369, 5, 874, 4)),
    ((257, 1025, 9), 0, 2, "wallgeo", (1, 257, 17, 4369, 2, 2185, 1)),
    ((258, 1025, 9), 1, 4, "wallgeo", (1, 257, 17, 4369, 2, 2185, 1)),
    ((16, 4, 64), 0, 2, "signal", (1, 1, 1, 1, 1, 1, 1)),
    ((33, 9, 70), 0, 4, "wallgeo", (1, 3, 3, 9, 1, 9, 1)),
    # the full-size configuration, for scale: 2048^3 uint32 is 8 x 512 x 128 tiles
    ((2048, 2048, 2048), 0, 4, "signal", (8, 512, 128, 524288, 512, 1024, 512)),
    ((2048, 2048, 2048), 0, 4, "wallgeo", (8, 512, 128, 524288, 128, 4096, 128)),
]


@pytest.mark.parametrize("dims,first_owned,itemsize,which,want", RECORDED)
def test_plan_gives_the_recorded_numbers(dims, first_owned, itemsize, which, want):
    assert tuple(rt.plan(dims, first_owned, itemsize, which)) == want


def test_the_voxel_cap_limits_a_range():
    # a volume of one tile column and 2^15 tiles of uint16: 32 tiles a group by the group count, and the cap (2^31 / 2^15 voxels
    # a tile = 2^16 tiles) is far; a cap that binds needs more than 2^41 voxels and is out of any test's reach
    p = rt.plan((16 * 1024, 4 * 32, 512), 0, 2, "signal")
    assert (p.tiles, p.per, p.groups) == (32768, 32, 1024)
    assert (1 << rt.VOXEL_CAP_LOG2["wallgeo"]) // (rt.WAVES * 512 * rt.PLANES) == 32768


def test_every_case_has_the_property_it_is_used_for():
    c = rt.CASE
    for name in ("a_u16", "a_u32", "a_u16_scalar", "a_u16_halo"):
        for which in ("signal", "overlap"):
            p = rt.plan(c[name].dims, c[name].first_owned, c[name].dtype.itemsize, which)
            assert (p.tiles, p.per, p.groups, p.tiles_in_last_group) == (1105, 2, 553, 1), name     # a clipped last group
            assert p.nrb * rt.WAVES > c[name].dims[1] and p.nrb % p.per == 1                  # a partial row block; ranges straddle plane blocks
    for name in ("b_u32", "b_u32_scalar"):
        p = rt.plan(c[name].dims, 0, 4, "signal")
        assert (p.ncb, p.per, p.groups, p.tiles_in_last_group) == (2, 2, 514, 2), name             # a group = both column blocks of a row block
        assert c[name].dims[2] - rt.columns(4) in (3, 4)                                           # ... the second a few columns wide
        assert c[name].dims[1] % rt.WAVES == 1                                                     # the last row block has one row: r >= n1 skips in a range
    for name in ("c_u16", "c_u32", "c_u16_vector", "c_u32_vector", "c_u32_halo"):
        k = c[name]
        p = rt.plan(k.dims, k.first_owned, k.dtype.itemsize, "signal")
        assert (p.tiles, p.per, p.groups, p.tiles_in_last_group) == (4369, 5, 874, 4), name
        assert p == rt.plan(k.dims, k.first_owned, k.dtype.itemsize, "overlap")
        w = rt.plan(k.dims, k.first_owned, k.dtype.itemsize, "wallgeo")
        assert (w.per, w.groups, w.tiles_in_last_group) == (2, 2185, 1), name
        assert p.nrb % p.per != 0 and w.nrb % w.per != 0                                          # ranges start anywhere in a plane block
    # the load path each case takes (aligned buffers)
    vec = dict((k.name, rt.vector_path(k.dims, k.dtype.itemsize)) for k in rt.CASES)
    assert vec == {"a_u16": True, "a_u32": True, "a_u16_scalar": False, "b_u32": True, "b_u32_scalar": False, "c_u16": False,
                   "c_u32": False, "c_u16_vector": True, "c_u32_vector": True, "a_u16_halo": True, "c_u32_halo": False}
    # the halo cases own exactly the planes of the cases without one
    assert c["a_u16_halo"].dims[0] - 1 == c["a_u16"].dims[0] and c["c_u32_halo"].dims[0] - 1 == c["c_u32"].dims[0]
    # no small shape of the older GPU tests reaches a second tile in a group
    assert rt.plan((128, 128, 64), 0, 2, "signal").per == 1


def test_group_image_walks_the_tiles_in_the_kernels_order():
    dims = (35, 9, 600)
    for first_owned in (0, 1):
        g = rt.group_image(dims, first_owned, 4, "signal")                     # 3 column blocks x 3 row blocks x 3 plane blocks, a tile a group
        p = rt.plan(dims, first_owned, 4, "signal")
        assert (p.ncb, p.nrb, p.npb, p.per) == (3, 3, 3, 1)
        assert g.shape == dims and (g[:first_owned] == -1).all()
        f = first_owned
        assert g[f, 0, 0] == 0 and g[f, 0, 256] == 1 and g[f, 4, 0] == 3 and g[f + 16, 0, 0] == 9 and g[-1, -1, -1] == 26
        assert g[f + 15, 3, 255] == 0
    g = rt.group_image(rt.CASE["b_u32"].dims, 0, 4, "signal")
    assert g[0, 0, 0] == g[0, 3, 259] == 0 and g[0, 4, 0] == 1 and g.max() == 513


def test_spill_bounds_on_the_permutation_volumes():
    V = rt.permutation_labels(rt.SPILL_DIMS, np.uint16, 1)
    assert sorted(V.reshape(-1).tolist()) == list(range(4096))
    assert tuple(rt.plan(V.shape, 0, 2, "signal")) == (1, 1, 1, 1, 1, 1, 1)
    S = rt.random_image(V.shape, np.uint16, 2)
    w = signal_reference.walls(V, S)
    faces = 15 * 4 * 64 + 16 * 3 * 64 + 16 * 4 * 63
    assert w["keys"].size == faces == 10944 and (w["faces"].sum(axis=1) == 1).all()           # every face its own pair
    assert wall_geometry_reference.rows(V)["lo"].size == 10944
    assert rt.label_spill_bound(V, 0) == 4096 - 512
    assert rt.wall_spill_bound(V, 0, "signal") == 10944 - 2048
    assert rt.wall_spill_bound(V, 0, "wallgeo") == 10944 - 512
    for B in (np.zeros(V.shape, np.uint16), rt.block_labels(V.shape, np.uint32, 3)):
        assert overlap_reference.table(V, B)[0].size == 4096                                  # against any B
        assert rt.overlap_spill_bound(V, B, 0) == 4096 - 2048
    W = rt.permutation_labels(rt.SPILL_DIMS_WIDE, np.uint32, 1)
    assert W.size == 20790 and signal_reference.walls(W, np.zeros(W.shape, np.uint8))["keys"].size == 59133
    assert not rt.vector_path(W.shape, 4) and rt.plan(W.shape, 0, 4, "signal").groups == 9
    # nine groups, partial ones among them: the bounds come from the distinct keys of each
    g = rt.group_image(W.shape, 0, 4, "signal")
    sizes = np.bincount(g.reshape(-1))
    assert rt.label_spill_bound(W, 0) == int(np.maximum(sizes - 512, 0).sum()) > 10000
    assert rt.wall_spill_bound(W, 0, "signal") > 40000 and rt.wall_spill_bound(W, 0, "wallgeo") > 50000
    assert rt.overlap_spill_bound(W, W, 0) == int(np.maximum(sizes - 2048, 0).sum()) > 5000


def test_spill_bounds_follow_the_halo_rule_and_the_groups():
    # two labels in stripes along axis 2: one pair however many faces; a table of 512 slots never has to spill
    V = np.zeros((20, 9, 40), dtype=np.uint16)
    V[:, :, 1::2] = 1
    assert rt.wall_spill_bound(V, 0, "wallgeo") == 0 and rt.label_spill_bound(V, 0) == 0
    # a halo plane of noise adds its faces with plane 1 only, and no label
    H = rt.permutation_labels((3, 8, 600), np.uint32, 4) + np.uint32(100)
    H[1:] = 7
    assert rt.label_spill_bound(H, 1) == 0
    # plane 1 walks 8 x 600 faces of distinct pairs (7, x): 3 column blocks x 2 row blocks, 1024 or 352 faces a group
    assert rt.wall_spill_bound(H, 1, "wallgeo") == 4 * (1024 - 512)
    assert rt.wall_spill_bound(H, 1, "signal") == 0
    assert rt.wall_spill_bound(H, 0, "signal") > 0                                             # without the rule the plane's own faces count


def test_volume_makers():
    for k in rt.CASES:
        V = rt.block_labels(k.dims, k.dtype, 1)
        assert V.shape == k.dims and V.dtype == k.dtype and V.flags.c_contiguous
        assert 1 <= V.min() and V.max() <= 300
    V = rt.block_labels((40, 40, 40), np.uint16, 1)
    assert (V[:5, :7, :3] == V[0, 0, 0]).all() and np.unique(V).size > 250
    # blocks of 5 x 7 x 3 never line up with tiles of 16 x 4 x 256: label runs cross every kind of boundary
    assert all(b % 2 == 1 for b in (5, 7, 3))
    for axis in range(3):
        for swap in (False, True):
            h = rt.half_space((6, 8, 10), np.uint16, axis, swap=swap)
            r = wall_geometry_reference.rows(h)
            assert r["lo"].tolist() == [2] and r["hi"].tolist() == [5]
            side, other = (r["rev"], r["fwd"]) if swap else (r["fwd"], r["rev"])
            assert not other.any() and side[0].tolist() == [h.size // h.shape[axis] if a == axis else 0 for a in range(3)]
    N = rt.noise_box(V, (slice(3, 9), slice(0, 40), slice(10, 20)), 5, 60000)
    assert (N != V).sum() > 0.99 * 6 * 40 * 10 and np.array_equal(N[9:], V[9:]) and np.array_equal(N[:, :, 20:], V[:, :, 20:])
