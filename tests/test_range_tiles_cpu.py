"""range_tiles.py does what it claims, with no GPU: the restated launch plan gives the recorded numbers, every shape of
test_gpu_tile_ranges.py and test_gpu_feature_table_spills.py has the property it is used for, and the restated constants are
the ones the kernels are compiled with today."""
import os
import re
import subprocess

import numpy as np
import pytest

import overlap_reference
import range_tiles as rt
import sighist_reference
import signal_reference
import wall_geometry_reference

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tissue_analysis_amd", "csrc")


def _constant(source, name):
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*\d+\s*,\s*)*%s\s*=\s*(\d+)" % name, open(os.path.join(CSRC, source)).read())
    assert m, name
    return int(m.group(1))


def _named(text, name):
    """The integer behind `name` in the sources `text`: a literal, a constexpr, or the default a #define gives."""
    return int(name) if name.isdigit() else _named(text, re.search(r"(?:constexpr\s+\w+|#define)\s+%s\s*=?\s*(\w+)" % name, text).group(1))


def range_shape(which):
    """(waves, planes, max_groups, voxel_cap_log2) of the one RangeShape line of the pass's kernel file (names: there or in its header)."""
    text = "".join(open(os.path.join(CSRC, f % which)).read() for f in ("kernels_%s.hip", "ta_%s.h"))
    (fields,) = re.findall(r"constexpr\s+RangeShape\s+\w+\s*=\s*\{([^}]*)\}", text)
    return tuple(_named(text, f.strip()) for f in fields.split(","))


def test_restated_constants_are_the_sources():
    """A retuned tile, table, group count or voxel cap must change range_tiles.py (and the shapes below) deliberately."""
    assert sorted(rt.MAX_GROUPS) == sorted(rt.VOXEL_CAP_LOG2) == ["overlap", "profile", "sighist", "sigmoments", "signal", "wallgeo"]
    for which in rt.MAX_GROUPS:
        assert range_shape(which) == (rt.WAVES, rt.PLANES, rt.MAX_GROUPS[which], rt.VOXEL_CAP_LOG2[which]), which
    assert _constant("ta_sigmoments.h", "SM_SLOTS") == rt.LABEL_SLOTS["sigmoments"]
    assert _constant("ta_profile.h", "PROF_SLOTS") == rt.KEY_SLOTS["profile"]
    assert _named(open(os.path.join(CSRC, "ta_sighist.h")).read(), "SH_SLOTS") == rt.KEY_SLOTS["sighist"]
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


@pytest.fixture(scope="module")
def range_plan_exe(tmp_path_factory):
    """tests/native/range_plan.cpp: csrc/ta_range_plan.h compiled as plain host C++ by the compiler of the build."""
    from tissue_analysis_amd import build as ta_build
    exe = str(tmp_path_factory.mktemp("range_plan") / "range_plan")
    subprocess.check_call([ta_build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-I", CSRC,
                           os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "range_plan.cpp"), "-o", exe])
    return lambda mode, lines: subprocess.run([exe, mode], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True,
                                              universal_newlines=True, timeout=60).stdout.split("\n")[:-1]


def test_the_header_computes_the_restated_plan(range_plan_exe):
    """range_tiles + plan_ranges of ta_range_plan.h against rt.plan: the recorded rows, and the passes they do not cover."""
    rows = [(dims, first_owned, itemsize, which) for dims, first_owned, itemsize, which, _ in RECORDED]
    rows += [(sighist_reference.two_tile_dims(itemsize, vector), 0, itemsize, "sighist") for itemsize in (2, 4) for vector in (True, False)]
    rows += [((1 << 14, 1 << 16, 1 << 18), 0, 2, "sighist")]                          # 2^48 voxels: the voxel cap binds
    rows += [((257, 1025, 9), 0, itemsize, which) for itemsize in (2, 4) for which in ("profile", "sigmoments")]
    rows += [((1, 5, 7), 1, 2, "signal"), ((0, 5, 7), 0, 4, "wallgeo")]               # nothing owned: no tile, no group
    out = range_plan_exe("plan", ["%d %d %d %d %d %d %d %d %d" % (tuple(dims) + (first_owned, itemsize, rt.WAVES, rt.PLANES, rt.MAX_GROUPS[which],
                                                                                  rt.VOXEL_CAP_LOG2[which])) for dims, first_owned, itemsize, which in rows])
    assert len(out) == len(rows)
    for (dims, first_owned, itemsize, which), line in zip(rows, out):
        want = tuple(rt.plan(dims, first_owned, itemsize, which))[:6] if dims[0] > first_owned else (0,) * 6
        assert tuple(int(v) for v in line.split()) == want, (dims, first_owned, itemsize, which)
    assert out[len(RECORDED) + 4].split()[4:] == ["65536", "131072"]                # the capped plan, by hand: 2^31 / 2^15 tiles a group


def test_the_header_takes_the_vector_loads_where_expected(range_plan_exe):
    """strips_vectorize: rows of whole strips, and every buffer aligned to min(strip, 16) bytes.  Expected by hand."""
    whole = {2: (8, 24), 4: (8, 24)}                                   # n2 of 8, 9, 23, 24 that are whole strips of 8 / 4 labels
    aligned = {(2, 1): (0, 8, 16), (4, 1): (0, 4, 8, 16),              # uint8 signal: strips of 8 / 4 bytes
               (2, 2): (0, 16), (4, 2): (0, 8, 16),                    # uint16 signal: 16 / 8 bytes
               (2, 8): (0, 16), (4, 8): (0, 16)}                       # f64: 64 / 32 bytes, loaded 16 at a time
    cases = [(n2, lw, size, off) for n2 in (8, 9, 23, 24) for lw in (2, 4)
             for size, offs in ((1, (0, 2, 4, 8, 16)), (2, (0, 2, 4, 8, 16)), (8, (0, 8, 16))) for off in offs]
    out = range_plan_exe("vec", ["%d %d 2 4096 %d %d %d" % (n2, lw, lw, 4096 + off, size) for n2, lw, size, off in cases])
    assert [int(v) for v in out] == [int(n2 in whole[lw] and off in aligned[lw, size]) for n2, lw, size, off in cases]
    assert sum(int(v) for v in out) == 2 * (3 + 4 + 2 + 3 + 2 + 2)
    # the labels' own buffer needs 16 bytes; a buffer of item size 0 is not read
    assert range_plan_exe("vec", ["8 2 1 4104 2", "8 2 1 4112 2", "8 2 2 4096 2 4099 0"]) == ["0", "1", "1"]


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
