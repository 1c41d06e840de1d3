"""The distance-shell profiles on the GPU (include/tissue_scan_profile.h, csrc/kernels_profile.hip) against
tests/profile_reference.py, bit for bit: every case feeds the reference with the D2 image the context holds (ta_distance_image), and
where the volume is small enough for it and the spacing a power of two also with distance_reference.brute_d2, to which the header of
the distance maps promises that image to be bit-identical.

The shapes are the smallest at which the pass can still go wrong: rows that are whole 16-byte strips of labels (528, 264) and rows
that are not (531), planes that are no whole tiles, several tiles and workgroups, ranges of two tiles a workgroup, axes of one
voxel, one voxel, a table with more keys than a workgroup's LDS table has slots, and buffers off a 16-byte boundary."""
import ctypes
import functools

import numpy as np
import pytest

import distance_reference as dref
import profile_reference as pref
import range_tiles as rt
from feature_passes import Pass, code, poke
from tissue_analysis_amd import DICT, ShellProfile, SpatialImage, SpatialImageAnalysis, _capi, synth
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu

OWN, FROM = _capi.DIST_OWN_WALL, _capi.DIST_FROM_LABEL
UNIT, HALF = (1.0, 1.0, 1.0), (0.5, 0.5, 1.0)
BG = synth.BACKGROUND
EDGES = np.array([0.0, 1.0, 1.5, 2.0, 3.0, np.inf])          # distances; the kernels take their squares
PLAN = "profile"                                             # range_tiles.plan: 4096 workgroups at most, every plane walked (first_owned = 0)


@functools.lru_cache(maxsize=None)
def voronoi(shape, cells, seed=3):
    v = synth.voronoi_labels(shape, cells, seed, dtype=np.uint16)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def signal(shape, dtype, seed=8):
    s = rt.random_image(shape, dtype, seed)
    s.setflags(write=False)
    return s


def same(got, want):
    """The five columns of ctx.profile_get() against the reference's table."""
    assert got[0].shape == want["n"].shape and np.array_equal(got[0], want["n"])
    if "sum" not in want:
        assert got[1:] == (None, None, None, None)
        return
    assert np.array_equal(got[1], want["sum"])
    assert np.array_equal(got[2], pref.words(want["sumsq"]))
    assert np.array_equal(got[3], want["min"]) and np.array_equal(got[4], want["max"])   # (empty: UINT32_MAX and 0 on both sides)


def profile(ctx, V, S, edges2, rows, d2=None):
    """One profile pass over the distance map the context holds, against the reference fed with that map's D2 (and with `d2` when
    given, which must be the same image); V, S and d2 in the axes of a C-ordered volume.  Returns (table, debug)."""
    held = ctx.distance_image().reshape(V.shape)
    if d2 is not None:
        assert np.array_equal(held, d2)
    ctx.profile_extract(edges2, S is not None)
    got = ctx.profile_get()
    same(got, pref.table(V, held, S, edges2, rows))
    assert ctx.profile_timing() >= 0.0
    return got, ctx.profile_debug()


# ---- 1. Voronoi volumes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
@pytest.mark.parametrize("shape,cells", [((19, 7, 531), 60), ((19, 7, 528), 60), ((33, 10, 264), 40)])
def test_voronoi(shape, cells, dtype):
    V = voronoi(shape, cells).astype(dtype)
    e2 = np.square(EDGES)
    with Pass(V) as p:
        p.extract(features=_capi.F_VOLUME)
        plan = p.plan(PLAN)
        assert plan.tiles > 4 and plan.groups > 1
        edge_flag_runs = 0
        for mode, edge in ((OWN, False), (FROM, False), (OWN, True)):
            p.ctx.distance_extract(mode, BG, HALF, _capi.DIST_EDGE_IS_SITE if edge else 0)
            edge_flag_runs += edge
            for sdtype in (None, np.uint8, np.uint16):
                S = None if sdtype is None else signal(shape, sdtype)
                if S is not None:
                    p.ctx.set_signal(S)                       # (a new signal leaves the distance map alone)
                got, debug = profile(p.ctx, V, S, e2, p.max_label + 1)
                assert (debug["tiles_per_group"], debug["groups"]) == (plan.per, plan.groups)
                assert debug["spills"] == 0
                assert int((got[0].sum(axis=0) > 0).sum()) >= 3  # the voxels spread over the shells
        assert edge_flag_runs == 1


@pytest.mark.parametrize("case,sdtype", [("c_u16_vector", np.uint8), ("c_u32", None), ("c_u16", np.uint16)])
def test_a_range_of_two_tiles_a_workgroup(case, sdtype):
    """(257, 1025, 8 or 9): 4369 tiles, two a workgroup, the last workgroup one; rows of 8 labels take the vector loads of uint16,
    rows of 9 the edge path."""
    c = rt.CASE[case]
    V = rt.block_labels(c.dims, c.dtype, 11)
    S = None if sdtype is None else signal(c.dims, sdtype)
    with Pass(V) as p:
        p.extract(features=_capi.F_VOLUME)
        p.ctx.distance_extract(OWN, 0, UNIT, 0)
        if S is not None:
            p.ctx.set_signal(S)
        _, debug = profile(p.ctx, V, S, np.square(EDGES), p.max_label + 1)
        plan = p.plan(PLAN)
        assert (debug["tiles_per_group"], debug["groups"]) == (plan.per, plan.groups) == (2, 2185) and plan.tiles_in_last_group == 1


# ---- 2. thin volumes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 77), (5, 1, 64), (1, 9, 40)])
def test_thin_volumes(shape):
    rng = np.random.default_rng(5)
    V = np.repeat(rng.integers(0, 3, shape[:2] + ((shape[2] + 3) // 4,)), 4, axis=2)[:, :, :shape[2]].astype(np.uint16)
    S = signal(shape, np.uint16)
    with Pass(V) as p:
        p.extract(max_label=2, features=_capi.F_VOLUME)
        p.ctx.set_signal(S)
        for mode in (OWN, FROM):
            for edge in (False, True):
                p.ctx.distance_extract(mode, 0, HALF, _capi.DIST_EDGE_IS_SITE if edge else 0)
                d2 = dref.brute_d2(V, HALF, mode, 0, edge)
                profile(p.ctx, V, S, np.square([0.0, 0.5, 1.0, 2.0, np.inf]), 3, d2)
                profile(p.ctx, V, None, np.square([0.0, 0.5, 1.0, 2.0, np.inf]), 3, d2)


# ---- 3. edge rules ------------------------------------------------------------------------------------------------------------
def test_edge_rules():
    shape = (19, 7, 528)
    V = voronoi(shape, 60)
    S = signal(shape, np.uint16)
    with Pass(V) as p:
        p.extract(features=_capi.F_VOLUME)
        rows = p.max_label + 1
        p.ctx.set_signal(S)
        p.ctx.distance_extract(OWN, 0, UNIT, 0)
        d2 = p.ctx.distance_image()
        top = float(d2[np.isfinite(d2)].max())
        assert d2.min() == 1.0 and top > 4.0
        got, _ = profile(p.ctx, V, S, np.array([0.0, np.inf]), rows)                       # K = 1
        assert int(got[0].sum()) == V.size
        got, _ = profile(p.ctx, V, S, np.linspace(0.0, top + 1.0, 65), rows)               # K = 64
        assert got[0].shape == (rows, 64) and int(got[0].sum()) == V.size
        got, _ = profile(p.ctx, V, S, np.concatenate([np.arange(64.0), [np.inf]]), rows)   # K = 64, a voxel on every edge it reaches
        assert int(got[0].sum()) == V.size and int((got[0].sum(axis=0) > 0).sum()) > 3
        got, _ = profile(p.ctx, V, None, np.array([2.0, 4.0, top]), rows)                  # neither the smallest nor the largest
        assert int(got[0].sum()) == int(((d2 >= 2.0) & (d2 < top)).sum()) < V.size - int((d2 == 1.0).sum())
        p.ctx.distance_extract(FROM, 9999, UNIT, 0)                                        # a site label the volume does not hold
        assert np.isinf(p.ctx.distance_image()).all()
        got, _ = profile(p.ctx, V, S, np.array([0.0, 1.0, np.inf]), rows)
        assert not got[0].any() and not got[1].any() and (got[3] == 0xFFFFFFFF).all() and not got[4].any()


def test_uniform_volume():
    V = np.full((5, 6, 70), 4, dtype=np.uint16)
    S = signal(V.shape, np.uint8)
    with Pass(V) as p:
        p.extract(features=_capi.F_VOLUME)
        p.ctx.set_signal(S)
        p.ctx.distance_extract(OWN, 0, HALF, 0)                                            # no other label, no margin: +inf everywhere
        got, _ = profile(p.ctx, V, S, np.square(EDGES), 5)
        assert not got[0].any() and not got[1].any() and not got[2].any() and (got[3] == 0xFFFFFFFF).all() and not got[4].any()
        p.ctx.distance_extract(OWN, 0, HALF, _capi.DIST_EDGE_IS_SITE)
        got, _ = profile(p.ctx, V, S, np.square(EDGES), 5)
        assert int(got[0][4].sum()) == V.size and not got[0][:4].any()


# ---- 4. totals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdtype", [np.uint8, np.uint16])
def test_totals_are_those_of_the_extraction_and_of_the_signal_pass(sdtype):
    shape = (33, 10, 264)
    V = voronoi(shape, 40)
    S = signal(shape, sdtype)
    with Pass(V) as p:
        p.extract()
        rows = p.max_label + 1
        p.ctx.set_signal(S)
        p.ctx.signal_extract(_capi.SIG_LABELS)
        n, s, q, mn, mx = p.ctx.signal_labels()
        count = p.ctx.labels()[0]
        p.ctx.distance_extract(OWN, 0, HALF, 0)
        d2 = p.ctx.distance_image().reshape(shape)
        finite = np.array([bool(np.isfinite(d2[V == l]).all()) for l in range(rows)])      # (an absent row: vacuously)
        assert finite.all() and (count > 0).sum() > 10
        got, _ = profile(p.ctx, V, S, np.array([0.0, np.inf]), rows)
        assert np.array_equal(got[0][:, 0], count) and np.array_equal(got[0][:, 0], n)
        assert np.array_equal(got[1][:, 0], s) and np.array_equal(got[2][:, 0], q)
        assert np.array_equal(got[3][:, 0], mn) and np.array_equal(got[4][:, 0], mx)


# ---- 5. spills ----------------------------------------------------------------------------------------------------------------
def test_more_keys_than_a_workgroup_has_slots():
    """A permutation volume of one tile and one workgroup: 4096 labels.  In mode 1 from one voxel's label every voxel has a finite
    distance, so under a last edge of +inf there are 4096 keys, spread over the shells; whatever the hash does, at least
    4096 - slots records find no slot (pigeonhole, as in test_gpu_feature_table_spills.py)."""
    V = rt.permutation_labels(rt.SPILL_DIMS, np.uint16, 21)
    S = signal(V.shape, np.uint16)
    edges2 = np.square([0.0, 2.0, 4.0, 8.0, 16.0, 32.0, np.inf])
    with Pass(V) as p:
        p.extract(features=_capi.F_VOLUME)
        p.ctx.set_signal(S)
        p.ctx.distance_extract(FROM, int(V[3, 1, 20]), UNIT, 0)
        got, debug = profile(p.ctx, V, S, edges2, p.max_label + 1)
        assert (debug["tiles_per_group"], debug["groups"]) == (1, 1)
        assert int(got[0].sum()) == 4096 and int((got[0] > 0).sum()) == 4096 and (got[0].sum(axis=0) > 0).all()
        assert debug["spills"] >= 4096 - _capi.PROFILE_SLOTS > 0
        got, debug = profile(p.ctx, V, None, edges2, p.max_label + 1)                      # the kernel without the signal columns
        assert debug["spills"] >= 4096 - _capi.PROFILE_SLOTS


# ---- 6. layouts and buffers ---------------------------------------------------------------------------------------------------
def test_layouts():
    shape = (24, 40, 56)
    V = voronoi(shape, 30)
    S = signal(shape, np.uint16)
    e2 = np.square(EDGES)
    tables = []
    for A, B in ((V, S), (np.asfortranarray(V), np.asfortranarray(S)),
                 (np.ascontiguousarray(V.transpose(1, 2, 0)).transpose(2, 0, 1), np.ascontiguousarray(S.transpose(2, 0, 1)).transpose(1, 2, 0))):
        rv = ResidentVolume(A)
        try:
            x = rv.extract(_capi.F_VOLUME, sparse=False)
            rv.ctx.distance_extract(OWN, 0, HALF, 0)
            d2 = np.array(rv.distance_image())                # array axes, whatever the memory layout
            rv.ctx.set_signal(B)                              # (stored in another permutation than the labels: copied into theirs)
            rv.ctx.profile_extract(e2, True)
            got = rv.ctx.profile_get()
            same(got, pref.table(V, d2, S, e2, x.nrows))
            tables.append(got)
        finally:
            rv.close()
    for t in tables[1:]:
        for a, b in zip(t, tables[0]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype,offsets", [(np.uint16, (0, 1, 4)), (np.uint32, (0, 1, 2))], ids=["u16", "u32"])
@pytest.mark.parametrize("sdtype,sbytes", [(np.uint8, 1), (np.uint16, 2), (np.uint16, 8)], ids=["s8+1B", "s16+2B", "s16+8B"])
def test_adopted_buffers_off_a_16_byte_boundary(dtype, offsets, sdtype, sbytes):
    from test_gpu_unaligned_buffers import adopt, offset_view, signal_image
    shape = (19, 7, 528)
    V = voronoi(shape, 60).astype(dtype)
    S = signal_image(shape, sdtype, 7)
    rows = int(V.max()) + 2                                   # a row for the sentinel of the pads too: it must stay empty
    e2 = np.square(EDGES)
    control = None
    for off in offsets:                                       # offset 0 is the aligned control (of the labels)
        ctx = _capi.Context(0)
        try:
            ov = adopt(ctx, V, off)
            sv = offset_view(S, sbytes // np.dtype(sdtype).itemsize, 5)
            assert sv.dev_ptr % 16 == sbytes
            ctx.set_signal_device(sv.dev_ptr, np.dtype(sdtype).itemsize, keep=sv.flat)
            ctx.extract(_capi.F_VOLUME, rows - 1)
            ctx.distance_extract(OWN, 0, HALF, 0)
            got, _ = profile(ctx, V, S, e2, rows)
            assert not got[0][rows - 1].any()
            ov.read_back()
            sv.read_back()
            control = got if control is None else control
            for a, b in zip(got, control):
                assert np.array_equal(a, b)
        finally:
            ctx.close()


# ---- 7. sparse ids ------------------------------------------------------------------------------------------------------------
def test_sparse_ids():
    shape = (19, 7, 528)
    V = voronoi(shape, 60)
    W = V.astype(np.uint32) * np.uint32(1000003)
    S = signal(shape, np.uint16)
    rv = ResidentVolume(W)
    try:
        x = rv.extract(_capi.F_VOLUME, sparse=True)
        assert rv.ctx.is_compact()
        dm = rv.distance_map(FROM, BG * 1000003, HALF)
        prof = dm.profile(EDGES, S)
        d2 = np.array(rv.distance_image())
        ids, want = pref.table_by_id(W, d2, S, np.square(EDGES))
        assert isinstance(prof, ShellProfile) and np.array_equal(prof.labels, ids) and np.array_equal(prof.labels, x.ids)
        assert np.array_equal(prof.n, want["n"]) and np.array_equal(prof.sum, want["sum"])
        assert prof.sumsq.tolist() == want["sumsq"].tolist()
        assert np.array_equal(prof.min, want["min"]) and np.array_equal(prof.max, want["max"])
        assert prof.count()[BG * 1000003].tolist() == [int((W == BG * 1000003).sum()), 0, 0, 0, 0]      # the site voxels read 0: shell 0
    finally:
        rv.close()


# ---- 8. invalidation and errors -----------------------------------------------------------------------------------------------
def test_invalidation_and_argument_checks():
    shape = (19, 7, 528)
    V = voronoi(shape, 60)
    S = signal(shape, np.uint16)
    top = int(V.max())
    e2 = np.square(EDGES)
    ctx = _capi.Context(0)
    try:
        getters = (ctx.profile_get, ctx.profile_debug, ctx.profile_timing)

        def stale():
            return all(code(call) == _capi.TA_EINVAL for call in getters)

        def current(labels, with_signal):
            ctx.distance_extract(OWN, 0, HALF, 0)
            assert stale()                                                         # a new ta_distance_extract
            profile(ctx, labels, S if with_signal else None, e2, top + 1)

        assert stale() and code(ctx.profile_extract, e2) == _capi.TA_EINVAL        # no volume
        ctx.set_volume(V)
        assert code(ctx.profile_extract, e2) == _capi.TA_EINVAL                    # no extraction
        ctx.extract(_capi.F_VOLUME, top)
        assert stale() and code(ctx.profile_extract, e2) == _capi.TA_EINVAL        # no distance results
        ctx.distance_extract(OWN, 0, HALF, 0)
        assert stale()
        assert code(ctx.profile_extract, e2, True) == _capi.TA_EINVAL              # a signal requested but absent
        for bad in ([0.0], np.arange(67.0), [0.0, 2.0, 1.0], [0.0, 1.0, 1.0], [-1.0, 1.0], [0.0, float("nan")], [float("nan"), 1.0],
                    [0.0, 1.0, float("nan"), 4.0], []):
            assert code(ctx.profile_extract, np.asarray(bad, dtype=np.float64)) == _capi.TA_EINVAL, bad
        edges = (ctypes.c_double * 3)(0.0, 1.0, 4.0)
        assert ctx._lib.ta_profile_extract(ctx._h, 2, edges, 2) == _capi.TA_EINVAL           # an unknown flag
        assert ctx._lib.ta_profile_extract(ctx._h, 2, None, 0) == _capi.TA_EINVAL
        assert ctx._lib.ta_profile_extract(ctx._h, 65, edges, 0) == _capi.TA_EINVAL
        assert stale()
        profile(ctx, V, None, e2, top + 1)
        n = np.zeros((top + 1, 5), dtype=np.uint64)
        assert ctx._lib.ta_profile_get(ctx._h, None, None, None, None, None) == _capi.TA_OK
        for column in range(1, 5):                                                 # a pass without signal has no signal columns
            args = [None] * 5
            args[column] = n.ctypes.data
            assert ctx._lib.ta_profile_get(ctx._h, *args) == _capi.TA_EINVAL
        ctx.set_signal(S)
        assert not stale()                                                         # a new signal, but the table did not read one
        profile(ctx, V, S, e2, top + 1)
        ctx.set_signal(S)                                                          # a new signal under a table that read the old one
        assert stale()
        current(V, True)

        ctx.extract(_capi.F_ALL, top)                                              # a new ta_extract
        assert stale() and code(ctx.profile_extract, e2) == _capi.TA_EINVAL
        current(V, True)
        lut = np.arange(top + 1, dtype=np.uint32)
        lut[5] = 3
        ctx.relabel(lut)                                                           # ta_volume_relabel
        assert stale() and code(ctx.profile_extract, e2) == _capi.TA_EINVAL
        ctx.extract(_capi.F_VOLUME, top)
        current(lut[V].astype(np.uint16), True)
        ctx.set_volume(V)                                                          # a new volume (of the same dims: the signal stays)
        assert stale()
        ctx.extract(_capi.F_VOLUME, top)
        current(V, False)
    finally:
        ctx.close()


def test_a_label_above_max_label():
    V = rt.block_labels((24, 20, 70), np.uint16, 31, nlabels=40)
    S = signal(V.shape, np.uint16)
    e2 = np.square(EDGES)
    with Pass(V, adopted=True) as p:
        p.extract(features=_capi.F_VOLUME)
        p.set_signal(S)
        p.ctx.distance_extract(OWN, 0, UNIT, 0)
        before, _ = profile(p.ctx, V, S, e2, p.max_label + 1)
        poke(p.t, (3, 4, 5), 65535)                            # 65535 * K + shell is far outside the rows
        p.ctx.profile_extract(e2, True)
        for get in (p.ctx.profile_get, p.ctx.profile_debug):
            assert code(get) == _capi.TA_ERANGE
        p.ctx.profile_extract(e2, False)
        assert code(p.ctx.profile_get) == _capi.TA_ERANGE
        poke(p.t, (3, 4, 5), V[3, 4, 5])
        assert code(p.ctx.profile_get) == _capi.TA_ERANGE      # the results of that pass stay what they are
        after, _ = profile(p.ctx, V, S, e2, p.max_label + 1)   # the same distance map, the volume as it was: the context works on
        for a, b in zip(after, before):
            assert np.array_equal(a, b)
        p.extract(features=_capi.F_VOLUME)
        p.ctx.distance_extract(OWN, 0, UNIT, 0)
        profile(p.ctx, V, S, e2, p.max_label + 1)


# ---- 9. the public API, end to end --------------------------------------------------------------------------------------------
def test_public_api():
    shape, vs = (8, 10, 16), (0.5, 0.5, 1.0)
    V = voronoi(shape, 6, 5)
    S = signal(shape, np.uint16)
    edges = [0.0, 0.6, 1.0, 1.5, np.inf]
    e2 = np.square(edges)
    sia = SpatialImageAnalysis(SpatialImage(V, voxelsize=vs), ignoredlabels=0, return_type=DICT, background=BG)
    labels = sia.labels()
    assert BG not in labels and len(labels) > 3
    rows = int(V.max()) + 1
    wall, depth = dref.brute_d2(V, vs), dref.brute_d2(V, vs, FROM, BG)
    own, deep = pref.table(V, wall, S, e2, rows), pref.table(V, depth, S, e2, rows)

    volumes = sia.shell_volumes(edges)
    assert sorted(volumes) == labels
    assert all(np.array_equal(volumes[l], own["n"][l].astype(np.float64) * 0.25) for l in labels)
    below = sia.shell_volumes(edges, from_label=BG)           # (the context holds this map now)
    assert all(np.array_equal(below[l], deep["n"][l].astype(np.float64) * 0.25) for l in labels)
    voxels = sia.shell_volumes([0.0, 1.5, 2.5, np.inf], labels=labels[:3], real=False)
    unit = pref.table(V, dref.brute_d2(V), None, np.square([0.0, 1.5, 2.5, np.inf]), rows)
    assert sorted(voxels) == labels[:3] and all(np.array_equal(voxels[l], unit["n"][l].astype(np.float64)) for l in labels[:3])
    edged = sia.shell_volumes(edges, edge_is_wall=True)
    cut = pref.table(V, dref.brute_d2(V, vs, edge=True), None, e2, rows)
    assert all(np.array_equal(edged[l], cut["n"][l].astype(np.float64) * 0.25) for l in labels)

    def column(t, name):
        with np.errstate(invalid="ignore", divide="ignore"):
            n, s = t["n"].astype(np.float64), t["sum"].astype(np.float64)
            if name == "mean":
                return np.where(n > 0, s / n, np.nan)
            if name == "fraction":
                return s / s.sum(axis=1, keepdims=True)
            if name == "sum":
                return t["sum"]
            return np.where(n > 0, t[name].astype(np.float64), np.nan)

    for statistic in ("mean", "fraction", "sum", "min", "max"):
        got = sia.signal_profile(S, edges, statistic=statistic)          # the wall map was displaced by the later ones: it runs again
        want = column(own, statistic)
        assert sorted(got) == labels and all(np.array_equal(got[l], want[l], equal_nan=True) for l in labels), statistic
    got = sia.signal_profile(S, edges, statistic="std", from_label=BG)
    for l in labels:
        for k in range(4):
            v = S[(V == l) & (depth >= e2[k]) & (depth < e2[k + 1])].astype(np.float64)
            assert (np.isnan(got[l][k]) and not v.size) or abs(got[l][k] - v.std()) <= 1e-9 * max(v.std(), 1.0)
    with pytest.raises(ValueError):
        sia.signal_profile(S, edges, statistic="median")

    dm = sia.wall_distance()                                  # the cached map; the context holds the depth map by now
    prof = dm.profile(edges)
    assert not prof.has_signal and np.array_equal(prof.n, own["n"]) and prof.edges.tolist() == edges and prof.ms >= 0.0
    assert np.array_equal(sia.distance_from().profile(edges, S).sum, deep["sum"])
    assert np.array_equal(dm.profile(edges, S).sum, own["sum"])
