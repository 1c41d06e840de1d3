"""What the entry points behind the count-then-emit passes answer in every state of a context: the code and the FULL message of
ta_junctions_size / _get_edges / _get_vertices / _debug / _timing, ta_components_size / _get / _image / _debug / _timing,
ta_overlap_size / _get / _debug / _timing / _timing_compaction and ta_mesh_size / _get / _timing.

Written the way test_gpu_getter_answers.py is: host logic only (the volumes are tiny).  A scenario brings a fresh Context into one
state and asks every entry point once, each as C would call it; the answer is (code, message), (0, "") for success -- the values of
a successful answer are the business of each feature's own file, and what a cause of staleness does to the tables themselves that
of test_gpu_state_invalidation.py.  The table EXPECTED below was RECORDED on the commit before these passes got their shared
count/scan block, sort view and summed timing: it states what the library did, not what it should do, and is never regenerated from
the code under test.
"""
import ctypes

import numpy as np
import pytest

from tissue_analysis_amd import _capi, synth

pytestmark = pytest.mark.gpu

TissueScanError = _capi.TissueScanError
VARIANTS = {"u32": ((6, 10, 72), np.uint32, 4), "u16": ((5, 10, 72), np.uint16, 3)}      # dims, label type, seed
STATES = ("no_volume", "volume_set", "extracted", "enqueued", "settled", "extract_again", "relabel")
ROOM = 1 << 17                      # entries of room in every output column: more than these volumes have voxel faces

PROBES = ("junctions_size", "junctions_get_edges", "junctions_get_vertices", "junctions_debug", "junctions_timing",
          "components_size", "components_get", "components_image", "components_debug", "components_timing",
          "overlap_size", "overlap_get", "overlap_debug", "overlap_timing", "overlap_timing_compaction",
          "mesh_size", "mesh_get", "mesh_timing")
# the state "enqueued" asks the timings first: a size, a getter or a debug call would settle the tables
TIMINGS_FIRST = tuple(p for p in PROBES if "timing" in p) + tuple(p for p in PROBES if "timing" not in p)


def volume(variant, seed_offset=0):
    dims, dtype, seed = VARIANTS[variant]
    return synth.voronoi_labels(dims, 8, seed + seed_offset, dtype=np.uint16).astype(dtype)


def raw(ctx, name, *args):
    rc = getattr(ctx._lib, name)(ctx._h, *args)
    if rc != _capi.TA_OK:
        raise TissueScanError(rc, ctx._lib.ta_last_error().decode(errors="replace"))


def make_probes(voxels, planes):
    """{entry point: call}; every output has ROOM entries (the image: the whole buffer, one element for no volume)."""
    u32 = [np.zeros(4 * ROOM, dtype=np.uint32) for _ in range(4)]
    u64 = [np.zeros(3 * ROOM, dtype=np.uint64) for _ in range(3)]
    i32 = [np.zeros(6 * ROOM, dtype=np.int32) for _ in range(2)]
    image = np.zeros(max(voxels, 1), dtype=np.uint32)
    n = [ctypes.c_uint64(0) for _ in range(3)]
    ms = [ctypes.c_double(0.0) for _ in range(2)]
    words, passes = (ctypes.c_uint32 * 4)(), ctypes.c_int(0)
    p = lambda a: a.ctypes.data
    r = ctypes.byref
    return {
        "junctions_size": lambda c: raw(c, "ta_junctions_size", r(n[0]), r(n[1]), r(n[2])),
        "junctions_get_edges": lambda c: raw(c, "ta_junctions_get_edges", p(u32[0]), p(u64[0]), p(u64[1])),
        "junctions_get_vertices": lambda c: raw(c, "ta_junctions_get_vertices", p(u32[0]), p(u64[0]), p(u64[1])),
        "junctions_debug": lambda c: raw(c, "ta_junctions_debug", words),
        "junctions_timing": lambda c: raw(c, "ta_junctions_timing", r(ms[0]), r(ms[1])),
        "components_size": lambda c: raw(c, "ta_components_size", r(n[0])),
        "components_get": lambda c: raw(c, "ta_components_get", p(u32[0]), p(u64[0]), p(i32[0]), p(i32[1]), p(u64[1])),
        "components_image": lambda c: raw(c, "ta_components_image", 0, planes, p(image)),
        "components_debug": lambda c: raw(c, "ta_components_debug", words),
        "components_timing": lambda c: raw(c, "ta_components_timing", r(ms[0]), r(ms[1])),
        "overlap_size": lambda c: raw(c, "ta_overlap_size", r(n[0])),
        "overlap_get": lambda c: raw(c, "ta_overlap_get", p(u32[0]), p(u32[1]), p(u64[0])),
        "overlap_debug": lambda c: raw(c, "ta_overlap_debug", words),
        "overlap_timing": lambda c: raw(c, "ta_overlap_timing", r(ms[0])),
        "overlap_timing_compaction": lambda c: raw(c, "ta_overlap_timing_compaction", r(ms[0]), r(passes)),
        "mesh_size": lambda c: raw(c, "ta_mesh_size", r(n[0]), r(n[1]), r(n[2])),
        "mesh_get": lambda c: raw(c, "ta_mesh_get", p(u32[0]), p(u64[0]), p(u64[1]), p(u64[2]), p(u32[1]), p(u32[2]), p(u32[3])),
        "mesh_timing": lambda c: raw(c, "ta_mesh_timing", r(ms[0])),
    }


def ask(ctx, probes, order=PROBES):
    seen = {}
    for name in order:
        try:
            probes[name](ctx)
            seen[name] = (0, "")
        except TissueScanError as e:
            text = str(e)
            seen[name] = (e.code, text[text.index(": ") + 2:])
    return seen


def observe(variant, state):
    """{entry point: (code, message)} of one state, on a context of its own."""
    vol = volume(variant)
    probes = make_probes(0, 0) if state == "no_volume" else make_probes(vol.size, vol.shape[0])
    with _capi.Context(0) as ctx:
        if state != "no_volume":
            ctx.set_volume(vol)
        if state not in ("no_volume", "volume_set"):
            ctx.set_overlap(volume(variant, 1))
            ctx.extract(_capi.F_ALL, int(vol.max()))
        if state in ("enqueued", "settled", "extract_again", "relabel"):
            ctx.junctions_extract()
            ctx.components_extract()
            ctx.overlap_extract()
            raw(ctx, "ta_mesh_extract", 1, None)
        if state == "enqueued":
            return ask(ctx, probes, TIMINGS_FIRST)
        if state in ("extract_again", "relabel"):
            assert all(v == (0, "") for v in ask(ctx, probes).values())       # (every result fetched once: settled)
        if state == "extract_again":
            ctx.extract(_capi.F_ALL, int(vol.max()))
        if state == "relabel":
            lut = np.arange(int(vol.max()) + 1, dtype=np.uint32)
            lut[[2, 3]] = lut[[3, 2]]
            ctx.relabel(lut)
        return ask(ctx, probes)


# ---- the table, recorded on the commit before the change (see the module docstring); both label widths answered the same ------
# Read with the rules in mind: the junction, component and overlap tables are keyed by the volume (a second extraction leaves them
# alone, new label values end them), the mesh by the extraction.  The two-interval timings ask "settled" and say so; ta_mesh_timing
# and ta_overlap_timing ask "has a pass run": the mesh's still answers with the old pass's time after a second extraction and after
# a relabel, while its getters refuse.
OK = (0, "")
NO_JUNCTIONS = (-1, "no junction tables for the current volume (run ta_junctions_extract)")
JUNCTIONS_NOT_SETTLED = (-1, "no settled junction tables (ask ta_junctions_size first)")
NO_COMPONENTS = (-1, "no component tables for the current volume (run ta_components_extract)")
COMPONENTS_NOT_SETTLED = (-1, "no settled component tables (ask ta_components_size first)")
NO_OVERLAP = (-1, "no overlap table for the current volume and B (run ta_overlap_extract)")
NO_OVERLAP_PASS = (-1, "no overlap pass has been run")
OVERLAP_NOT_SETTLED = (-1, "no settled overlap table (ask ta_overlap_size first)")
NO_MESH = (-1, "no mesh of the current extraction (run ta_mesh_extract)")
NO_MESH_PASS = (-1, "no mesh pass has been run")

NOTHING = dict(
    junctions_size=NO_JUNCTIONS, junctions_get_edges=NO_JUNCTIONS, junctions_get_vertices=NO_JUNCTIONS, junctions_debug=NO_JUNCTIONS,
    junctions_timing=JUNCTIONS_NOT_SETTLED,
    components_size=NO_COMPONENTS, components_get=NO_COMPONENTS, components_image=NO_COMPONENTS, components_debug=NO_COMPONENTS,
    components_timing=COMPONENTS_NOT_SETTLED,
    overlap_size=NO_OVERLAP, overlap_get=NO_OVERLAP, overlap_debug=NO_OVERLAP, overlap_timing=NO_OVERLAP_PASS,
    overlap_timing_compaction=OVERLAP_NOT_SETTLED,
    mesh_size=NO_MESH, mesh_get=NO_MESH, mesh_timing=NO_MESH_PASS)
ALL_OK = dict((name, OK) for name in PROBES)
EXPECTED = {
    "no_volume": NOTHING,
    "volume_set": NOTHING,
    "extracted": NOTHING,
    "enqueued": dict(ALL_OK, junctions_timing=JUNCTIONS_NOT_SETTLED, components_timing=COMPONENTS_NOT_SETTLED,
                     overlap_timing_compaction=OVERLAP_NOT_SETTLED),
    "settled": ALL_OK,
    "extract_again": dict(ALL_OK, mesh_size=NO_MESH, mesh_get=NO_MESH),
    "relabel": dict(NOTHING, mesh_timing=OK),
}


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
def test_a_volume_of_one_label_gives_no_mesh_when_no_row_is_wanted_and_one_overlap_pair(dtype):
    """Zero records behind a count (the junction and component tables of this volume: their own limits files): the mesh of no row
    has no cell, vertex or triangle; the overlap with an equal B is the one pair (7, 7) of every voxel."""
    vol = np.full((4, 6, 72), 7, dtype=dtype)
    with _capi.Context(0) as ctx:
        ctx.set_volume(vol)
        ctx.set_overlap(vol.copy())
        ctx.extract(_capi.F_ALL, 7)
        cells, voff, toff, corners, triangles, tcell, tnb = ctx.mesh(1, wanted_rows=np.zeros(8, dtype=np.uint8))[:7]
        assert cells.size == corners.size == triangles.size == tcell.size == tnb.size == 0 and voff.tolist() == toff.tolist() == [0]
        ctx.overlap_extract()
        a, b, n = ctx.overlap_get()
        assert (a.tolist(), b.tolist(), n.tolist()) == ([7], [7], [vol.size])


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("state", STATES)
def test_what_every_entry_point_answers(variant, state):
    seen, want = observe(variant, state), EXPECTED[state]
    assert sorted(seen) == sorted(want) == sorted(PROBES)
    wrong = dict((k, (seen[k], want[k])) for k in want if seen[k] != want[k])
    assert not wrong, "(seen, recorded): %r" % wrong
