"""What becomes stale on a context, and when: every result a context can hold, crossed with everything that can invalidate it.

Each feature's own test file checks its own invalidation; this file pins the cross product, which is host logic only (the volumes
are tiny).  A scenario brings a fresh Context into a base state, fetches every result once (so it is settled), applies ONE cause
and then asks for every result again WITHOUT redoing its pass.  Each answer is classified as one of

    ("error", code, message)   a TissueScanError; the recorded text is a substring of its message
    "current"                  equal to the CPU reference (tests/*_reference.py, the oracle) of the volume as it is NOW
    "held"                     bit-equal to what was fetched before the cause (and not the current reference: where the cause
                               changed the voxels, a stale answer served without an error)
    ("wrong", digest)          neither, served without an error: "empty", or the first bytes of the sha1 of the answer
    ("value", v)               scalars that have no CPU reference (option values, is_compact)

and the classification of every (scenario, probe) cell must equal the literal table EXPECTED below.  The table was RECORDED on the
commit before the host layer got one invalidation path (a state struct per concern, volume_replaced / volume_labels_changed): it
states what the library did, not what it should do.  What looks wrong in it is named in the comment above the table and stays as
it is until a change sets out to fix it.  After every cause a fresh count, fetch and medians of the wall voxels must equal the reference of the
current labels (a staging buffer left with old records would show there).
"""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import components_reference
import junction_reference
import mesh_reference
import overlap_reference
import signal_reference
import wall_geometry_reference
from oracle import onepass_c
from tissue_analysis_amd import _capi, geometry, synth

from helpers import brute_wall_records

pytestmark = pytest.mark.gpu

DIMS, DIMS_W = (6, 10, 72), (5, 10, 72)
ID_STRIDE = 1000003                                    # the compacted scenarios hold label * ID_STRIDE
TissueScanError = _capi.TissueScanError


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def volume(name, dtype=np.uint32):
    """V: 10 labels (background 1 included), 11 components, edges and a vertex; V2 ("V'"): same dims, other labels; W: other dims;
    the sparse ones: the same with every label times ID_STRIDE."""
    if name.startswith("sparse_"):
        return frozen((volume(name[7:], np.uint32).astype(np.uint64) * ID_STRIDE).astype(np.uint32))
    dims, seed = {"V": (DIMS, 4), "V2": (DIMS, 5), "W": (DIMS_W, 3)}[name]
    return frozen(synth.voronoi_labels(dims, 8, seed, dtype=np.uint16).astype(dtype))


@functools.lru_cache(maxsize=None)
def image(name, dtype, seed):
    """A signal image (uint8) or a second label volume (uint16) of the dims of volume `name`."""
    rng = np.random.default_rng(seed)
    return frozen(rng.integers(0, 200 if dtype == np.uint8 else 7, size=volume(name).shape).astype(dtype))


def test_the_volumes_have_what_the_rules_are_about():
    V, V2 = volume("V"), volume("V2")
    assert V.shape == V2.shape == DIMS and volume("W").shape == DIMS_W and (V != V2).any()
    rows, _ = components_reference.table(V)
    (_, en, _), (_, vn, _), _ = junction_reference.tables(V)
    assert np.unique(V).size == 10 and rows[0].size == 11 and en.size == 10 and vn.size == 1
    assert brute_wall_records(V)[0].size > 1000 and int(volume("sparse_V").max()) == 10 * ID_STRIDE


# ---- the truth a scenario keeps beside the context: what the references are computed from --------------------------------------
class World(object):
    def __init__(self, vol, first_owned=0):
        self.vol, self.first_owned = np.array(vol), first_owned
        self.S = self.B = None
        self.ids = None                                # compacted: rank -> id
        self.mask = _capi.F_ALL
        self.keep = None                               # the torch tensor of an adopted volume

    def rows(self):
        """The row of every voxel, and the number of rows the next extraction should have."""
        if self.ids is None:
            return self.vol, int(self.vol.max()) + 1
        return np.searchsorted(self.ids, self.vol).astype(np.uint32), self.ids.size

    def max_label(self):
        return self.rows()[1] - 1


def sweep_reference(w):
    rows, n = w.rows()
    # (a halo plane lies one below the slab's origin, and only its faces with plane 1 count)
    return onepass_c.extract(rows.astype(w.vol.dtype), max_label=n - 1, origin=(-w.first_owned, 0, 0), own_first_plane=not w.first_owned)


def ref_labels(w):
    r = sweep_reference(w)
    sum2 = r["sum2"] if w.mask & _capi.F_MOMENT2 else np.zeros_like(r["sum2"])
    return r["count"], r["bbox"], r["sum1"], sum2


def ref_adjacency(w):
    r = sweep_reference(w)
    lo, hi = r["pair_lo"].astype(np.uint32), r["pair_hi"].astype(np.uint32)
    if w.ids is not None:
        lo, hi = w.ids[lo.astype(np.int64)], w.ids[hi.astype(np.int64)]
    return lo, hi, r["pair_faces"]


def canonical(lo, hi, coords):
    order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0], hi, lo))
    return lo[order], hi[order], coords[order]


def ref_walls(w):
    return brute_wall_records(w.vol)                   # (sorted by pair, then voxel: canonical() of itself)


def ref_medians(w):
    lo, hi, coords = brute_wall_records(w.vol)
    k = (lo.astype(np.uint64) << np.uint64(32)) | hi.astype(np.uint64)
    uk, count = np.unique(k, return_counts=True)
    med = geometry.median_voxels(coords.astype(np.int64), count).reshape(-1, 3).astype(np.int32)
    return uk, count.astype(np.uint32), med


def ref_signal_labels(w):
    if w.S is None:
        return None
    rows, n = w.rows()
    r = signal_reference.labels(w.vol, w.S, n, rows=rows, first_owned=w.first_owned)
    present = r["n"] > 0                               # (rows without voxels: the device's initial values)
    return (r["n"], r["sum"], np.stack([r["sumsq"], np.zeros_like(r["sumsq"])], axis=1),
            np.where(present, r["min"], 0xFFFFFFFF).astype(np.uint32), np.where(present, r["max"], 0).astype(np.uint32))


def ref_signal_walls(w):
    if w.S is None:
        return None
    r = signal_reference.walls(w.vol, w.S, first_owned=w.first_owned)
    return r["side_lo"], r["side_hi"]


def ref_wallgeo(w):
    r = wall_geometry_reference.rows(w.vol, first_owned=w.first_owned)
    return tuple(r[k] for k in ("fwd", "rev", "sum1", "sum2"))


def ref_mesh(w):
    rows, _ = w.rows()
    m = mesh_reference.mesh(rows)
    g = tuple(n + 1 for n in rows.shape)
    nb = np.where(m["triangle_neighbor"] == mesh_reference.OUTSIDE, _capi.MESH_OUTSIDE, m["triangle_neighbor"]).astype(np.uint32)
    return (m["labels"].astype(np.uint32), m["vertex_offsets"], m["triangle_offsets"],
            np.ravel_multi_index(tuple(m["corners"].T), g).astype(np.uint64), m["triangles"], m["triangle_cell"].astype(np.uint32), nb)


def ref_overlap(w):
    return None if w.B is None else overlap_reference.table(w.vol, w.B, first_owned=w.first_owned)


def ref_junctions(w):
    (el, en, es), (vl, vn, vs), deg = junction_reference.tables(w.vol, first_owned=w.first_owned)
    return el, en, es, vl, vn, vs, np.uint64(deg)


def ref_components(w):
    return components_reference.table(w.vol, first_owned=w.first_owned)[0]


def ref_components_image(w):
    return (components_reference.table(w.vol, first_owned=w.first_owned)[1].reshape(-1),)


def ref_census(w):
    ids = np.unique(w.vol).astype(np.uint32)
    return np.uint32(ids[-1]), ids


def ref_compact_ids(w):
    return (np.unique(w.vol).astype(np.uint32),)


# ---- the probes: one result each, asked for WITHOUT redoing its pass -----------------------------------------------------------
ROOM = 20 * int(np.prod(DIMS))                         # records of room for a raw fetch whose count the test does not know


def check(ctx, rc):
    if rc != _capi.TA_OK:
        raise TissueScanError(rc, ctx._lib.ta_last_error().decode(errors="replace"))


def get_walls(ctx, n):
    """ta_wall_voxels_get alone: no new count."""
    pairs, coords = np.zeros((ROOM, 2), dtype=np.uint32), np.zeros((ROOM, 3), dtype=np.int32)
    check(ctx, ctx._lib.ta_wall_voxels_get(ctx._h, pairs.ctypes.data, coords.ctypes.data, None))
    return canonical(pairs[:n, 0].copy(), pairs[:n, 1].copy(), coords[:n].copy())


def get_medians(ctx, E):
    """ta_wall_medians_get alone: no new ta_wall_medians."""
    pairs, sizes, med = np.zeros((ROOM, 2), dtype=np.uint32), np.zeros(ROOM, dtype=np.uint32), np.zeros((ROOM, 3), dtype=np.int32)
    check(ctx, ctx._lib.ta_wall_medians_get(ctx._h, pairs.ctypes.data, sizes.ctypes.data, med.ctypes.data))
    keys = (pairs[:E, 0].astype(np.uint64) << np.uint64(32)) | pairs[:E, 1].astype(np.uint64)
    return keys, sizes[:E].copy(), med[:E].copy()


def fresh_walls(ctx):
    lo, hi, coords, _ = ctx.wall_voxels()
    return canonical(lo, hi, coords)


def fresh_medians(ctx):
    keys, sizes, med, _, moving = ctx.wall_medians()
    assert not moving.any()
    return keys, sizes, med


def get_mesh(ctx):
    """ta_mesh_size + ta_mesh_get alone: no new ta_mesh_extract."""
    C, V, T = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(ctx, ctx._lib.ta_mesh_size(ctx._h, ctypes.byref(C), ctypes.byref(V), ctypes.byref(T)))
    C, V, T = C.value, V.value, T.value
    cells, voff, toff = np.zeros(C, dtype=np.uint32), np.zeros(C + 1, dtype=np.uint64), np.zeros(C + 1, dtype=np.uint64)
    corners, tri = np.zeros(V, dtype=np.uint64), np.zeros((T, 3), dtype=np.uint32)
    tcell, tnb = np.zeros(T, dtype=np.uint32), np.zeros(T, dtype=np.uint32)
    check(ctx, ctx._lib.ta_mesh_get(ctx._h, cells.ctypes.data, voff.ctypes.data, toff.ctypes.data, corners.ctypes.data,
                                    tri.ctypes.data, tcell.ctypes.data, tnb.ctypes.data))
    return cells, voff, toff, corners, tri, tcell, tnb


def get_junctions(ctx):
    (el, en, es), (vl, vn, vs), deg = ctx.junctions_get()
    return el, en, es, vl, vn, vs, np.uint64(deg)


# name -> (probe(ctx, held), reference(world) or None for a scalar)
PROBES = {
    "labels": (lambda c, h: c.labels(), ref_labels),
    "adjacency": (lambda c, h: c.adjacency(), ref_adjacency),
    "walls_get": (lambda c, h: get_walls(c, h["walls_n"]), ref_walls),
    "medians_get": (lambda c, h: get_medians(c, h["medians_n"]), ref_medians),
    "signal_labels": (lambda c, h: c.signal_labels(), ref_signal_labels),
    "signal_walls": (lambda c, h: c.signal_walls(), ref_signal_walls),
    "wallgeo": (lambda c, h: c.wallgeo_get(), ref_wallgeo),
    "mesh": (lambda c, h: get_mesh(c), ref_mesh),
    "overlap": (lambda c, h: c.overlap_get(), ref_overlap),
    "junctions": (lambda c, h: get_junctions(c), ref_junctions),
    "components": (lambda c, h: c.components_get(), ref_components),
    "components_image": (lambda c, h: (c.components_image(),), ref_components_image),
    "label_census": (lambda c, h: tuple(np.asarray(x) for x in c.label_census()), ref_census),
    "compact_ids": (lambda c, h: (c.compact_ids(),), ref_compact_ids),
    "is_compact": (lambda c, h: c.is_compact(), None),
    "shape_used": (lambda c, h: c.get_option(_capi.OPT_SWEEP_SHAPE_USED), None),
    "tile_planes": (lambda c, h: c.get_option(_capi.OPT_TILE_PLANES), None),
    # always last: a NEW count, fetch and medians (they replace what the raw fetches above would answer with)
    "fresh_walls": (lambda c, h: fresh_walls(c), ref_walls),
    "fresh_medians": (lambda c, h: fresh_medians(c), ref_medians),
}
# the sparse-id probes come after the results: ta_volume_label_census builds a census, which the probes before it must not see
ORDER = ("labels", "adjacency", "walls_get", "medians_get", "signal_labels", "signal_walls", "wallgeo", "mesh", "overlap", "junctions",
         "components", "components_image", "is_compact", "compact_ids", "shape_used", "tile_planes", "label_census", "fresh_walls",
         "fresh_medians")


def same(got, want):
    if want is None or len(got) != len(want):
        return False
    return all(np.asarray(g).shape == np.asarray(w).shape and np.array_equal(np.asarray(g).astype(np.asarray(w).dtype), w)
               and np.array_equal(g, np.asarray(w).astype(np.asarray(g).dtype)) for g, w in zip(got, want))


_MEMO = {}


def memo(reference, w):
    """reference(w), computed once per state of the world."""
    key = (reference.__name__, w.vol.dtype.str, w.vol.tobytes(), w.first_owned, w.ids is not None, id(w.S), id(w.B), w.mask)
    if key not in _MEMO:
        _MEMO[key] = reference(w)
    return _MEMO[key]


def digest(got):
    if all(np.asarray(g).size == 0 for g in got):
        return "empty"
    h = hashlib.sha1()
    for g in got:
        a = np.ascontiguousarray(g)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:12]


def ask(name, ctx, held, world):
    probe, reference = PROBES[name]
    try:
        got = probe(ctx, held)
    except TissueScanError as e:
        text = str(e)
        return ("error", e.code, text[text.index(": ") + 2:]), None
    if reference is None:
        return ("value", int(got)), got
    if same(got, memo(reference, world)):
        return "current", got
    if name in held and same(got, held[name]):
        return "held", got
    return ("wrong", digest(got)), got


# ---- base states ---------------------------------------------------------------------------------------------------------------
def new_signal(ctx, w, seed=11):
    w.S = image("W" if w.vol.shape == DIMS_W else "V", np.uint8, seed)
    ctx.set_signal(w.S)


def new_overlap(ctx, w, seed=12):
    w.B = image("W" if w.vol.shape == DIMS_W else "V", np.uint16, seed)
    ctx.set_overlap(w.B)


def adopt_slab(ctx, w):
    """The volume as a device slab whose plane 0 is a low halo plane, from a torch tensor."""
    import torch
    if w.keep is None:
        w.keep = torch.from_numpy(w.vol.view(np.int32)).to("cuda:0")
        torch.cuda.synchronize()
    ctx.set_volume_device(w.keep.data_ptr(), 4, w.vol.shape, a0_origin=0, has_low_halo=True, keep=w.keep)


def base_state(ctx, variant):
    if variant == "slab":
        w = World(volume("V"), first_owned=1)
        adopt_slab(ctx, w)
    elif variant == "compact":
        w = World(volume("sparse_V"))
        ctx.set_volume(w.vol)
        w.ids = ctx.compact_labels()
        assert np.array_equal(w.ids, np.unique(w.vol))
    else:
        w = World(volume("V", {"u32": np.uint32, "u16": np.uint16}[variant]))
        ctx.set_volume(w.vol)
    new_signal(ctx, w)
    new_overlap(ctx, w)
    return w


def run_passes(ctx, w):
    """Every pass once, every result fetched once: what the context holds before the cause.  A pass the base state cannot run
    (the wall voxels and the mesh of a slab with a halo plane) holds nothing."""
    held = {"walls_n": 0, "medians_n": 0}
    ctx.extract(w.mask, w.max_label())

    def keep(name, fn):
        try:
            held[name] = fn()
        except TissueScanError:
            pass

    keep("labels", ctx.labels)
    keep("adjacency", ctx.adjacency)
    keep("walls_get", lambda: fresh_walls(ctx))
    keep("medians_get", lambda: fresh_medians(ctx))
    held["walls_n"] = held["walls_get"][0].size if "walls_get" in held else 0
    held["medians_n"] = held["medians_get"][0].size if "medians_get" in held else 0
    ctx.signal_extract()
    keep("signal_labels", ctx.signal_labels)
    keep("signal_walls", ctx.signal_walls)
    ctx.wallgeo_extract()
    keep("wallgeo", ctx.wallgeo_get)
    keep("mesh", lambda: ctx.mesh(1)[:7])
    ctx.overlap_extract()
    keep("overlap", ctx.overlap_get)
    ctx.junctions_extract()
    keep("junctions", lambda: get_junctions(ctx))
    ctx.components_extract()
    keep("components", ctx.components_get)
    keep("components_image", lambda: (ctx.components_image(),))
    if w.ids is None:
        keep("label_census", lambda: tuple(np.asarray(x) for x in ctx.label_census()))
    else:
        keep("compact_ids", lambda: (ctx.compact_ids(),))
    return held


# ---- causes: each changes the context AND the world ----------------------------------------------------------------------------
def cause_set_volume_other_labels(ctx, w, held):
    w.vol = np.array(volume("sparse_V2" if w.ids is not None else "V2", w.vol.dtype))
    w.first_owned, w.ids, w.keep = 0, None, None
    ctx.set_volume(w.vol)


def cause_set_volume_other_dims(ctx, w, held):
    w.vol = np.array(volume("W", w.vol.dtype))
    w.first_owned, w.ids, w.keep, w.S, w.B = 0, None, None, None, None
    ctx.set_volume(w.vol)


def cause_set_volume_device_again(ctx, w, held):
    adopt_slab(ctx, w)


def relabel_table(w):
    n = w.ids.size if w.ids is not None else int(w.vol.max()) + 1
    lut = np.arange(n, dtype=np.uint32) if w.ids is None else w.ids.copy()
    lut[-1], lut[-2] = lut[-3], lut[-1]                # two labels fused, one renamed
    return lut


def cause_relabel(ctx, w, held):
    lut = relabel_table(w)
    rows, _ = w.rows()
    w.vol = lut[rows.astype(np.int64)].astype(w.vol.dtype)
    w.ids = None
    ctx.relabel(lut)


def cause_components_relabel(ctx, w, held):
    rows, image_ = components_reference.table(w.vol, first_owned=w.first_owned)
    new = rows[0].astype(np.uint32).copy()
    new[1::2] += 20                                    # every second component gets a label of its own
    w.vol = new[image_.astype(np.int64)].astype(w.vol.dtype)
    w.ids = None
    ctx.components_relabel(new)
    ctx.synchronize()


def cause_extract_again(ctx, w, held):
    ctx.extract(w.mask, w.max_label())


def cause_extract_without_adjacency(ctx, w, held):
    w.mask = 0x0f
    ctx.extract(w.mask, w.max_label())


def cause_compact_labels(ctx, w, held):
    w.ids = ctx.compact_labels()


def cause_uncompact(ctx, w, held):
    ctx.uncompact()
    w.ids = None


def cause_rerank(ctx, w, held):
    ctx.rerank()


def cause_set_sweep_shape(ctx, w, held):
    ctx.set_option(_capi.OPT_SWEEP_SHAPE, 1)


def cause_set_signal(ctx, w, held):
    new_signal(ctx, w, seed=21)


def cause_set_overlap(ctx, w, held):
    new_overlap(ctx, w, seed=22)


CAUSES = dict((f.__name__[6:], f) for f in (
    cause_set_volume_other_labels, cause_set_volume_other_dims, cause_set_volume_device_again, cause_relabel, cause_components_relabel,
    cause_extract_again, cause_extract_without_adjacency, cause_compact_labels, cause_uncompact, cause_rerank, cause_set_sweep_shape,
    cause_set_signal, cause_set_overlap))

SCENARIOS = (
    [("u32", c) for c in ("set_volume_other_labels", "set_volume_other_dims", "relabel", "components_relabel", "extract_again",
                          "extract_without_adjacency", "compact_labels", "uncompact", "set_sweep_shape", "set_signal", "set_overlap")] +
    [("u16", c) for c in ("set_volume_other_labels", "set_volume_other_dims", "relabel", "components_relabel", "set_sweep_shape")] +
    [("slab", c) for c in ("set_volume_device_again", "set_volume_other_labels", "extract_again", "extract_without_adjacency",
                           "set_signal")] +
    [("compact", c) for c in ("set_volume_other_labels", "relabel", "components_relabel", "extract_again", "compact_labels", "uncompact",
                              "rerank", "set_overlap")])


def observe(variant, cause):
    """{probe: outcome} of one scenario, on a context of its own."""
    ctx = _capi.Context(0)
    try:
        w = base_state(ctx, variant)
        held = run_passes(ctx, w)
        CAUSES[cause](ctx, w, held)
        seen = {}
        for name in ORDER:
            seen[name], _ = ask(name, ctx, held, w)
        extra = after_other_dims(ctx, w) if cause == "set_volume_other_dims" else None
    finally:
        ctx.close()
    return seen, extra


def after_other_dims(ctx, w):
    """The signal and the B volume of the old dims are gone: the passes say so, arrays of the old dims are refused, and after
    setting arrays of the new dims both passes answer with the reference of the new volume."""
    out = {}
    old_s, old_b = image("V", np.uint8, 11), image("V", np.uint16, 12)
    d, st8, st16 = _capi._i64x3(DIMS), _capi._i64x3(old_s.strides), _capi._i64x3(old_b.strides)
    ctx.extract(w.mask, w.max_label())
    for name, call in (("signal_extract", ctx.signal_extract), ("overlap_extract", ctx.overlap_extract),
                       ("signal_set_old_dims", lambda: check(ctx, ctx._lib.ta_signal_set(ctx._h, old_s.ctypes.data, 1, d, st8))),
                       ("overlap_set_old_dims", lambda: check(ctx, ctx._lib.ta_overlap_set(ctx._h, old_b.ctypes.data, 2, d, st16)))):
        try:
            call()
            out[name] = "ok"
        except TissueScanError as e:
            text = str(e)
            out[name] = ("error", e.code, text[text.index(": ") + 2:])
    with pytest.raises(ValueError):
        ctx.set_signal(old_s)                          # (the binding knows the label volume's shape too)
    with pytest.raises(ValueError):
        ctx.set_overlap(old_b)
    new_signal(ctx, w)
    new_overlap(ctx, w)
    ctx.signal_extract()
    ctx.overlap_extract()
    for name in ("signal_labels", "signal_walls", "overlap"):
        out[name + "_set_again"], _ = ask(name, ctx, {}, w)
    return out


# ---- the table, recorded on the commit before the change (see the module docstring) -------------------------------------------
# Read with the rules in mind: a new volume, a relabel and a components_relabel end everything; a second extraction ends what is keyed
# by the extraction (signal, wall geometry, mesh) and nothing keyed by the volume; compact / uncompact end the extraction only;
# ta_volume_rerank ends the junction and component tables but NOT the overlap table (!) nor the wall records (!): after an edit of an
# adopted buffer in place those two would be answered from the old voxels (here the voxels are unchanged, so they read "current").
# No cell of these scenarios is "held" or "wrong": nothing stale was served without an error.
EXPECTED = {('compact', 'compact_labels'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                 'compact_ids': 'current',
                                 'components': 'current',
                                 'components_image': 'current',
                                 'fresh_medians': 'current',
                                 'fresh_walls': 'current',
                                 'is_compact': ('value', 1),
                                 'junctions': 'current',
                                 'label_census': ('error', -1, 'the context is compacted: its census is the one it was compacted with'),
                                 'labels': ('error', -1, 'no extraction has been run on this context'),
                                 'medians_get': 'current',
                                 'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                 'overlap': 'current',
                                 'shape_used': ('value', 0),
                                 'signal_labels': ('error',
                                                   -1,
                                                   'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                 'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                                 'tile_planes': ('value', 32),
                                 'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                                 'walls_get': 'current'},
 ('compact', 'components_relabel'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                     'compact_ids': ('error', -1, 'the context is not compacted'),
                                     'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                     'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                     'fresh_medians': 'current',
                                     'fresh_walls': 'current',
                                     'is_compact': ('value', 0),
                                     'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                                     'label_census': 'current',
                                     'labels': ('error', -1, 'no extraction has been run on this context'),
                                     'medians_get': ('error', -1, 'call ta_wall_medians first'),
                                     'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                     'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                                     'shape_used': ('value', 0),
                                     'signal_labels': ('error',
                                                       -1,
                                                       'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                     'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                                     'tile_planes': ('value', 32),
                                     'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                                     'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('compact', 'extract_again'): {'adjacency': 'current',
                                'compact_ids': 'current',
                                'components': 'current',
                                'components_image': 'current',
                                'fresh_medians': 'current',
                                'fresh_walls': 'current',
                                'is_compact': ('value', 1),
                                'junctions': 'current',
                                'label_census': ('error', -1, 'the context is compacted: its census is the one it was compacted with'),
                                'labels': 'current',
                                'medians_get': 'current',
                                'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                'overlap': 'current',
                                'shape_used': ('value', 0),
                                'signal_labels': ('error',
                                                  -1,
                                                  'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                'signal_walls': ('error',
                                                 -1,
                                                 'no per-wall signal results for the current extraction (run ta_signal_extract with TA_SIG_WALLS)'),
                                'tile_planes': ('value', 32),
                                'wallgeo': ('error', -1, 'no wall-geometry rows for the current extraction (run ta_wallgeo_extract)'),
                                'walls_get': 'current'},
 ('compact', 'relabel'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                          'compact_ids': ('error', -1, 'the context is not compacted'),
                          'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                          'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                          'fresh_medians': 'current',
                          'fresh_walls': 'current',
                          'is_compact': ('value', 0),
                          'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                          'label_census': 'current',
                          'labels': ('error', -1, 'no extraction has been run on this context'),
                          'medians_get': ('error', -1, 'call ta_wall_medians first'),
                          'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                          'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                          'shape_used': ('value', 0),
                          'signal_labels': ('error', -1, 'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                          'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                          'tile_planes': ('value', 32),
                          'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                          'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('compact', 'rerank'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                         'compact_ids': 'current',
                         'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                         'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                         'fresh_medians': 'current',
                         'fresh_walls': 'current',
                         'is_compact': ('value', 1),
                         'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                         'label_census': ('error', -1, 'the context is compacted: its census is the one it was compacted with'),
                         'labels': ('error', -1, 'no extraction has been run on this context'),
                         'medians_get': 'current',
                         'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                         'overlap': 'current',
                         'shape_used': ('value', 0),
                         'signal_labels': ('error', -1, 'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                         'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                         'tile_planes': ('value', 32),
                         'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                         'walls_get': 'current'},
 ('compact', 'set_overlap'): {'adjacency': 'current',
                              'compact_ids': 'current',
                              'components': 'current',
                              'components_image': 'current',
                              'fresh_medians': 'current',
                              'fresh_walls': 'current',
                              'is_compact': ('value', 1),
                              'junctions': 'current',
                              'label_census': ('error', -1, 'the context is compacted: its census is the one it was compacted with'),
                              'labels': 'current',
                              'medians_get': 'current',
                              'mesh': 'current',
                              'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                              'shape_used': ('value', 0),
                              'signal_labels': 'current',
                              'signal_walls': 'current',
                              'tile_planes': ('value', 32),
                              'wallgeo': 'current',
                              'walls_get': 'current'},
 ('compact', 'set_volume_other_labels'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                          'compact_ids': ('error', -1, 'the context is not compacted'),
                                          'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                          'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                          'fresh_medians': 'current',
                                          'fresh_walls': 'current',
                                          'is_compact': ('value', 0),
                                          'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                                          'label_census': 'current',
                                          'labels': ('error', -1, 'no extraction has been run on this context'),
                                          'medians_get': ('error', -1, 'call ta_wall_medians first'),
                                          'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                          'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                                          'shape_used': ('value', 0),
                                          'signal_labels': ('error',
                                                            -1,
                                                            'no per-label signal results for the current extraction (run ta_signal_extract with '
                                                            'TA_SIG_LABELS)'),
                                          'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                                          'tile_planes': ('value', 32),
                                          'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                                          'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('compact', 'uncompact'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                            'compact_ids': ('error', -1, 'the context is not compacted'),
                            'components': 'current',
                            'components_image': 'current',
                            'fresh_medians': 'current',
                            'fresh_walls': 'current',
                            'is_compact': ('value', 0),
                            'junctions': 'current',
                            'label_census': 'current',
                            'labels': ('error', -1, 'no extraction has been run on this context'),
                            'medians_get': 'current',
                            'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                            'overlap': 'current',
                            'shape_used': ('value', 0),
                            'signal_labels': ('error', -1, 'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                            'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                            'tile_planes': ('value', 32),
                            'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                            'walls_get': 'current'},
 ('slab', 'extract_again'): {'adjacency': 'current',
                             'compact_ids': ('error', -1, 'the context is not compacted'),
                             'components': 'current',
                             'components_image': 'current',
                             'fresh_medians': ('error', -1, 'wall voxels are not available on a slab that carries a halo plane'),
                             'fresh_walls': ('error', -1, 'wall voxels are not available on a slab that carries a halo plane'),
                             'is_compact': ('value', 0),
                             'junctions': 'current',
                             'label_census': 'current',
                             'labels': 'current',
                             'medians_get': ('error', -1, 'call ta_wall_medians first'),
                             'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                             'overlap': 'current',
                             'shape_used': ('value', 0),
                             'signal_labels': ('error',
                                               -1,
                                               'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                             'signal_walls': ('error', -1, 'no per-wall signal results for the current extraction (run ta_signal_extract with TA_SIG_WALLS)'),
                             'tile_planes': ('value', 32),
                             'wallgeo': ('error', -1, 'no wall-geometry rows for the current extraction (run ta_wallgeo_extract)'),
                             'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('slab', 'extract_without_adjacency'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                         'compact_ids': ('error', -1, 'the context is not compacted'),
                                         'components': 'current',
                                         'components_image': 'current',
                                         'fresh_medians': ('error', -1, 'wall voxels are not available on a slab that carries a halo plane'),
                                         'fresh_walls': ('error', -1, 'wall voxels are not available on a slab that carries a halo plane'),
                                         'is_compact': ('value', 0),
                                         'junctions': 'current',
                                         'label_census': 'current',
                                         'labels': 'current',
                                         'medians_get': ('error', -1, 'call ta_wall_medians first'),
                                         'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                         'overlap': 'current',
                                         'shape_used': ('value', 0),
                                         'signal_labels': ('error',
                                                           -1,
                                                           'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                         'signal_walls': ('error',
                                                          -1,
                                                          'no per-wall signal results for the current extraction (run ta_signal_extract with TA_SIG_WALLS)'),
                                         'tile_planes': ('value', 16),
                                         'wallgeo': ('error', -1, 'no wall-geometry rows for the current extraction (run ta_wallgeo_extract)'),
                                         'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('slab', 'set_signal'): {'adjacency': 'current',
                          'compact_ids': ('error', -1, 'the context is not compacted'),
                          'components': 'current',
                          'components_image': 'current',
                          'fresh_medians': ('error', -1, 'wall voxels are not available on a slab that carries a halo plane'),
                          'fresh_walls': ('error', -1, 'wall voxels are not available on a slab that carries a halo plane'),
                          'is_compact': ('value', 0),
                          'junctions': 'current',
                          'label_census': 'current',
                          'labels': 'current',
                          'medians_get': ('error', -1, 'call ta_wall_medians first'),
                          'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                          'overlap': 'current',
                          'shape_used': ('value', 0),
                          'signal_labels': ('error', -1, 'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                          'signal_walls': ('error', -1, 'no per-wall signal results for the current extraction (run ta_signal_extract with TA_SIG_WALLS)'),
                          'tile_planes': ('value', 32),
                          'wallgeo': 'current',
                          'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('slab', 'set_volume_device_again'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                       'compact_ids': ('error', -1, 'the context is not compacted'),
                                       'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                       'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                       'fresh_medians': ('error', -1, 'wall voxels are not available on a slab that carries a halo plane'),
                                       'fresh_walls': ('error', -1, 'wall voxels are not available on a slab that carries a halo plane'),
                                       'is_compact': ('value', 0),
                                       'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                                       'label_census': 'current',
                                       'labels': ('error', -1, 'no extraction has been run on this context'),
                                       'medians_get': ('error', -1, 'call ta_wall_medians first'),
                                       'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                       'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                                       'shape_used': ('value', 0),
                                       'signal_labels': ('error',
                                                         -1,
                                                         'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                       'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                                       'tile_planes': ('value', 32),
                                       'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                                       'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('slab', 'set_volume_other_labels'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                       'compact_ids': ('error', -1, 'the context is not compacted'),
                                       'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                       'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                       'fresh_medians': 'current',
                                       'fresh_walls': 'current',
                                       'is_compact': ('value', 0),
                                       'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                                       'label_census': 'current',
                                       'labels': ('error', -1, 'no extraction has been run on this context'),
                                       'medians_get': ('error', -1, 'call ta_wall_medians first'),
                                       'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                       'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                                       'shape_used': ('value', 0),
                                       'signal_labels': ('error',
                                                         -1,
                                                         'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                       'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                                       'tile_planes': ('value', 32),
                                       'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                                       'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('u16', 'components_relabel'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                 'compact_ids': ('error', -1, 'the context is not compacted'),
                                 'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                 'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                 'fresh_medians': 'current',
                                 'fresh_walls': 'current',
                                 'is_compact': ('value', 0),
                                 'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                                 'label_census': 'current',
                                 'labels': ('error', -1, 'no extraction has been run on this context'),
                                 'medians_get': ('error', -1, 'call ta_wall_medians first'),
                                 'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                 'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                                 'shape_used': ('value', 0),
                                 'signal_labels': ('error',
                                                   -1,
                                                   'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                 'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                                 'tile_planes': ('value', 28),
                                 'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                                 'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('u16', 'relabel'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                      'compact_ids': ('error', -1, 'the context is not compacted'),
                      'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                      'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                      'fresh_medians': 'current',
                      'fresh_walls': 'current',
                      'is_compact': ('value', 0),
                      'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                      'label_census': 'current',
                      'labels': ('error', -1, 'no extraction has been run on this context'),
                      'medians_get': ('error', -1, 'call ta_wall_medians first'),
                      'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                      'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                      'shape_used': ('value', 0),
                      'signal_labels': ('error', -1, 'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                      'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                      'tile_planes': ('value', 28),
                      'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                      'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('u16', 'set_sweep_shape'): {'adjacency': 'current',
                              'compact_ids': ('error', -1, 'the context is not compacted'),
                              'components': 'current',
                              'components_image': 'current',
                              'fresh_medians': 'current',
                              'fresh_walls': 'current',
                              'is_compact': ('value', 0),
                              'junctions': 'current',
                              'label_census': 'current',
                              'labels': 'current',
                              'medians_get': 'current',
                              'mesh': 'current',
                              'overlap': 'current',
                              'shape_used': ('value', 0),
                              'signal_labels': 'current',
                              'signal_walls': 'current',
                              'tile_planes': ('value', 28),
                              'wallgeo': 'current',
                              'walls_get': 'current'},
 ('u16', 'set_volume_other_dims'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                    'compact_ids': ('error', -1, 'the context is not compacted'),
                                    'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                    'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                    'fresh_medians': 'current',
                                    'fresh_walls': 'current',
                                    'is_compact': ('value', 0),
                                    'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                                    'label_census': 'current',
                                    'labels': ('error', -1, 'no extraction has been run on this context'),
                                    'medians_get': ('error', -1, 'call ta_wall_medians first'),
                                    'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                    'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                                    'shape_used': ('value', 0),
                                    'signal_labels': ('error',
                                                      -1,
                                                      'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                    'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                                    'tile_planes': ('value', 28),
                                    'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                                    'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('u16', 'set_volume_other_labels'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                      'compact_ids': ('error', -1, 'the context is not compacted'),
                                      'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                      'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                      'fresh_medians': 'current',
                                      'fresh_walls': 'current',
                                      'is_compact': ('value', 0),
                                      'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                                      'label_census': 'current',
                                      'labels': ('error', -1, 'no extraction has been run on this context'),
                                      'medians_get': ('error', -1, 'call ta_wall_medians first'),
                                      'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                      'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                                      'shape_used': ('value', 0),
                                      'signal_labels': ('error',
                                                        -1,
                                                        'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                      'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                                      'tile_planes': ('value', 28),
                                      'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                                      'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('u32', 'compact_labels'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                             'compact_ids': 'current',
                             'components': 'current',
                             'components_image': 'current',
                             'fresh_medians': 'current',
                             'fresh_walls': 'current',
                             'is_compact': ('value', 1),
                             'junctions': 'current',
                             'label_census': ('error', -1, 'the context is compacted: its census is the one it was compacted with'),
                             'labels': ('error', -1, 'no extraction has been run on this context'),
                             'medians_get': 'current',
                             'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                             'overlap': 'current',
                             'shape_used': ('value', 0),
                             'signal_labels': ('error',
                                               -1,
                                               'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                             'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                             'tile_planes': ('value', 32),
                             'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                             'walls_get': 'current'},
 ('u32', 'components_relabel'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                 'compact_ids': ('error', -1, 'the context is not compacted'),
                                 'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                 'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                 'fresh_medians': 'current',
                                 'fresh_walls': 'current',
                                 'is_compact': ('value', 0),
                                 'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                                 'label_census': 'current',
                                 'labels': ('error', -1, 'no extraction has been run on this context'),
                                 'medians_get': ('error', -1, 'call ta_wall_medians first'),
                                 'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                 'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                                 'shape_used': ('value', 0),
                                 'signal_labels': ('error',
                                                   -1,
                                                   'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                 'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                                 'tile_planes': ('value', 32),
                                 'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                                 'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('u32', 'extract_again'): {'adjacency': 'current',
                            'compact_ids': ('error', -1, 'the context is not compacted'),
                            'components': 'current',
                            'components_image': 'current',
                            'fresh_medians': 'current',
                            'fresh_walls': 'current',
                            'is_compact': ('value', 0),
                            'junctions': 'current',
                            'label_census': 'current',
                            'labels': 'current',
                            'medians_get': 'current',
                            'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                            'overlap': 'current',
                            'shape_used': ('value', 0),
                            'signal_labels': ('error', -1, 'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                            'signal_walls': ('error', -1, 'no per-wall signal results for the current extraction (run ta_signal_extract with TA_SIG_WALLS)'),
                            'tile_planes': ('value', 32),
                            'wallgeo': ('error', -1, 'no wall-geometry rows for the current extraction (run ta_wallgeo_extract)'),
                            'walls_get': 'current'},
 ('u32', 'extract_without_adjacency'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                        'compact_ids': ('error', -1, 'the context is not compacted'),
                                        'components': 'current',
                                        'components_image': 'current',
                                        'fresh_medians': 'current',
                                        'fresh_walls': 'current',
                                        'is_compact': ('value', 0),
                                        'junctions': 'current',
                                        'label_census': 'current',
                                        'labels': 'current',
                                        'medians_get': 'current',
                                        'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                        'overlap': 'current',
                                        'shape_used': ('value', 0),
                                        'signal_labels': ('error',
                                                          -1,
                                                          'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                        'signal_walls': ('error',
                                                         -1,
                                                         'no per-wall signal results for the current extraction (run ta_signal_extract with TA_SIG_WALLS)'),
                                        'tile_planes': ('value', 16),
                                        'wallgeo': ('error', -1, 'no wall-geometry rows for the current extraction (run ta_wallgeo_extract)'),
                                        'walls_get': 'current'},
 ('u32', 'relabel'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                      'compact_ids': ('error', -1, 'the context is not compacted'),
                      'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                      'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                      'fresh_medians': 'current',
                      'fresh_walls': 'current',
                      'is_compact': ('value', 0),
                      'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                      'label_census': 'current',
                      'labels': ('error', -1, 'no extraction has been run on this context'),
                      'medians_get': ('error', -1, 'call ta_wall_medians first'),
                      'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                      'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                      'shape_used': ('value', 0),
                      'signal_labels': ('error', -1, 'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                      'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                      'tile_planes': ('value', 32),
                      'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                      'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('u32', 'set_overlap'): {'adjacency': 'current',
                          'compact_ids': ('error', -1, 'the context is not compacted'),
                          'components': 'current',
                          'components_image': 'current',
                          'fresh_medians': 'current',
                          'fresh_walls': 'current',
                          'is_compact': ('value', 0),
                          'junctions': 'current',
                          'label_census': 'current',
                          'labels': 'current',
                          'medians_get': 'current',
                          'mesh': 'current',
                          'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                          'shape_used': ('value', 0),
                          'signal_labels': 'current',
                          'signal_walls': 'current',
                          'tile_planes': ('value', 32),
                          'wallgeo': 'current',
                          'walls_get': 'current'},
 ('u32', 'set_signal'): {'adjacency': 'current',
                         'compact_ids': ('error', -1, 'the context is not compacted'),
                         'components': 'current',
                         'components_image': 'current',
                         'fresh_medians': 'current',
                         'fresh_walls': 'current',
                         'is_compact': ('value', 0),
                         'junctions': 'current',
                         'label_census': 'current',
                         'labels': 'current',
                         'medians_get': 'current',
                         'mesh': 'current',
                         'overlap': 'current',
                         'shape_used': ('value', 0),
                         'signal_labels': ('error', -1, 'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                         'signal_walls': ('error', -1, 'no per-wall signal results for the current extraction (run ta_signal_extract with TA_SIG_WALLS)'),
                         'tile_planes': ('value', 32),
                         'wallgeo': 'current',
                         'walls_get': 'current'},
 ('u32', 'set_sweep_shape'): {'adjacency': 'current',
                              'compact_ids': ('error', -1, 'the context is not compacted'),
                              'components': 'current',
                              'components_image': 'current',
                              'fresh_medians': 'current',
                              'fresh_walls': 'current',
                              'is_compact': ('value', 0),
                              'junctions': 'current',
                              'label_census': 'current',
                              'labels': 'current',
                              'medians_get': 'current',
                              'mesh': 'current',
                              'overlap': 'current',
                              'shape_used': ('value', 0),
                              'signal_labels': 'current',
                              'signal_walls': 'current',
                              'tile_planes': ('value', 32),
                              'wallgeo': 'current',
                              'walls_get': 'current'},
 ('u32', 'set_volume_other_dims'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                    'compact_ids': ('error', -1, 'the context is not compacted'),
                                    'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                    'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                    'fresh_medians': 'current',
                                    'fresh_walls': 'current',
                                    'is_compact': ('value', 0),
                                    'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                                    'label_census': 'current',
                                    'labels': ('error', -1, 'no extraction has been run on this context'),
                                    'medians_get': ('error', -1, 'call ta_wall_medians first'),
                                    'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                    'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                                    'shape_used': ('value', 0),
                                    'signal_labels': ('error',
                                                      -1,
                                                      'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                    'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                                    'tile_planes': ('value', 32),
                                    'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                                    'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('u32', 'set_volume_other_labels'): {'adjacency': ('error', -1, 'no extraction with adjacency has been run on this context'),
                                      'compact_ids': ('error', -1, 'the context is not compacted'),
                                      'components': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                      'components_image': ('error', -1, 'no component tables for the current volume (run ta_components_extract)'),
                                      'fresh_medians': 'current',
                                      'fresh_walls': 'current',
                                      'is_compact': ('value', 0),
                                      'junctions': ('error', -1, 'no junction tables for the current volume (run ta_junctions_extract)'),
                                      'label_census': 'current',
                                      'labels': ('error', -1, 'no extraction has been run on this context'),
                                      'medians_get': ('error', -1, 'call ta_wall_medians first'),
                                      'mesh': ('error', -1, 'no mesh of the current extraction (run ta_mesh_extract)'),
                                      'overlap': ('error', -1, 'no overlap table for the current volume and B (run ta_overlap_extract)'),
                                      'shape_used': ('value', 0),
                                      'signal_labels': ('error',
                                                        -1,
                                                        'no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)'),
                                      'signal_walls': ('error', -1, 'no extraction has been run on this context'),
                                      'tile_planes': ('value', 32),
                                      'wallgeo': ('error', -1, 'no extraction has been run on this context'),
                                      'walls_get': ('error', -1, 'call ta_wall_voxels_count first')},
 ('u32', 'uncompact'): {'adjacency': 'current',
                        'compact_ids': ('error', -1, 'the context is not compacted'),
                        'components': 'current',
                        'components_image': 'current',
                        'fresh_medians': 'current',
                        'fresh_walls': 'current',
                        'is_compact': ('value', 0),
                        'junctions': 'current',
                        'label_census': 'current',
                        'labels': 'current',
                        'medians_get': 'current',
                        'mesh': 'current',
                        'overlap': 'current',
                        'shape_used': ('value', 0),
                        'signal_labels': 'current',
                        'signal_walls': 'current',
                        'tile_planes': ('value', 32),
                        'wallgeo': 'current',
                        'walls_get': 'current'}}

EXPECTED_AFTER_OTHER_DIMS = {'u16': {'overlap_extract': ('error', -1, 'no second label volume set (ta_overlap_set)'),
         'overlap_set_again': 'current',
         'overlap_set_old_dims': ('error', -1, "B: dims (6, 10, 72) differ from the label volume's (5, 10, 72)"),
         'signal_extract': ('error', -1, 'no signal set'),
         'signal_labels_set_again': 'current',
         'signal_set_old_dims': ('error', -1, "the signal: dims (6, 10, 72) differ from the label volume's (5, 10, 72)"),
         'signal_walls_set_again': 'current'},
 'u32': {'overlap_extract': ('error', -1, 'no second label volume set (ta_overlap_set)'),
         'overlap_set_again': 'current',
         'overlap_set_old_dims': ('error', -1, "B: dims (6, 10, 72) differ from the label volume's (5, 10, 72)"),
         'signal_extract': ('error', -1, 'no signal set'),
         'signal_labels_set_again': 'current',
         'signal_set_old_dims': ('error', -1, "the signal: dims (6, 10, 72) differ from the label volume's (5, 10, 72)"),
         'signal_walls_set_again': 'current'}}


@pytest.mark.parametrize("variant,cause", SCENARIOS, ids=["%s-%s" % s for s in SCENARIOS])
def test_what_is_stale_after(variant, cause):
    seen, extra = observe(variant, cause)
    want = EXPECTED[(variant, cause)]
    assert sorted(seen) == sorted(want)
    wrong = dict((k, (seen[k], want[k])) for k in want if not matches(seen[k], want[k]))
    assert not wrong, "(seen, recorded): %r" % wrong
    if extra is not None:
        want = EXPECTED_AFTER_OTHER_DIMS[variant]
        wrong = dict((k, (extra.get(k), want[k])) for k in want if not matches(extra.get(k), want[k]))
        assert not wrong and sorted(extra) == sorted(want), "(seen, recorded): %r" % wrong
    if cause in ("set_volume_other_labels", "relabel", "components_relabel") and variant != "slab":
        assert seen["fresh_walls"] == "current" and seen["fresh_medians"] == "current"


def matches(seen, want):
    if isinstance(want, tuple) and want[0] == "error":
        return isinstance(seen, tuple) and seen[:2] == want[:2] and want[2] in seen[2]
    return seen == want
