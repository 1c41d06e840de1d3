"""Every feature pass on the seeded random volumes of tests/random_cases.py, enqueued back to back on ONE context in an order
drawn per case, fetched afterwards in another drawn order, and compared bit for bit with the CPU references of the features' own
test files (random_cases.references).

What the per-feature files do not do, and this one does: the variables are drawn together (label and signal type, C / F /
transposed layout, whole strips or ragged rows, uploaded / adopted / adopted off a 16-byte boundary, dense or compacted ids, whole
volume or slab with a halo, tile heights, the options of every pass); all passes share one context, stream, extraction, signal
companion and distance image with no fetch and no synchronisation between them; and in test_cases_on_one_reused_context a
context that held a larger volume serves the next five cases out of buffers full of the previous case's bytes.

The only order among the passes is the documented one (random_cases.pass_order).  A pass is left out of a case only where the
library documents a refusal -- on a slab the distance map, the profile, the order statistics, the mesh and the wall voxels; the
wall medians of a volume that is not C-ordered -- and there the documented error code is asserted instead."""
import numpy as np
import pytest

import random_cases as rc
from feature_passes import code
from helpers import assert_same_accumulators
from oracle import sia_oracle
from test_gpu_cell_meshes import assert_identical, assert_same_sets, context_meshes
from test_gpu_components import same_rows
from test_gpu_junctions import check_tables
from test_gpu_profile import same as same_profile
from test_gpu_wall_geometry import check_rows
from test_voxel_layers_cpu import brute_layer18
from tissue_analysis_amd import DICT, SpatialImage, SpatialImageAnalysis, _capi, hollow_out_cells

pytestmark = pytest.mark.gpu

CASES = rc.cases()
TORCH_VIEW = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
PAD = 32                                               # elements in front of an adopted volume (a multiple of 16 bytes for every type) and behind it


def absent_value(a):
    """The smallest value the array does not hold: what the pads around an adopted buffer hold, so that a load that strays into them
    shows as a label the references do not know.  (A uint8 signal that holds all 256 values: 0.)"""
    present = np.unique(a)
    gaps = np.flatnonzero(present != np.arange(present.size))
    return int(gaps[0]) if gaps.size else int(present.size) % (int(np.iinfo(a.dtype).max) + 1)


class Adopted(object):
    """The C-ordered array `a` on the device, `off` elements behind a 256-byte boundary, between two pads."""

    def __init__(self, a, off):
        import torch
        self.a, self.off, self.pad = a, PAD + off, absent_value(a)
        host = np.full(self.off + a.size + PAD, self.pad, dtype=a.dtype)
        host[self.off:self.off + a.size] = a.reshape(-1)
        self.host = host
        self.flat = torch.from_numpy(host.view(TORCH_VIEW[a.dtype]).copy()).to("cuda:0")
        torch.cuda.synchronize()
        self.ptr = int(self.flat.data_ptr()) + self.off * a.dtype.itemsize
        assert int(self.flat.data_ptr()) % 256 == 0 and self.ptr % 16 == (off * a.dtype.itemsize) % 16

    def unchanged(self):
        import torch
        torch.cuda.synchronize()
        return np.array_equal(self.flat.cpu().numpy().view(self.a.dtype), self.host)


def in_axes(c, flat):
    """A flat image in memory order (ta_distance_image, ta_components_image) with the axes of the volume."""
    return flat.reshape(rc.memory_dims(c)).transpose(np.argsort(rc.memory_order(c)))


# ---- the runner ------------------------------------------------------------------------------------------------------------------
def load(ctx, c):
    """Bring the context into the case's mode: options, volume, signal, second volume.  Returns the adopted buffers."""
    V, S, B = rc.volume(c), rc.signal(c), rc.second(c)
    ctx.set_option(_capi.OPT_TILE_PLANES, c.tile_planes)
    ctx.set_option(_capi.OPT_SWEEP_SHAPE, c.sweep_shape)
    held = []
    if c.mode in ("adopt", "adopt_offset", "slab"):
        v, s, b = Adopted(V, c.label_off), Adopted(S, c.signal_off), Adopted(B, c.second_off)
        ctx.set_volume_device(v.ptr, V.dtype.itemsize, V.shape, a0_origin=c.origin, has_low_halo=c.mode == "slab", keep=v.flat)
        assert ctx.get_option(_capi.OPT_VOLUME_SLACK) == 0, c.name
        ctx.set_signal_device(s.ptr, S.dtype.itemsize, keep=s.flat)
        ctx.set_overlap_device(b.ptr, B.dtype.itemsize, keep=b.flat)
        held = [v, s, b]
    else:
        ctx.set_volume(rc.in_layout(c, V))
        if rc.compacted(c):
            assert np.array_equal(ctx.compact_labels(), rc.row_image(c)[2]), c.name
        ctx.set_signal(rc.in_layout(c, S))
        ctx.set_overlap(rc.in_layout(c, B))
    assert ctx.is_compact() == rc.compacted(c), c.name
    return held


def enqueue(ctx, c, what):
    flags = _capi.DIST_EDGE_IS_SITE if c.edge_is_site else 0
    calls = dict(signal=lambda: ctx.signal_extract(_capi.SIG_LABELS | _capi.SIG_WALLS), wallgeo=ctx.wallgeo_extract,
                 overlap=ctx.overlap_extract, junctions=ctx.junctions_extract, components=ctx.components_extract,
                 distance=lambda: ctx.distance_extract(c.dist_mode, rc.site_label(c), c.spacing, flags),
                 profile=lambda: ctx.profile_extract(rc.edges2(c), c.prof_signal),
                 sighist=lambda: ctx.sighist_extract(c.log2_width),
                 sigrank=lambda: ctx.sigrank_extract(rc.ranks(c)))
    if rc.runs(c, what):
        calls[what]()
    else:                                              # INTEGRATION.md sections 18, 19, 20: a slab is refused
        assert code(calls[what]) == _capi.TA_EINVAL, (c.name, what)


def fetch(ctx, c, what, ref):
    """One result against its reference.  Every assertion names the case."""
    V, name = rc.volume(c), (c.name, what)
    if what == "labels":
        count, bbox, sum1, sum2 = ctx.labels()
        got = dict(ref["sweep"], count=count, bbox=bbox, sum1=sum1, sum2=sum2)
        assert_same_accumulators(got, ref["sweep"], c.name)
    elif what == "adjacency":
        lo, hi, faces = ctx.adjacency()
        got = dict(ref["sweep"], pair_lo=lo, pair_hi=hi, pair_faces=faces)
        assert_same_accumulators(got, ref["sweep"], c.name)
    elif what == "signal":
        r, w = ref["signal_labels"], ref["signal_walls"]
        n, s, q, mn, mx = ctx.signal_labels()
        assert np.array_equal(n, r["n"]) and np.array_equal(s, r["sum"]), name
        assert np.array_equal(q[:, 0], r["sumsq"]) and not q[:, 1].any(), name
        assert np.array_equal(mn, r["min"]) and np.array_equal(mx, r["max"]), name       # (absent rows: UINT32_MAX and 0 on both sides)
        slo, shi = ctx.signal_walls()
        assert np.array_equal(slo, w["side_lo"]) and np.array_equal(shi, w["side_hi"]), name
    elif what == "wallgeo":
        lo, hi, faces = ctx.adjacency()
        check_rows((lo, hi) + ctx.wallgeo_get(), ref["wallgeo"], faces)
    elif what == "overlap":
        a, b, n = ctx.overlap_get()
        want = ref["overlap"]
        assert np.array_equal(a.astype(np.int64), want[0]) and np.array_equal(b.astype(np.int64), want[1]), name
        assert np.array_equal(n, want[2]) and int(n.sum()) == V[rc.first_owned(c):].size, name
    elif what == "junctions":
        check_tables(ctx.junctions_get(), ref["junctions"])
    elif what == "components":
        rows, image = ref["components"]
        same_rows(ctx.components_get(), rows)
        assert np.array_equal(in_axes(c, ctx.components_image()), image), name
    elif what == "distance":
        if not rc.runs(c, what):
            assert code(ctx.distance_get) == _capi.TA_EINVAL and code(ctx.distance_image) == _capi.TA_EINVAL, name
            return
        assert np.array_equal(in_axes(c, ctx.distance_image()), ref["d2"]), name
        for g, w in zip(ctx.distance_get(), ref["distance"]):
            assert g.shape == w.shape and np.array_equal(g, w), name
    elif what == "profile":
        if not rc.runs(c, what):
            assert code(ctx.profile_get) == _capi.TA_EINVAL, name
            return
        same_profile(ctx.profile_get(), ref["profile"])
    elif what == "sighist":
        got = ctx.sighist_get()
        assert got.shape == ref["sighist"].shape and np.array_equal(got, ref["sighist"]), name
    elif what == "sigrank":
        if not rc.runs(c, what):
            assert code(ctx.sigrank_get) == _capi.TA_EINVAL, name
            return
        got = ctx.sigrank_get()
        assert got.shape == ref["sigrank"].shape and np.array_equal(got, ref["sigrank"]), name
    elif what == "mesh":
        if not rc.runs(c, what):                       # a slab adopted with a halo answers TA_EINVAL
            assert code(ctx.mesh) == _capi.TA_EINVAL, name
            return
        got = context_meshes(ctx, ids=ref["ids"])
        (assert_identical if rc.c_ordered(c) else assert_same_sets)(got, ref["mesh"])
    elif what == "walls":
        if not rc.whole(c):
            assert code(ctx.wall_voxels) == _capi.TA_EINVAL, name
            return
        if not rc.runs(c, what):                       # (more voxels than the brute-force reference is for)
            return
        lo, hi, coords, _ = ctx.wall_voxels()
        order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0], hi, lo))
        for g, w in zip((lo[order], hi[order], coords[order]), ref["walls"]):
            assert g.shape == w.shape and np.array_equal(g, w), name
        if not rc.c_ordered(c):                        # refused in the C entry point too
            assert code(ctx.wall_medians) == _capi.TA_EINVAL, name
            return
        for g, w in zip(ctx.wall_voxels(by_pair=True)[:3], ref["walls"]):
            assert g.shape == w.shape and np.array_equal(g, w), name
        keys, sizes, med, _, moving = ctx.wall_medians()
        wkeys, wsizes, wmed, wmoving = ref["medians"]
        assert np.array_equal(keys, wkeys) and np.array_equal(sizes, wsizes) and np.array_equal(moving, wmoving), name
        assert np.array_equal(med[~moving], wmed[~moving]), name
    else:
        raise KeyError(what)


def run_case(ctx, c):
    print("case", c.name)                              # (shown with a failure: which case of a chain it was)
    ref = rc.references(c.index)                       # (memoised: the two tests pay for them once)
    held = load(ctx, c)
    ctx.extract(_capi.F_ALL, ref["nrows"] - 1)
    for what in rc.pass_order(c.index):                # back to back: no fetch, no synchronize
        enqueue(ctx, c, what)
    for what in rc.fetch_order(c.index):
        fetch(ctx, c, what, ref)
    for buf in held:
        assert buf.unchanged(), c.name


# ---- the tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_on_a_fresh_context(c):
    with _capi.Context(0) as ctx:
        run_case(ctx, c)


@pytest.mark.parametrize("chain", rc.chains(), ids=["-".join("%02d" % i for i in ch) for ch in rc.chains()])
def test_cases_on_one_reused_context(chain):
    """Six cases on one context that is never closed in between: the largest first, so that every later one runs in buffers a
    bigger one left; the volume changes type, dims, layout and mode on the way, compaction begins and ends."""
    assert min(rc.transitions(chain)) >= 1
    with _capi.Context(0) as ctx:
        for i in chain:
            run_case(ctx, rc.case(i))


WHOLE = [c for c in CASES if rc.whole(c)]


@pytest.mark.parametrize("c", WHOLE, ids=[c.name for c in WHOLE])
def test_stencils_on_random_cases(c):
    """hollow_out_cells and the 18-neighbour layer of the whole-volume cases, in the case's memory layout, through the entry points
    of test_gpu_voxel_layers.py."""
    assert len(WHOLE) == 40
    vol = rc.in_layout(c, rc.volume(c))
    present, absent = int(rc.volume(c).reshape(-1)[0]), absent_value(rc.volume(c))
    for bg, remove in ((present, True), (present, False), (absent, True), (absent, False), (None, True), (None, False)):
        got = hollow_out_cells(SpatialImage(vol, voxelsize=(1., 1., 1.)), bg, remove_background=remove, verbose=False)
        want = sia_oracle.hollow_out_cells(vol, bg, remove_background=remove)
        assert np.asarray(got).dtype == vol.dtype and np.array_equal(np.asarray(got), want), (c.name, bg, remove)
    sia = SpatialImageAnalysis(SpatialImage(vol, voxelsize=(1., 1., 1.)), ignoredlabels=0, return_type=DICT, background=1)
    assert np.array_equal(sia._layer18(), brute_layer18(np.ascontiguousarray(vol))), c.name
