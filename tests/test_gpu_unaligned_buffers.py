"""Every pass of the C ABI on adopted device buffers whose base address is NOT a multiple of 16 bytes.

ta_volume_set_device / ta_signal_set_device / ta_overlap_set_device ask only for the alignment of the element type, so a pointer
2, 4 or 8 bytes off a 16-byte boundary is a valid input: a Z-slab cut out of one resident tensor whose planes are not a multiple
of 16 bytes, or any tensor view with a storage offset.  Almost every pass then leaves its 16-byte loads for a guarded scalar
variant -- a branch taken on the ADDRESS, which no other module reaches: their scalar cases all come from the row length.

The volumes here have rows of whole 16-byte strips (528 and 64 columns), so the address alone decides.  Every case builds its
buffer with offset_view(): one flat tensor, pads of a sentinel label that the volume does not hold in front of and behind the
voxels, and asserts the residue of the pointer it adopts -- offset 0, in the same parametrisation, is the control that runs the
aligned path through the same code.  After a pass the pads must still hold the sentinel and no result row may name it: a vector
store over the edge of the view, or a load that strays outside it, shows.

Which variant of a kernel ran is INFERRED from the launcher's condition and the asserted address; it is not observed on the device.

The tiling the shapes are chosen from is the signal / wall-geometry pass's: 4 rows x 64 * VPL columns x 16 planes (VPL = 8 for
uint16, 4 for uint32): (19, 7, 528) has more than one tile and a partial tile on every axis."""
import functools

import numpy as np
import pytest

import components_reference
import junction_reference
import overlap_reference
import signal_reference
import wall_geometry_reference
from oracle import onepass, onepass_c, sia_oracle
from oracle.sia_oracle import OracleSIA
from tissue_analysis_amd import CellJunctions, LabelComponents, WallGeometry, _capi, geometry, synth

from helpers import assert_same_accumulators, brute_wall_records
from test_gpu_components import same_rows
from test_gpu_junctions import check_tables
from test_gpu_wall_geometry import FIELDS, check_rows
from test_voxel_layers_cpu import brute_layer18

pytestmark = pytest.mark.gpu

SHAPE_A = (19, 7, 528)
SHAPE_B = (10, 12, 64)
TORCH_VIEW = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}

# (label type, offset of the volume in elements): offset 0 is the control; 1 element is 2 / 4 bytes off; 4 uint16 / 2 uint32
# elements are 8 bytes off -- where the wall-voxel pass keeps its 8-byte loads of uint16 while every 16-byte pass falls back
LABEL_CASES = [(np.uint16, 0), (np.uint16, 1), (np.uint16, 4), (np.uint32, 0), (np.uint32, 1), (np.uint32, 2)]
LABEL_IDS = ["u16+0B", "u16+2B", "u16+8B", "u32+0B", "u32+4B", "u32+8B"]
labels_param = pytest.mark.parametrize("dtype,off", LABEL_CASES, ids=LABEL_IDS)


class OffsetView(object):
    """What offset_view() made, and the check of its pads."""

    def __init__(self, flat, view, dev_ptr, dtype, off, size, sentinel):
        self.flat, self.view, self.dev_ptr = flat, view, dev_ptr
        self.dtype, self.off, self.size, self.sentinel = np.dtype(dtype), off, size, sentinel

    def __iter__(self):
        return iter((self.flat, self.view, self.dev_ptr))

    def read_back(self):
        """The voxels of the view as they are on the device now, after asserting that both pads still hold the sentinel."""
        import torch
        torch.cuda.synchronize()
        host = self.flat.cpu().numpy().view(self.dtype)
        head, tail = host[:self.off], host[self.off + self.size:]
        assert (head == self.sentinel).all(), "the pad in front of the view was written: %s" % head
        assert (tail == self.sentinel).all(), "the pad behind the view was written: %s" % tail
        return host[self.off:self.off + self.size]


def offset_view(host_array, offset_elems, tail_elems, sentinel=None):
    """One flat device tensor of offset_elems + size + tail_elems elements: `sentinel` (default: the largest value + 1, which the
    volume cannot hold) in both pads, the volume in between.  Returns (flat, view, dev_ptr), unpackable; .read_back() checks the
    pads.  The asserts keep a case from passing vacuously should the allocator ever hand out other addresses."""
    import torch
    a = np.ascontiguousarray(host_array)
    if sentinel is None:
        sentinel = int(a.max()) + 1
    assert sentinel <= np.iinfo(a.dtype).max and not (a == sentinel).any()
    host = np.full(offset_elems + a.size + tail_elems, sentinel, dtype=a.dtype)
    host[offset_elems:offset_elems + a.size] = a.reshape(-1)
    flat = torch.empty((host.size,), dtype=torch.from_numpy(host[:1].view(TORCH_VIEW[a.dtype])).dtype, device="cuda:0")
    flat.copy_(torch.from_numpy(host.view(TORCH_VIEW[a.dtype])))
    torch.cuda.synchronize()
    view = flat[offset_elems:offset_elems + a.size].view(*a.shape)
    dev_ptr = int(view.data_ptr())
    assert int(flat.data_ptr()) % 256 == 0
    assert dev_ptr == int(flat.data_ptr()) + offset_elems * a.dtype.itemsize
    assert dev_ptr % 16 == (offset_elems * a.dtype.itemsize) % 16
    return OffsetView(flat, view, dev_ptr, a.dtype, offset_elems, a.size, sentinel)


def adopt(ctx, V, off, tail=3, sentinel=None, slack=False):
    """V on the device `off` elements into a flat tensor, adopted by ctx.  keep = the WHOLE tensor: its data_ptr is not the
    pointer adopted (or, at offset 0, nothing of its storage lies behind it), so no slack is declared; slack = True keeps the
    view instead, whose storage goes on for `tail` elements."""
    ov = offset_view(V, off, tail, sentinel)
    ctx.set_volume_device(ov.dev_ptr, V.dtype.itemsize, V.shape, keep=ov.view if slack else ov.flat)
    assert (ctx.get_option(_capi.OPT_VOLUME_SLACK) >= 16) == slack
    return ov


def never_names(sentinel, *label_arrays):
    for a in label_arrays:
        assert not (np.asarray(a).astype(np.int64) == int(sentinel)).any(), "a result row names the sentinel label of the pads"


# ---- the volumes and their references: made once, never written to -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vol_a(dtype, cells=60, seed=3):
    v = synth.voronoi_labels(SHAPE_A, cells, seed, dtype=np.uint16).astype(dtype)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def vol_b(dtype):
    v = synth.voronoi_labels(SHAPE_B, 14, 5, dtype=np.uint16).astype(dtype)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def sweep_reference(dtype):
    V = vol_a(dtype)
    return onepass_c.extract(V, max_label=int(V.max()) + 1)          # (one row more: the sentinel's, which must stay empty)


def signal_image(shape, dtype, seed):
    """Every intensity of the type but the largest, which pads the signal buffers (offset_view's default sentinel)."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, np.iinfo(dtype).max, size=shape).astype(dtype)
    s.reshape(-1)[:2] = (0, np.iinfo(dtype).max - 1)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def signal_case(ldtype, sdtype):
    V, S = vol_a(ldtype), signal_image(SHAPE_A, sdtype, 7)
    return S, signal_reference.labels(V, S, int(V.max()) + 2), signal_reference.walls(V, S)


@functools.lru_cache(maxsize=None)
def overlap_case(da, db):
    A, B = vol_a(da), vol_a(db, 45, 4)
    return B, overlap_reference.table(A, B)


@functools.lru_cache(maxsize=None)
def structure_references(dtype):
    V = vol_a(dtype)
    return wall_geometry_reference.rows(V), junction_reference.tables(V), components_reference.table(V)


def sweep_arrays(ctx, adjacency=True):
    count, bbox, sum1, sum2 = ctx.labels()
    got = dict(count=count, bbox=bbox, sum1=sum1, sum2=sum2)
    if adjacency:
        got["pair_lo"], got["pair_hi"], got["pair_faces"] = ctx.adjacency()
    return got


# ---- 1. the fused sweep -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slack", [False, True], ids=["no_slack", "slack"])
@labels_param
def test_sweep(gpu_ctx, dtype, off, slack):
    """ta_api.hip run_extract: vec_ok = (base and rows 16-byte aligned) or declared slack.  Off the boundary without slack
    everything goes to the plain edge kernel; with >= 16 bytes of slack declared the interior / padded kernels issue their
    16-byte loads from the odd address.  impl 1 is the one-thread-a-voxel cross-check kernel."""
    V, want = vol_a(dtype), sweep_reference(dtype)
    L = int(V.max()) + 1
    try:
        ov = adopt(gpu_ctx, V, off, tail=16 if slack else 3, slack=slack)
        assert ov.sentinel == L
        for impl in (0, 1):
            gpu_ctx.set_option(_capi.OPT_IMPL, impl)
            for features in (_capi.F_ALL, 0x0f):
                gpu_ctx.extract(features, L)
                adjacency = bool(features & _capi.F_ADJACENCY)
                got = sweep_arrays(gpu_ctx, adjacency)
                if not adjacency:                                 # (no pair list was asked for: nothing of it to compare)
                    got.update((k, want[k]) for k in ("pair_lo", "pair_hi", "pair_faces"))
                assert_same_accumulators(got, want, "offset %d impl %d features %#x slack %s" % (off, impl, features, slack))
                assert got["count"][L] == 0
                never_names(L, got["pair_lo"], got["pair_hi"])
        ov.read_back()
    finally:
        gpu_ctx.set_option(_capi.OPT_IMPL, 0)


@labels_param
def test_sweep_of_ragged_rows_with_declared_slack(gpu_ctx, dtype, off):
    """Rows of 531 voxels are no whole strips: with slack declared the padded kernel loads the strip that straddles the end of a
    row where it is -- from the odd address, and behind the very last row out of the pad, whose sentinel is a valid row of the
    extraction: it must stay empty (the voxels outside the volume are overwritten with the filler when the plane lands)."""
    V = synth.voronoi_labels((19, 7, 531), 60, 3, dtype=np.uint16).astype(dtype)
    L = int(V.max()) + 1
    want = onepass_c.extract(V, max_label=L)
    ov = adopt(gpu_ctx, V, off, tail=16, slack=True)
    for features in (_capi.F_ALL, 0x0f):
        gpu_ctx.extract(features, L)
        adjacency = bool(features & _capi.F_ADJACENCY)
        got = sweep_arrays(gpu_ctx, adjacency)
        if not adjacency:
            got.update((k, want[k]) for k in ("pair_lo", "pair_hi", "pair_faces"))
        assert_same_accumulators(got, want, "offset %d features %#x" % (off, features))
        assert got["count"][L] == 0
        never_names(L, got["pair_lo"], got["pair_hi"])
    ov.read_back()


# ---- 2. signal statistics ---------------------------------------------------------------------------------------------------
SIGNAL_CASES = [(np.uint8, 0), (np.uint8, 1), (np.uint8, 4), (np.uint8, 8), (np.uint16, 0), (np.uint16, 2), (np.uint16, 8)]


@pytest.mark.parametrize("sdtype,sbytes", SIGNAL_CASES, ids=["s8+0B", "s8+1B", "s8+4B", "s8+8B", "s16+0B", "s16+2B", "s16+8B"])
@pytest.mark.parametrize("dtype,off", [(np.uint16, 0), (np.uint16, 1), (np.uint32, 0), (np.uint32, 1)],
                         ids=["u16+0B", "u16+2B", "u32+0B", "u32+4B"])
def test_signal(gpu_ctx, dtype, off, sdtype, sbytes):
    """kernels_signal.hip launch: vec = rows of whole strips and label base % 16 == 0 and signal base % (VPL * itemsize) == 0: the
    signal's own term is 8 / 16 bytes under uint16 labels (uint8 / uint16 signal) and 4 / 8 bytes under uint32 labels."""
    V = vol_a(dtype)
    S, r, w = signal_case(dtype, sdtype)
    L = int(V.max()) + 1
    ov = adopt(gpu_ctx, V, off)
    sv = offset_view(S, sbytes // np.dtype(sdtype).itemsize, 5)
    assert sv.dev_ptr % 16 == sbytes
    gpu_ctx.set_signal_device(sv.dev_ptr, np.dtype(sdtype).itemsize, keep=sv.flat)
    gpu_ctx.extract(_capi.F_ALL, L)
    gpu_ctx.signal_extract(_capi.SIG_LABELS | _capi.SIG_WALLS)
    n, s, q, mn, mx = gpu_ctx.signal_labels()
    lo, hi, faces = gpu_ctx.adjacency()
    slo, shi = gpu_ctx.signal_walls()
    assert np.array_equal(n, r["n"]) and np.array_equal(s, r["sum"])
    assert np.array_equal(q[:, 0], r["sumsq"]) and not q[:, 1].any()
    present = r["n"] > 0
    assert present.sum() > 50 and not present[L]
    assert np.array_equal(mn[present], r["min"][present]) and np.array_equal(mx[present], r["max"][present])
    assert (mn[~present] == 0xFFFFFFFF).all() and (mx[~present] == 0).all()
    assert w["lo"].size > 100
    assert np.array_equal(lo, w["lo"]) and np.array_equal(hi, w["hi"]) and np.array_equal(faces, w["faces"])
    assert np.array_equal(slo, w["side_lo"]) and np.array_equal(shi, w["side_hi"])
    never_names(L, lo, hi)
    ov.read_back()
    sv.read_back()


# ---- 3. overlap with a second volume ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_off,b_bytes", [(0, 0), (0, "1elem"), (0, 8), (1, 0), (1, "1elem"), (1, 8)],
                         ids=["A+0,B+0", "A+0,B+1elem", "A+0,B+8B", "A+1elem,B+0", "A+1elem,B+1elem", "A+1elem,B+8B"])
@pytest.mark.parametrize("da", [np.uint16, np.uint32], ids=["A16", "A32"])
@pytest.mark.parametrize("db", [np.uint16, np.uint32], ids=["B16", "B32"])
def test_overlap(gpu_ctx, da, db, a_off, b_bytes):
    """kernels_overlap.hip launch: vec = rows of whole strips and A % 16 == 0 and B % min(16, bytes of B's strip) == 0 -- B's strip
    is 8 bytes where A is uint32 and B uint16 (VPL = 4), so B 8 bytes off keeps the vector loads there and nowhere else."""
    A = vol_a(da)
    B, want = overlap_case(da, db)
    b_off = 1 if b_bytes == "1elem" else b_bytes // np.dtype(db).itemsize
    sentinel = 60000
    ov = adopt(gpu_ctx, A, a_off, sentinel=sentinel)
    bv = offset_view(B, b_off, 5, sentinel=sentinel)
    assert bv.dev_ptr % 16 == b_off * np.dtype(db).itemsize
    gpu_ctx.set_overlap_device(bv.dev_ptr, np.dtype(db).itemsize, keep=bv.flat)
    gpu_ctx.overlap_extract()
    a, b, n = gpu_ctx.overlap_get()
    assert want[0].size > 200
    assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(n, want[2])
    assert int(n.sum()) == A.size
    never_names(sentinel, a, b)
    ov.read_back()
    bv.read_back()


# ---- 4. wall geometry, junctions, components -------------------------------------------------------------------------------
@labels_param
def test_wall_geometry(gpu_ctx, dtype, off):
    """kernels_wallgeo.hip launch: vec = rows of whole strips and base % 16 == 0."""
    V = vol_a(dtype)
    want = structure_references(dtype)[0]
    L = int(V.max()) + 1
    ov = adopt(gpu_ctx, V, off)
    gpu_ctx.extract(_capi.F_ALL, L)
    plo, phi, faces = gpu_ctx.adjacency()
    gpu_ctx.wallgeo_extract()
    check_rows((plo, phi) + gpu_ctx.wallgeo_get(), want, faces, nonempty=True)
    never_names(L, plo, phi)
    ov.read_back()


@labels_param
def test_junctions(gpu_ctx, dtype, off):
    """kernels_junctions.hip launch: vec = rows of whole strips and base % 16 == 0."""
    V = vol_a(dtype)
    want = structure_references(dtype)[1]
    ov = adopt(gpu_ctx, V, off)
    gpu_ctx.junctions_extract()
    got = gpu_ctx.junctions_get()
    check_tables(got, want, nonempty=True)
    never_names(ov.sentinel, got[0][0], got[1][0])
    ov.read_back()


@labels_param
def test_components_their_image_and_the_relabelling_in_place(gpu_ctx, dtype, off):
    """kernels_components.hip local pass: vec = rows of whole strips and base % 16 == 0; ta_components_relabel writes the adopted
    buffer in place."""
    V = vol_a(dtype)
    rows, image = structure_references(dtype)[2]
    assert rows[0].size > np.unique(rows[0]).size > 50
    sentinel = 60000                                              # (the split names its new labels from the largest one up)
    ov = adopt(gpu_ctx, V, off, sentinel=sentinel)
    gpu_ctx.components_extract()
    got = gpu_ctx.components_get()
    same_rows(got, rows)
    never_names(sentinel, got[0])
    assert np.array_equal(gpu_ctx.components_image().reshape(V.shape), image)
    assert np.array_equal(gpu_ctx.components_image(3, 2), image[3:5].reshape(-1))
    assert np.array_equal(ov.read_back(), V.reshape(-1))
    new = components_reference.split_labels(rows[0], rows[1])
    assert (new != rows[0]).any() and new.max() < sentinel
    gpu_ctx.components_relabel(new.astype(np.uint32))
    gpu_ctx.synchronize()
    want = components_reference.split(V)[0]
    back = np.empty(V.shape, dtype=V.dtype)
    assert np.array_equal(gpu_ctx.get_volume(back), want)
    assert np.array_equal(ov.read_back().reshape(V.shape), want)


# ---- 5. census, compaction, plane events: sparse ids up to 2^32 - 1 ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sparse_case():
    V = vol_a(np.uint32)
    rng = np.random.default_rng(17)
    old = np.unique(V)
    new = np.unique(rng.integers(0, 1 << 32, size=4 * old.size, dtype=np.uint64))[:old.size]
    rng.shuffle(new)                                              # (an id's rank is not the rank of the label it replaces)
    new[0] = (1 << 32) - 1
    lut = np.zeros(int(old.max()) + 1, dtype=np.uint64)
    lut[old] = new
    S = lut[V].astype(np.uint32)
    S.setflags(write=False)
    ids, inv = np.unique(S, return_inverse=True)
    ranks = inv.reshape(S.shape).astype(np.uint32)
    return S, ids, onepass_c.extract(ranks, max_label=ids.size - 1)


@pytest.mark.parametrize("off", [0, 1, 2], ids=["u32+0B", "u32+4B", "u32+8B"])
def test_census_compaction_and_plane_events_on_sparse_ids(gpu_ctx, off):
    """kernels_basic.hip max_label (nvec = 0 off the boundary), kernels_census.hip: the row kernel gives up on a base that is not
    16-byte aligned (census_rows), the flat kernel then runs with nvec = 0, and so does the rank kernel that writes the compacted
    copy (launch_census_rank)."""
    S, ids, want = sparse_case()
    sentinel = 0x7FFFFFF1
    ov = adopt(gpu_ctx, S, off, sentinel=sentinel)
    assert gpu_ctx.max_label() == int(S.max()) == 0xFFFFFFFF
    top, present = gpu_ctx.label_census()
    assert top == 0xFFFFFFFF and np.array_equal(present, ids)
    events = gpu_ctx.plane_events()
    assert np.array_equal(events, (S[:, :, 1:] != S[:, :, :-1]).sum(axis=(1, 2)).astype(np.uint64)) and events.sum() > 1000
    table = gpu_ctx.compact_labels()
    assert gpu_ctx.is_compact() and np.array_equal(table, ids)
    never_names(sentinel, present, table)
    for again in (False, True):
        if again:
            gpu_ctx.rerank()                                      # the rank copy written again from the adopted buffer
        gpu_ctx.extract(_capi.F_ALL, ids.size - 1)
        got = sweep_arrays(gpu_ctx)
        for k in ("count", "bbox", "sum1", "sum2"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["pair_lo"], ids[want["pair_lo"].astype(np.int64)])      # the pair list answers in ids
        assert np.array_equal(got["pair_hi"], ids[want["pair_hi"].astype(np.int64)])
        assert np.array_equal(got["pair_faces"], want["pair_faces"])
        never_names(sentinel, got["pair_lo"], got["pair_hi"])
    gpu_ctx.synchronize()
    assert np.array_equal(ov.read_back(), S.reshape(-1))
    # a compacted context relabels through one entry per rank: the kernel reads the library's rank copy and writes the adopted
    # buffer in place (launch_relabel: the vector variant needs BOTH on a 16-byte boundary)
    fused = ids.copy()
    fused[3] = ids[2]
    gpu_ctx.relabel(fused)
    assert not gpu_ctx.is_compact()
    want_fused = np.where(S == ids[3], ids[2], S)
    assert (want_fused != S).any()
    assert np.array_equal(ov.read_back().reshape(S.shape), want_fused)


# ---- 6. lookup tables -------------------------------------------------------------------------------------------------------
@labels_param
def test_relabel_in_place_and_map_labels(gpu_ctx, dtype, off):
    """kernels_basic.hip launch_relabel: 16-byte loads AND stores only where the buffer is 16-byte aligned, else the whole volume
    goes through the scalar tail.  The table renames the sentinel too: a store over the edge of the view would change a pad."""
    V = vol_a(dtype)
    ov = adopt(gpu_ctx, V, off)
    rng = np.random.default_rng(23)
    lut = rng.integers(0, 60000, size=ov.sentinel + 1).astype(np.uint32)
    lut[ov.sentinel] = 60001
    mapped = gpu_ctx.map_labels(lut.astype(np.float64) * 0.25, -1.0, V)
    assert mapped.dtype == np.float64 and np.array_equal(mapped, lut[V] * 0.25)
    short = lut[:int(V.max())]                                    # the largest label lies beyond this table: it stays / is filled
    assert np.array_equal(gpu_ctx.map_labels(short.astype(np.uint16), 65535, V), np.where(V < short.size, lut[np.minimum(V, short.size - 1)], 65535))
    gpu_ctx.relabel(lut)
    want = lut[V].astype(dtype)
    assert (want != V).any()
    back = np.empty(V.shape, dtype=V.dtype)
    assert np.array_equal(gpu_ctx.get_volume(back), want)
    assert np.array_equal(ov.read_back().reshape(V.shape), want)


# ---- 7. the voxel-layer stencils --------------------------------------------------------------------------------------------
@labels_param
def test_first_layer_hollow_and_layer18(gpu_ctx, dtype, off):
    """kernels_basic.hip first_layer / hollow / layer18 kernels: vec_ok = rows of whole strips and (input | output) % 16 == 0 (the
    output is the library's own buffer: only the input's address varies here).  64 columns: eight strips of uint16, sixteen of
    uint32."""
    V = vol_b(dtype)
    ov = adopt(gpu_ctx, V, off)
    for keep in (True, False):
        want = OracleSIA(np.array(V), background=1).voxel_first_layer(keep)
        got = gpu_ctx.first_layer(1, keep, V)
        assert got.dtype == V.dtype and np.array_equal(got, want) and np.count_nonzero(want) > 100, keep
    for bg, remove in ((1, True), (1, False), (3, True)):
        want = sia_oracle.hollow_out_cells(np.array(V), bg, remove_background=remove)
        got = gpu_ctx.hollow(bg, remove, V)
        assert got.dtype == V.dtype and np.array_equal(got, want) and np.count_nonzero(want) > 100, (bg, remove)
    want = brute_layer18(V)
    got = gpu_ctx.layer18(V)
    assert got.dtype == np.uint8 and np.array_equal(got, want) and 100 < np.count_nonzero(want) < V.size
    assert np.array_equal(ov.read_back(), V.reshape(-1))


# ---- 8. wall voxels, medians, meshes ----------------------------------------------------------------------------------------
def canonical(lo, hi, coords):
    order = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0], hi, lo))
    return lo[order], hi[order], coords[order]


@functools.lru_cache(maxsize=None)
def aligned_wall_answers(dtype):
    """The same calls on a context that holds an aligned copy of the volume (the library's own upload): what the wall-voxel and
    mesh modules hold against the CPU references."""
    V = vol_b(dtype)
    ctx = _capi.Context(0)
    try:
        ctx.set_volume(V)
        plain, grouped, medians = ctx.wall_voxels(), ctx.wall_voxels(by_pair=True), ctx.wall_medians()
        ctx.extract(_capi.F_ALL, int(V.max()) + 1)
        mesh = ctx.mesh(1)
    finally:
        ctx.close()
    return plain, grouped, medians, mesh


@labels_param
def test_wall_voxels_medians_and_mesh(gpu_ctx, dtype, off):
    """kernels_walls.hip launch: QUADS = rows of a multiple of 4 columns and base % (4 * itemsize) == 0, i.e. 8 bytes for uint16 --
    which an 8-byte offset keeps and a 2-byte offset loses -- and 16 bytes for uint32."""
    V = vol_b(dtype)
    plain, grouped, medians, mesh = aligned_wall_answers(dtype)
    ov = adopt(gpu_ctx, V, off)
    lo, hi, coords, _ = gpu_ctx.wall_voxels()
    for got, want in zip(canonical(lo, hi, coords), canonical(*plain[:3])):
        assert np.array_equal(got, want)
    glo, ghi, gcoords, _ = gpu_ctx.wall_voxels(by_pair=True)
    for got, want in zip(canonical(glo, ghi, gcoords), canonical(*grouped[:3])):
        assert np.array_equal(got, want)
    for got, want in zip((glo, ghi, gcoords), brute_wall_records(V)):                # ... and the brute force over the 18 offsets
        assert np.array_equal(got, want)
    assert glo.size > 1000
    never_names(ov.sentinel, lo, hi, glo, ghi)
    keys, sizes, med, _, moving = gpu_ctx.wall_medians()
    assert not moving.any() and keys.size > 5
    assert np.array_equal(keys, medians[0]) and np.array_equal(sizes, medians[1]) and np.array_equal(med, medians[2])
    k = (glo.astype(np.uint64) << np.uint64(32)) | ghi.astype(np.uint64)
    uk, count = np.unique(k, return_counts=True)
    assert np.array_equal(keys, uk) and np.array_equal(sizes, count.astype(np.uint32))
    assert np.array_equal(med.astype(np.int64), geometry.median_voxels(gcoords.astype(np.int64), count).reshape(-1, 3))
    gpu_ctx.extract(_capi.F_ALL, int(V.max()) + 1)
    got = gpu_ctx.mesh(1)
    assert got[4].shape[0] > 1000                                 # triangles
    for g, w in zip(got[:7], mesh[:7]):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert np.array_equal(ov.read_back(), V.reshape(-1))


# ---- slabs as views of ONE resident tensor whose planes are not a multiple of 16 bytes -----------------------------------------
SLAB_CASES = [
    ("u16_plane_506B", (9, 11, 23), np.uint16, np.uint8, np.uint32, (4,)),
    ("u16_plane_506B", (9, 11, 23), np.uint16, np.uint8, np.uint32, (3, 6)),
    ("u32_plane_6020B", (6, 5, 301), np.uint32, np.uint16, np.uint16, (4,)),
    ("u32_plane_6020B", (6, 5, 301), np.uint32, np.uint16, np.uint16, (2, 4)),
]


@functools.lru_cache(maxsize=None)
def slab_volumes(shape, dtype, sdtype, bdtype):
    V = synth.voronoi_labels(shape, 14, 31, dtype=np.uint16).astype(dtype)
    B = synth.voronoi_labels(shape, 9, 32, dtype=np.uint16).astype(bdtype)
    S = signal_image(shape, sdtype, 33)
    L = int(V.max())
    whole = dict(sweep=onepass_c.extract(V), signal=(signal_reference.labels(V, S, L + 1), signal_reference.walls(V, S)),
                 overlap=overlap_reference.table(V, B), junctions=junction_reference.tables(V),
                 wallgeo=wall_geometry_reference.rows(V), components=components_reference.table(V)[0])
    return V, S, B, whole


def on_device(a):
    import torch
    t = torch.from_numpy(np.array(a).view(TORCH_VIEW[a.dtype])).cuda()
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("name,shape,dtype,sdtype,bdtype,cuts", SLAB_CASES, ids=["%s-cuts%s" % (c[0], "_".join(map(str, c[5]))) for c in SLAB_CASES])
def test_slabs_cut_out_of_one_resident_tensor_merge_to_the_whole(name, shape, dtype, sdtype, bdtype, cuts):
    """Each slab is adopted as whole.data_ptr() + (lo - halo) * plane_bytes -- labels, signal and second volume alike -- with its
    global origin and its low halo plane: sweep, signal, overlap, junctions, wall geometry and components of every slab against the
    reference of that slab, and merged against the reference of the whole volume."""
    V, S, B, whole = slab_volumes(shape, dtype, sdtype, bdtype)
    L = int(V.max())
    tv, ts, tb = on_device(V), on_device(S), on_device(B)
    plane = shape[1] * shape[2]
    edges = (0,) + tuple(cuts) + (shape[0],)
    residues = []
    sweeps, sig_rows, sig_walls, overlaps, junctions, wallgeos, wall_wants, comps, tops, halos = [], [], {}, [], [], [], [], [], [], []
    ctx = _capi.Context(0)
    try:
        for lo, hi in zip(edges[:-1], edges[1:]):
            halo = 1 if lo > 0 else 0
            first = lo - halo
            ptr = int(tv.data_ptr()) + first * plane * V.dtype.itemsize
            residues.append(ptr % 16)
            dims = (hi - first, shape[1], shape[2])
            sub, ssub, bsub = V[first:hi], S[first:hi], B[first:hi]
            ctx.set_volume_device(ptr, V.dtype.itemsize, dims, a0_origin=lo, has_low_halo=bool(halo), keep=tv)
            assert ctx.get_option(_capi.OPT_VOLUME_SLACK) == 0
            ctx.set_signal_device(int(ts.data_ptr()) + first * plane * S.dtype.itemsize, S.dtype.itemsize, keep=ts)
            ctx.set_overlap_device(int(tb.data_ptr()) + first * plane * B.dtype.itemsize, B.dtype.itemsize, keep=tb)
            # the sweep
            ctx.extract(_capi.F_ALL, L)
            part = sweep_arrays(ctx)
            assert_same_accumulators(part, onepass_c.extract(sub, max_label=L, origin=(first, 0, 0), own_first_plane=not halo), "slab %d:%d" % (lo, hi))
            part["max_label"] = L
            sweeps.append(part)
            # signal
            ctx.signal_extract()
            n, s, q, mn, mx = ctx.signal_labels()
            slo, shi = ctx.signal_walls()
            r = signal_reference.labels(sub, ssub, L + 1, first_owned=halo)
            w = signal_reference.walls(sub, ssub, first_owned=halo)
            p = r["n"] > 0
            assert np.array_equal(n, r["n"]) and np.array_equal(s, r["sum"]) and np.array_equal(q[:, 0], r["sumsq"])
            assert np.array_equal(mn[p], r["min"][p]) and np.array_equal(mx[p], r["max"][p])
            assert np.array_equal(part["pair_lo"], w["lo"]) and np.array_equal(part["pair_hi"], w["hi"])
            assert np.array_equal(slo, w["side_lo"]) and np.array_equal(shi, w["side_hi"])
            sig_rows.append((n, s, q[:, 0], np.where(p, mn, 0xFFFFFFFF), np.where(p, mx, 0)))
            for key, a, b in zip(w["keys"].tolist(), slo.tolist(), shi.tolist()):
                t = sig_walls.setdefault(key, [0, 0])
                t[0] += a
                t[1] += b
            # overlap
            ctx.overlap_extract()
            a, b, n = ctx.overlap_get()
            want = overlap_reference.table(sub, bsub, first_owned=halo)
            assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(n, want[2])
            overlaps.append((a.astype(np.int64), b.astype(np.int64), n))
            # junctions
            ctx.junctions_extract()
            got = ctx.junctions_get()
            check_tables(got, junction_reference.tables(sub, first_owned=halo, a0_origin=lo))
            junctions.append(tuple((g[0].astype(np.int64), g[1], g[2]) for g in got[:2]) + (got[2],))
            # wall geometry
            ctx.wallgeo_extract()
            got = (part["pair_lo"], part["pair_hi"]) + ctx.wallgeo_get()
            want = wall_geometry_reference.rows(sub, first_owned=halo, a0_origin=lo)
            check_rows(got, want, part["pair_faces"])
            wallgeos.append(WallGeometry(*got))
            wall_wants.append(want)
            # components
            ctx.components_extract()
            got = ctx.components_get()
            rows, image = components_reference.table(sub, first_owned=halo, a0_origin=lo)
            same_rows(got, rows)
            assert np.array_equal(ctx.components_image().reshape(dims), image)
            tops.append(ctx.components_image(dims[0] - 1, 1))
            halos.append(ctx.components_image(0, 1))
            comps.append(LabelComponents(*got))
    finally:
        ctx.close()
    assert any(residues) and residues[0] == 0, residues          # a slab pointer off the 16-byte boundary, and the aligned control
    assert_same_accumulators(onepass.merge(sweeps), whole["sweep"], "merged")
    r, w = whole["signal"]
    assert np.array_equal(sum(p[0] for p in sig_rows), r["n"]) and np.array_equal(sum(p[1] for p in sig_rows), r["sum"])
    assert np.array_equal(sum(p[2] for p in sig_rows), r["sumsq"])
    assert np.array_equal(np.minimum.reduce([p[3] for p in sig_rows]), r["min"])
    assert np.array_equal(np.maximum.reduce([p[4] for p in sig_rows]), r["max"])
    assert sorted(sig_walls) == w["keys"].tolist()
    assert [sig_walls[k] for k in w["keys"].tolist()] == [[a, b] for a, b in zip(w["side_lo"].tolist(), w["side_hi"].tolist())]
    for got, want in zip(overlap_reference.merge(overlaps), whole["overlap"]):
        assert np.array_equal(got, want)
    check_tables(junction_reference.merge(junctions), whole["junctions"])
    assert whole["junctions"][0][1].size > 0
    J = CellJunctions.merge([CellJunctions(p[0][0], p[0][1], p[0][2], p[1][0], p[1][1], p[1][2], p[2]) for p in junctions])
    check_tables(J, whole["junctions"])
    check_rows(WallGeometry.merge(wallgeos), whole["wallgeo"], nonempty=True)
    check_rows(tuple(wall_geometry_reference.merge(wall_wants)[k] for k in ("lo", "hi") + FIELDS), whole["wallgeo"])
    same_rows(LabelComponents.merge(comps, [(tops[k], halos[k + 1]) for k in range(len(comps) - 1)]), whole["components"])
