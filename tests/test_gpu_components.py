"""Connected components of the labels on the MI355X (include/tissue_scan_components.h, csrc/kernels_components.hip) against the
NumPy / SciPy restatement of tests/components_reference.py: every number is an integer and must be bit-exact, in the table and in
the row image.  The local pass's tile is 4 planes x 4 rows x 256 columns of voxels (components.TILE): the shapes below are chosen
from it."""
import numpy as np
import pytest

import components_reference as ref
from tissue_analysis_amd import DICT, LabelComponents, SpatialImage, SpatialImageAnalysis, _capi, components, label_components, synth
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu

TP, TR, TC = components.TILE


def test_the_tile_the_shapes_are_chosen_from():
    assert (TP, TR, TC) == (4, 4, 256) and components.NONE == ref.NONE == _capi.COMPONENT_NONE


def same_rows(got, want):
    """got: LabelComponents or the tuple of Context.components_get; want: the rows of ref.table()."""
    if isinstance(got, LabelComponents):
        assert got.label.dtype == np.int64 and got.n.dtype == np.uint64 and got.sum1.dtype == np.uint64
        got = (got.label, got.n, got.first, got.bbox, got.sum1)
    for g, w, name in zip(got, want, ("label", "n", "first", "bbox", "sum1")):
        assert g.shape == w.shape, name
        assert np.array_equal(g.astype(w.dtype), w), name


def run(V):
    rv = ResidentVolume(V)
    try:
        cc = rv.components()
        image = rv.components_image()
        assert cc.ms is not None and cc.ms[0] > 0.0 and cc.ms[1] >= 0.0
    finally:
        rv.close()
    return cc, image


def check(V, want=None):
    """The device's table and row image of V against the restatement's (`want`: ref.table(V) when the caller has it)."""
    rows, image = ref.table(V) if want is None else want
    cc, got = run(V)
    same_rows(cc, rows)
    V3 = V[:, :, None] if V.ndim == 2 else V
    assert got.dtype == np.uint32 and got.shape == V3.shape and np.array_equal(got, image)
    return cc


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
def test_label_types_and_strips(dtype):
    # rows of 531 voxels are not whole 16-byte strips (the scalar loads), rows of 528 and 264 are; partial tiles on every axis
    for dims in ((19, 7, 531), (19, 7, 528), (33, 10, 264), (2 * TP + 1, 2 * TR + 3, 2 * TC + 19)):
        V = synth.voronoi_labels(dims, 60, 3, dtype=np.uint16).astype(dtype)
        want = ref.table(V)
        if dims == (19, 7, 531):
            assert want[0][0].size == 97 and np.unique(want[0][0]).size == 91
        assert want[0][0].size > np.unique(want[0][0]).size > 50                # fragmented labels among many
        check(V, want)


def test_thin_and_tiny_volumes():
    for dims, least in (((1, 9, 40), 19), ((5, 1, 64), 17), ((1, 1, 77), 32), ((1, 1, 1), 1)):
        V = synth.voronoi_labels(dims, 6, 3, dtype=np.uint16)
        want = ref.table(V)
        assert want[0][0].size == least
        check(V, want)
        check(V.astype(np.uint32), want)
    A = synth.voronoi_labels((1, 200, 150), 40, 3, dtype=np.uint16)[0]          # a 2-D image through the public function
    rows, _ = ref.table(A)
    assert rows[0].size == 276 and np.unique(rows[0]).size == 273
    img = SpatialImage(A.astype(np.int64), voxelsize=(0.5, 0.25))
    cc = label_components(img)
    same_rows(cc, rows)
    assert not cc.sum1[:, 2].any() and cc.voxelsize == (0.5, 0.25, 1.0)
    assert np.array_equal(cc.bbox[:, 5], np.ones(len(cc), dtype=np.int64))


def test_dense_layouts_other_than_c_order():
    V = synth.voronoi_labels((24, 40, 56), 60, 3, dtype=np.uint16)
    want = ref.table(V)
    assert want[0][0].size == 57 and np.unique(want[0][0]).size == 43
    c_rows = check(V, want)
    f_rows = check(np.asfortranarray(V), want)                                  # the same array: the same table, bit for bit
    same_rows(f_rows, (c_rows.label, c_rows.n, c_rows.first, c_rows.bbox, c_rows.sum1))
    VT = V.transpose(1, 2, 0)                                                   # the axes permuted: the table of the permuted array
    t_rows = check(VT, ref.table(VT))
    same_rows(check(np.ascontiguousarray(VT)), (t_rows.label, t_rows.n, t_rows.first, t_rows.bbox, t_rows.sum1))
    check(np.asfortranarray(V.astype(np.uint32)), want)


def test_noise():
    rng = np.random.default_rng(7)
    V = rng.integers(0, 3, size=(24, 24, 40)).astype(np.uint16)
    want = ref.table(V)
    assert want[0][0].size == 3593 and np.unique(want[0][0]).size == 3
    check(V, want)
    V = rng.integers(0, 2, size=(33, 20, 130)).astype(np.uint32)
    want = ref.table(V)
    assert want[0][0].size > 1000 and np.unique(want[0][0]).size == 2
    check(V, want)
    V = rng.integers(0, 4000, size=(16, 16, 16)).astype(np.uint16)              # nearly every voxel a component of its own
    want = ref.table(V)
    assert want[0][0].size == 4092
    check(V, want)


def test_checkerboard_never_joins_diagonally():
    i, j, k = np.indices((12, 12, 70))
    V = ((i + j + k) % 2 + 1).astype(np.uint16)
    want = ref.table(V)
    assert want[0][0].size == V.size == 10080 and int(want[0][1].max()) == 1    # the table at one row per voxel
    check(V, want)


def test_uniform_volume_is_one_row():
    V = np.full((40, 40, 300), 3, dtype=np.uint16)
    want = ref.table(V)
    assert want[0][0].tolist() == [3] and want[0][1].tolist() == [480000]
    cc = check(V, want)
    assert cc.bbox.tolist() == [[0, 0, 0, 40, 40, 300]] and cc.first.tolist() == [[0, 0, 0]]


def serpentine(dims):
    """Label 1 winds through every tile between walls of label 2: every second row of every second plane, neighbouring rows
    joined at alternating ends, neighbouring planes at alternating corners."""
    n0, n1, n2 = dims
    V = np.full(dims, 2, dtype=np.uint16)
    rows = list(range(0, n1, 2))
    for q in range(0, n0, 2):
        for a, r in enumerate(rows):
            V[q, r, :] = 1
            if a + 1 < len(rows):
                V[q, r + 1, n2 - 1 if a % 2 == 0 else 0] = 1
        if q + 2 < n0:
            if (q // 2) % 2 == 0:                                               # the snake leaves where the plane's last row ends
                V[q + 1, rows[-1], n2 - 1 if (len(rows) - 1) % 2 == 0 else 0] = 1
            else:
                V[q + 1, 0, 0] = 1
    return V


def helix(V, origin, turns):
    """Label 3 inside the tile at `origin`, in a block of label 2: it goes round the 4 x 4 ring of the tile's planes and rows (eleven
    of its twelve voxels) in one column and steps two columns on for the next turn."""
    q0, r0, c0 = origin
    ring = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 3), (2, 3), (3, 3), (3, 2), (3, 1), (3, 0), (2, 0), (1, 0)]
    V[q0:q0 + TP, r0:r0 + TR, c0:c0 + 2 * turns] = 2
    at = 0
    for t in range(turns):
        for step in range(11):
            q, r = ring[(at + step) % 12]
            V[q0 + q, r0 + r, c0 + 2 * t] = 3
        at = (at + 10) % 12
        q, r = ring[at]
        if t + 1 < turns:
            V[q0 + q, r0 + r, c0 + 2 * t + 1] = 3


def test_serpentine_through_every_tile_and_a_helix_inside_one():
    dims = (3 * TP + 1, 3 * TR + 1, 3 * TC + 2)
    V = serpentine(dims)
    helix(V, (TP, TR, TC), 100)                                                 # inside the tile (1, 1, 1): columns 256 .. 455
    want = ref.table(V)
    label, n = want[0][0], want[0][1]
    assert np.count_nonzero(label == 3) == 1 and int(n[label == 3][0]) == 100 * 11 + 99
    snakes = np.flatnonzero(label == 1)
    # the helix's block cuts the one snake of the serpentine where it passes the tile: every piece is one row, the restatement counts them
    assert 1 <= snakes.size <= 8 and int(n[snakes].max()) > 2 * TC * TR
    W = serpentine(dims)
    whole = ref.table(W)
    assert whole[0][0].tolist().count(1) == 1                                   # the uncut serpentine: ONE row through every tile
    assert int(whole[0][1][whole[0][0] == 1][0]) == int((W == 1).sum()) > 7 * 7 * dims[2]
    check(W, whole)
    check(V, want)
    check(V.astype(np.uint32), want)


def test_u_across_a_tile_face_for_each_axis():
    V = np.ones((2 * TP, 2 * TR, 2 * TC), dtype=np.uint16)
    V[1:TP + 1, 1, 10] = V[1:TP + 1, 1, 12] = 5                                 # arms along axis 0, joined in the next tile
    V[TP, 1, 10:13] = 5
    V[1, 1:TR + 1, 20] = V[1, 1:TR + 1, 22] = 6                                 # along axis 1
    V[1, TR, 20:23] = 6
    V[2, 0, TC - 6:TC + 1] = V[2, 2, TC - 6:TC + 1] = 7                         # along axis 2
    V[2, 0:3, TC] = 7
    want = ref.table(V)
    for l in (5, 6, 7):
        assert want[0][0].tolist().count(l) == 1
    assert ref.table(V[:TP])[0][0].tolist().count(5) == 2                       # two arms inside the first tile
    assert ref.table(V[:, :TR])[0][0].tolist().count(6) == 2
    assert ref.table(V[:, :, :TC])[0][0].tolist().count(7) == 2
    check(V, want)
    check(V.astype(np.uint32), want)


def test_extreme_ids_and_a_compacted_context():
    rng = np.random.default_rng(5)
    ids = np.array([0, 7, 70000, 2**31 + 5, 2**32 - 2, 2**32 - 1], dtype=np.uint32)
    V = ids[rng.integers(0, ids.size, size=(12, 9, 33))]
    rows, image = ref.table(V)
    assert rows[0].min() == 0 and rows[0].max() == 2**32 - 1 and rows[0].size > 1000
    rv = ResidentVolume(V)
    try:
        same_rows(rv.components(), rows)
        x = rv.extract(sparse=True)
        assert rv.ctx.is_compact() and x.ids is not None
        same_rows(rv.components(), rows)                                         # rows of the sweep are ranks, the table speaks in ids
        assert np.array_equal(rv.components_image(), image)
        rv.ctx.uncompact()
        same_rows(rv.components(), rows)
    finally:
        rv.close()


def test_two_runs_on_one_context_are_identical():
    V = synth.voronoi_labels((2 * TP + 3, 2 * TR + 1, 2 * TC + 40), 80, 3, dtype=np.uint16)
    assert ref.table(V)[0][0].size > 40
    ctx = _capi.Context(0)
    try:
        ctx.set_volume(V)
        ctx.components_extract()
        a, ia = ctx.components_get(), ctx.components_image()
        ctx.components_extract()
        b, ib = ctx.components_get(), ctx.components_image()
    finally:
        ctx.close()
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.array_equal(ia, ib)


def u_volume():
    """Voronoi cells, and a U of label 500 whose arms run along axis 0 and are joined at plane 20 only: a cut below plane 20 leaves
    two rows in the lower slab that only the upper slab joins."""
    V = synth.voronoi_labels((24, 20, 30), 30, 3, dtype=np.uint16)
    V[2:21, 5, 4] = 500
    V[2:21, 5, 12] = 500
    V[20, 5, 4:13] = 500
    V[6:9, 15, 20:23] = 500
    return V


def test_three_slabs_with_a_low_halo_merge_to_the_whole():
    import torch
    V = u_volume()
    whole, _ = ref.table(V)
    assert whole[0].tolist().count(500) == 2
    want_parts, want_seams = ref.slabs(V, (7, 15))
    assert want_parts[0][0].tolist().count(500) == 3 and want_parts[1][0].tolist().count(500) == 3
    assert any((s[1] == ref.NONE).any() for s in want_seams)                    # a component that lives in a halo plane only
    edges = (0, 7, 15, V.shape[0])
    parts, tops, halos = [], [], []
    for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        halo = lo > 0
        lo_ = lo - 1 if halo else lo
        t = torch.from_numpy(V[lo_:hi].view(np.int16).copy()).cuda()
        torch.cuda.synchronize()
        ctx = _capi.Context(0)
        try:
            ctx.set_volume_device(t.data_ptr(), 2, t.shape, a0_origin=lo, has_low_halo=halo, keep=t)
            ctx.components_extract()
            got = ctx.components_get()
            image = ctx.components_image().reshape(t.shape)
            tops.append(ctx.components_image(hi - lo_ - 1, 1))
            halos.append(ctx.components_image(0, 1))
        finally:
            ctx.close()
        rows, want_image = ref.table(V[lo_:hi], first_owned=1 if halo else 0, a0_origin=lo)
        same_rows(got, rows)
        same_rows(got, want_parts[k])
        assert np.array_equal(image, want_image)
        assert np.array_equal(tops[-1], want_image[-1].reshape(-1)) and np.array_equal(halos[-1], want_image[0].reshape(-1))
        parts.append(LabelComponents(*got))
    merged = LabelComponents.merge(parts, [(tops[k], halos[k + 1]) for k in range(2)])
    same_rows(merged, whole)


def _code(call, *args):
    with pytest.raises(_capi.TissueScanError) as e:
        call(*args)
    return e.value.code


def test_argument_checks_and_invalidation():
    V = synth.voronoi_labels((10, 12, 40), 30, 3, dtype=np.uint16)
    ctx = _capi.Context(0)
    try:
        assert _code(ctx.components_extract) == _capi.TA_EINVAL                  # no volume
        ctx.set_volume(V)
        getters = (ctx.components_size, ctx.components_get, ctx.components_timing, ctx.components_image)
        for call in getters:
            assert _code(call) == _capi.TA_EINVAL                               # no pass yet
        lib, h = ctx._lib, ctx._h
        assert lib.ta_components_get(h, None, None, None, None, None) == _capi.TA_EINVAL
        ctx.components_extract()
        rows, image = ref.table(V)
        same_rows(ctx.components_get(), rows)
        R = ctx.components_size()
        assert lib.ta_components_get(h, None, None, None, None, None) == _capi.TA_OK          # any pointer may be NULL
        assert lib.ta_components_size(h, None) == _capi.TA_OK
        ms_pass, ms_after = ctx.components_timing()
        assert ms_pass > 0.0 and ms_after > 0.0
        assert np.array_equal(ctx.components_image(3, 2), image[3:5].reshape(-1))
        assert ctx.components_image(10, 0).size == 0
        assert _code(ctx.components_image, 9, 2) == _capi.TA_EINVAL              # planes outside the buffer
        assert _code(ctx.components_image, -1, 1) == _capi.TA_EINVAL
        assert _code(ctx.components_relabel, np.zeros(R + 1, dtype=np.uint32)) == _capi.TA_EINVAL
        big = rows[0].astype(np.uint32)
        big[-1] = 70000
        assert _code(ctx.components_relabel, big) == _capi.TA_ERANGE             # does not fit uint16
        back = np.empty_like(V)
        assert np.array_equal(ctx.get_volume(back), V)                           # both failed before the volume was touched
        assert ctx.components_size() == R                                        # ... and the tables still stand
        lut = np.arange(int(V.max()) + 1, dtype=np.uint32)
        lut[5] = 3                                                               # two cells fused
        ctx.relabel(lut)                                                         # ta_volume_relabel
        for call in getters:
            assert _code(call) == _capi.TA_EINVAL
        ctx.components_extract()
        same_rows(ctx.components_get(), ref.table(lut[V])[0])
        ctx.set_volume(V)                                                        # a new volume
        for call in getters:
            assert _code(call) == _capi.TA_EINVAL
        assert lib.ta_components_relabel(h, None, 0) == _capi.TA_EINVAL
        ctx.components_extract()
        ctx.set_volume(np.ascontiguousarray(V[:, :, :32]))                       # a new volume while the count is the only thing done
        assert _code(ctx.components_get) == _capi.TA_EINVAL
        ctx.components_extract()
        rows = ref.table(V[:, :, :32])[0]
        same_rows(ctx.components_get(), rows)
        ctx.components_relabel(ref.split_labels(rows[0], rows[1]).astype(np.uint32))     # ta_components_relabel
        for call in getters:
            assert _code(call) == _capi.TA_EINVAL
        back = np.empty_like(V[:, :, :32])
        assert np.array_equal(ctx.get_volume(back), ref.split(V[:, :, :32])[0])
    finally:
        ctx.close()


def test_relabel_components_of_a_resident_volume():
    V = synth.voronoi_labels((20, 24, 70), 60, 3, dtype=np.uint16)
    rows, _ = ref.table(V)
    assert rows[0].size > np.unique(rows[0]).size
    rv = ResidentVolume(V.copy())
    try:
        cc = rv.components()
        with pytest.raises(ValueError):
            rv.relabel_components(np.full(len(cc), 65536))
        assert _code(rv.relabel_components, cc.split_map()[:-1]) == _capi.TA_EINVAL
        x = rv.relabel_components(cc.split_map())
        want, _ = ref.split(V)
        assert np.array_equal(rv.host, want)
        assert np.array_equal(x.count[x.count > 0], np.bincount(want.reshape(-1))[np.bincount(want.reshape(-1)) > 0])
        assert _code(rv.ctx.components_size) == _capi.TA_EINVAL
        assert len(rv.components()) == np.unique(want).size                      # one component per label now
    finally:
        rv.close()


def test_split_and_erase_through_the_analysis():
    V = synth.voronoi_labels((64, 64, 64), 200, 3)
    rows, _ = ref.table(V)
    assert rows[0].size == 243 and np.unique(rows[0]).size == 156
    sia = SpatialImageAnalysis(SpatialImage(V.copy(), voxelsize=(0.5, 0.25, 2.0)), ignoredlabels=0, background=1, return_type=DICT)
    cc = sia.label_components()
    same_rows(cc, rows)
    assert sia.label_components() is cc and cc.voxelsize == (0.5, 0.25, 2.0)     # cached
    frag = sia.disconnected_labels()
    assert frag == dict((l, k) for l, k in cc.fragmented().items() if l not in (0, 1)) and len(frag) >= 20
    want, renamed = ref.split(V)
    got = sia.split_disconnected_labels()
    assert got == renamed and len(got) == 243 - 156
    assert np.array_equal(np.asarray(sia.image), want)
    after = sia.label_components()
    assert after is not cc and len(after) == 243 and after.fragmented() == {} and sia.disconnected_labels() == {}
    same_rows(after, ref.table(want)[0])
    # the tables after the edit describe the new image
    vol = sia.volume(real=False)
    counts = np.bincount(want.reshape(-1))
    new_id = max(got)
    assert vol[new_id] == counts[new_id] > 0
    assert sorted(sia.neighbors(new_id)) == sorted(set(brute_neighbors(want, new_id)))
    assert sia.split_disconnected_labels() == {}                                 # nothing left to split
    # erase
    sia2 = SpatialImageAnalysis(SpatialImage(V.copy(), voxelsize=(0.5, 0.25, 2.0)), ignoredlabels=0, background=1, return_type=DICT)
    want2 = ref.erase(V, 3)                                                      # fragments of 1 and 2 voxels go, those of 3 to 6 stay
    assert (want2 != V).any() and (ref.erase(V, 10 ** 9) != want2).any()
    erased = sia2.remove_small_fragments(3)
    assert erased == int(((ref.erase_labels(rows[0], rows[1], 3) != rows[0])).sum()) == 82
    assert np.array_equal(np.asarray(sia2.image), want2)
    same_rows(sia2.label_components(), ref.table(want2)[0])
    assert 0 in sia2.ignoredlabels()


def brute_neighbors(V, label):
    out = set()
    m = V == label
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        out |= set(V[tuple(b)][m[tuple(a)]].tolist()) | set(V[tuple(a)][m[tuple(b)]].tolist())
    out.discard(int(label))
    return out


def test_a_split_that_does_not_fit_uint16_raises_and_leaves_the_image():
    V = synth.voronoi_labels((20, 24, 70), 60, 3, dtype=np.uint16)
    top = int(V.max())
    V[V == top] = 65535                                                          # the largest label is the dtype's last value
    rows, _ = ref.table(V)
    assert rows[0].size > np.unique(rows[0]).size and rows[0].max() == 65535
    sia = SpatialImageAnalysis(SpatialImage(V.copy()), ignoredlabels=0, background=1, return_type=DICT)
    with pytest.raises(ValueError):
        sia.split_disconnected_labels()
    assert np.array_equal(np.asarray(sia.image), V)
    same_rows(sia.label_components(), rows)                                      # and the resident volume is what it was
    back = np.empty_like(V)
    assert np.array_equal(sia._resident().ctx.get_volume(back), V)
