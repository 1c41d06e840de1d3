"""The label-overlap table on the MI355X (include/tissue_scan_overlap.h, csrc/kernels_overlap.hip) against the NumPy restatement
of tests/overlap_reference.py: every number is an integer and must be bit-exact."""
import numpy as np
import pytest

import overlap_reference as ref
from tissue_analysis_amd import (DICT, LabelOverlap, SpatialImageAnalysis, _capi, label_overlap, lineage_from_images, synth)
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu


def check_table(ov, A, B):
    """ov: LabelOverlap of the label images A and B (any layout, 2-D or 3-D)."""
    assert isinstance(ov, LabelOverlap)
    a, b, n = ref.table(A, B)
    assert ov.a.dtype == np.int64 and ov.b.dtype == np.int64 and ov.n.dtype == np.uint64
    assert np.array_equal(ov.a, a) and np.array_equal(ov.b, b) and np.array_equal(ov.n, n)
    assert int(ov.n.sum()) == A.size


def _run(A, B, capacity=0):
    rv = ResidentVolume(A)
    try:
        rv.ctx.set_overlap_capacity(capacity)
        ov = rv.overlap(B)
        _, passes = rv.ctx.overlap_timing_compaction()
        assert ov.ms is not None and ov.ms > 0.0
    finally:
        rv.close()
    return ov, passes


def _frames(dims, da, db, cells=(60, 45), seeds=(3, 4)):
    A = synth.voronoi_labels(dims, cells[0], seeds[0], dtype=np.uint16).astype(da)
    B = synth.voronoi_labels(dims, cells[1], seeds[1], dtype=np.uint16).astype(db)
    return A, B


@pytest.mark.parametrize("da", [np.uint16, np.uint32])
@pytest.mark.parametrize("db", [np.uint16, np.uint32])
def test_label_types_and_edge_tiles(da, db):
    # a tile is 4 rows x 512 (uint16) or 256 (uint32) columns x 16 planes: partial tiles in every axis; rows of 531 voxels are
    # not a multiple of the strip width (the scalar-load path), rows of 528 are (the vector-load path)
    for dims in ((19, 7, 531), (19, 7, 528), (33, 10, 264)):
        A, B = _frames(dims, da, db)
        check_table(_run(A, B)[0], A, B)


def test_single_plane_single_row_and_two_dimensional_images():
    for dims in ((1, 9, 40), (1, 1, 77), (5, 1, 64), (1, 1, 1)):
        A, B = _frames(dims, np.uint16, np.uint32, cells=(6, 4))
        check_table(_run(A, B)[0], A, B)
    A, B = _frames((1, 200, 150), np.uint16, np.uint16, cells=(40, 30))
    A, B = A[0], B[0]
    check_table(_run(A, B)[0], A, B)
    check_table(label_overlap(A.astype(np.int64), B.astype(np.int32)), A, B)


def test_dense_layouts_other_than_c_order():
    A, B = _frames((24, 40, 56), np.uint16, np.uint32)
    AF, BF = np.asfortranarray(A), np.asfortranarray(B)
    check_table(_run(AF, BF)[0], A, B)
    AT, BT = A.transpose(1, 2, 0), B.transpose(1, 2, 0)           # a third axis permutation, shared by both
    check_table(_run(AT, BT)[0], AT, BT)
    check_table(_run(AF, B)[0], A, B)                             # B in another layout than A: copied into A's on the host
    check_table(_run(A, BF)[0], A, B)


def test_a_volume_against_itself_is_the_diagonal_and_margins_are_the_sweep_counts():
    c = synth.CONFIGS["C1"]
    A = synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], np.uint16)
    B = synth.voronoi_labels(c["dims"], 150, 9, np.uint16).astype(np.uint32)
    rv, rb = ResidentVolume(A), ResidentVolume(B)
    try:
        xa, xb = rv.extract(), rb.extract()
        diag = rv.overlap(A)
        ov = rv.overlap(B)
    finally:
        rv.close()
        rb.close()
    ids = np.flatnonzero(xa.count)
    assert np.array_equal(diag.a, ids) and np.array_equal(diag.b, ids) and np.array_equal(diag.n, xa.count[ids])
    check_table(ov, A, B)
    assert np.array_equal(ov.size_a[0], ids) and np.array_equal(ov.size_a[1], xa.count[ids])
    idb = np.flatnonzero(xb.count)
    assert np.array_equal(ov.size_b[0], idb) and np.array_equal(ov.size_b[1], xb.count[idb])


def test_sparse_ids_on_either_side_and_a_compacted_context():
    rng = np.random.default_rng(5)
    ids = np.array([0, 7, 70000, 2**31 + 5, 2**32 - 2, 2**32 - 1], dtype=np.uint32)
    A = ids[rng.integers(0, ids.size, size=(12, 9, 33))]
    B = ids[::-1][rng.integers(0, ids.size, size=(12, 9, 33))]
    ov, _ = _run(A, B)
    check_table(ov, A, B)
    assert ov.between(2**32 - 1, 2**32 - 1) > 0 and ov.a[-1] == 2**32 - 1 and ov.b[-1] == 2**32 - 1
    small = (np.arange(A.size).reshape(A.shape) % 5).astype(np.uint16)
    check_table(_run(A, small)[0], A, small)
    check_table(_run(small, B)[0], small, B)
    top = np.full((3, 4, 8), 2**32 - 1, dtype=np.uint32)           # nothing but the pair of the two largest ids
    check_table(_run(top, top)[0], top, top)
    rv = ResidentVolume(A)
    try:
        x = rv.extract(sparse=True)
        assert rv.ctx.is_compact() and x.ids is not None
        check_table(rv.overlap(B), A, B)                            # rows of the sweep are ranks, the table speaks in ids
        rv.ctx.uncompact()
        check_table(rv.overlap(B), A, B)
    finally:
        rv.close()


def test_noise_and_a_table_that_starts_too_small():
    rng = np.random.default_rng(11)
    A = rng.integers(0, 4000, size=(64, 64, 64)).astype(np.uint16)
    B = rng.integers(0, 4000, size=(64, 64, 64)).astype(np.uint32)
    ov, passes = _run(A, B)
    check_table(ov, A, B)
    assert len(ov) > 250000 and passes >= 1
    ov, passes = _run(A, B, capacity=4)                            # 16 slots for 2.6e5 pairs: the overflow path
    check_table(ov, A, B)
    assert passes > 1
    A2, B2 = _frames((40, 40, 40), np.uint16, np.uint16)
    ov, passes = _run(A2, B2, capacity=6)
    check_table(ov, A2, B2)
    assert passes > 1


@pytest.mark.parametrize("cuts", [(37,), (20, 41)])
def test_slabs_with_a_low_halo_merge_to_the_whole(cuts):
    import torch
    c = synth.CONFIGS["C1"]
    A = synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], np.uint16)
    B = synth.voronoi_labels(c["dims"], 170, 21, np.uint16).astype(np.uint32)
    edges = (0,) + tuple(cuts) + (A.shape[0],)
    parts = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        halo = lo > 0
        lo_ = lo - 1 if halo else lo
        ta = torch.from_numpy(A[lo_:hi].view(np.int16).copy()).cuda()
        tb = torch.from_numpy(B[lo_:hi].view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        ctx = _capi.Context(0)
        try:
            ctx.set_volume_device(ta.data_ptr(), 2, ta.shape, a0_origin=lo, has_low_halo=halo, keep=ta)
            ctx.set_overlap_device(tb.data_ptr(), 4, keep=tb)
            ctx.overlap_extract()
            a, b, n = ctx.overlap_get()
        finally:
            ctx.close()
        want = ref.table(A[lo_:hi], B[lo_:hi], first_owned=1 if halo else 0)
        assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(n, want[2])
        parts.append((a.astype(np.int64), b.astype(np.int64), n))
    for got, want in zip(ref.merge(parts), ref.table(A, B)):
        assert np.array_equal(got, want)


def test_a_cuda_tensor_as_second_volume():
    import torch
    A, B = _frames((24, 40, 56), np.uint32, np.uint16)
    tb = torch.from_numpy(B.view(np.int16).copy()).cuda()
    torch.cuda.synchronize()
    rv = ResidentVolume(A)
    try:
        check_table(rv.overlap(tb), A, B)
        with pytest.raises(ValueError):
            rv.overlap(tb[:, :, :48].contiguous())
    finally:
        rv.close()


def _einval(call, *args):
    with pytest.raises(_capi.TissueScanError) as e:
        call(*args)
    assert e.value.code == _capi.TA_EINVAL


def test_argument_checks_and_invalidation():
    A, B = _frames((10, 12, 40), np.uint16, np.uint16)
    ctx = _capi.Context(0)
    try:
        _einval(ctx.overlap_extract)                                # no volume
        ctx.set_volume(A)
        _einval(ctx.overlap_extract)                                # no B
        _einval(ctx.overlap_size)
        lib, h = ctx._lib, ctx._h
        i64x3 = _capi._i64x3
        other = np.ascontiguousarray(B[:, :, :39])
        assert lib.ta_overlap_set(h, other.ctypes.data, 2, i64x3(other.shape), i64x3(other.strides)) == _capi.TA_EINVAL     # dims
        BF = np.asfortranarray(B)
        assert lib.ta_overlap_set(h, BF.ctypes.data, 2, i64x3(BF.shape), i64x3(BF.strides)) == _capi.TA_EINVAL             # layout
        assert lib.ta_overlap_set(h, B.ctypes.data, 1, i64x3(B.shape), i64x3(B.strides)) == _capi.TA_EINVAL                 # itemsize
        assert lib.ta_overlap_set_capacity(h, 3) == _capi.TA_EINVAL and lib.ta_overlap_set_capacity(h, 32) == _capi.TA_EINVAL
        ctx.set_overlap(B)
        _einval(ctx.overlap_get)                                    # B, but no pass yet
        ctx.overlap_extract()
        a, b, n = ctx.overlap_get()
        want = ref.table(A, B)
        assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(n, want[2])
        assert lib.ta_overlap_get(h, None, None, None) == _capi.TA_OK           # any pointer may be NULL
        ctx.set_overlap(B)                                          # a new B
        _einval(ctx.overlap_size)
        _einval(ctx.overlap_get)
        ctx.overlap_extract()
        assert ctx.overlap_size() == want[0].size
        lut = np.arange(int(A.max()) + 1, dtype=np.uint32)
        lut[2:] += 100
        ctx.relabel(lut)                                            # ta_volume_relabel
        _einval(ctx.overlap_size)
        _einval(ctx.overlap_get)
        ctx.overlap_extract()
        a, b, n = ctx.overlap_get()
        want = ref.table(lut[A], B)
        assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(n, want[2])
        ctx.set_volume(A)                                           # a new volume of the same dims keeps B
        _einval(ctx.overlap_size)
        ctx.overlap_extract()
        assert ctx.overlap_size() == ref.table(A, B)[0].size
        ctx.set_volume(np.ascontiguousarray(A[:, :, :32]))          # other dims: B is dropped
        _einval(ctx.overlap_extract)
    finally:
        ctx.close()


def test_analysis_and_module_functions_on_a_constructed_division():
    A, B, truth = ref.division_fixture()
    a, b, n = ref.table(A, B)
    sia = SpatialImageAnalysis(A, background=1, return_type=DICT)
    ov = sia.overlap(B)
    check_table(ov, A, B)
    assert len(ov) == 223                                           # nothing is excluded by the analysis itself
    lin = ov.lineage(0.5, exclude=(0, sia.background()))
    assert dict((d, m) for m, ds in lin.items() for d in ds) == truth and len(truth) == 222
    assert lin == ref.lineage(a, b, n, 0.5, (0, 1))
    check_table(label_overlap(A, B), A, B)
    assert lineage_from_images(A, B) == lin
    assert np.array_equal(ov.jaccard(), ref.jaccard(a, b, n))
    Bs = ref.shifted(B, (1, 2, 1))
    sa, sb, sn = ref.table(A, Bs)
    assert lineage_from_images(A, Bs, min_fraction=0.5, background=1) == ref.lineage(sa, sb, sn, 0.5, (0, 1))
    assert lineage_from_images(A, Bs, min_fraction=0.3, background=None) == ref.lineage(sa, sb, sn, 0.3, (0,))


def test_full_size_512_cubed_against_numpy_unique():
    import torch
    from tissue_analysis_amd import device as dev
    c = synth.CONFIGS["C2"]
    dtype = np.dtype("uint16")
    ctx = dev.torch_context(0)
    try:
        va, _ = dev.synth_slab(ctx, c["dims"], dtype, c["n_cells"], c["seed"])
        vb, _ = dev.synth_slab(ctx, c["dims"], dtype, c["n_cells"], c["seed"] + 100)
        torch.cuda.synchronize()
        ctx.set_volume_device(va.data_ptr(), 2, va.shape, keep=va)
        ctx.set_overlap_device(vb.data_ptr(), 2, keep=vb)
        ctx.overlap_extract()
        a, b, n = ctx.overlap_get()
        A, B = va.cpu().numpy().view(dtype), vb.cpu().numpy().view(dtype)
    finally:
        ctx.close()
    check_table(LabelOverlap(a, b, n), A, B)
