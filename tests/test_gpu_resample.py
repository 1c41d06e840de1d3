"""The gather pass of include/tissue_scan_resample.h on the GPU: EXACT equality, of the output and of `outside`, with the NumPy
restatement (tests/resample_reference.py) over source types, modes, target shapes on both store paths and the maps that can go
wrong (ties, the rounding order, borders, everything outside); the error answers; the composition with the overlap and the
signal passes; slabs; a misaligned device source; the launch plan.  Every case is a few thousand to a few hundred thousand voxels."""
import functools

import numpy as np
import pytest

import overlap_reference
import resample_reference as ref
from tissue_analysis_amd import DICT, SpatialImage, SpatialImageAnalysis, _capi, index_matrix, lineage_from_images, synth
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu

EYE = np.eye(4)[:3]
TORCH_VIEW = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}


def affine(diag=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0)):
    A = np.zeros((3, 4))
    A[:, :3] = np.diag(diag)
    A[:, 3] = offset
    return A


def flip_and_permute(m):
    """s0 = i1, s1 = (m1 - 1) - i0, s2 = (m2 - 1) - i2: entries +-1, offsets m - 1."""
    A = np.zeros((3, 4))
    A[0, 1] = 1.0
    A[1, 0], A[1, 3] = -1.0, m[1] - 1
    A[2, 2], A[2, 3] = -1.0, m[2] - 1
    return A


def planar_rotation():
    c, s = np.cos(0.4), np.sin(0.4)
    return np.array([[0.8 * c, -0.8 * s, 0.0, 1.2], [0.8 * s, 0.8 * c, 0.0, -0.9], [0.0, 0.0, 1.0, 0.0]])


def contraction_axis():
    """Source axis 2 reads s = (0.1 i0 + 0 i1) + 0.3 i2 + 0: in target plane i0 = 1 that is 0.1 + 0.3 i2, and at i2 = 18 and 48 a
    fused multiply-add of 0.3 i2 into the sum before it lands ON the tie and goes up, while the stated order stays just below it
    (test_resample_cpu.py shows it in rational arithmetic).  The 0.1 stands in a product term, not in the offset column: the
    offset is added last, by a plain addition that no compiler can fuse with the product two steps earlier."""
    A = EYE.copy()
    A[2, 0], A[2, 2] = 0.1, 0.3
    return A


# name: (target shape, source shape, map).  Rows of 70 and 1100 voxels are no whole strips of any type (the scalar stores); 64 and
# 1104 are whole strips of all three (one 16-byte store a lane); 1100 and 1104 columns are three column tiles of a uint16 volume
CASES = {
    "rotation-scalar": ((5, 7, 70), (6, 9, 24), ref.rotation_with_scales()),
    "rotation-vector": ((4, 6, 64), (6, 9, 24), ref.rotation_with_scales()),
    "three-column-tiles-scalar": ((3, 5, 1100), (4, 6, 300), affine((0.9, 1.1, 0.27), (0.2, -0.3, 1.6))),
    "three-column-tiles-vector": ((3, 5, 1104), (4, 6, 300), affine((0.9, 1.1, 0.27), (0.2, -0.3, 1.6))),
    "2d-image": ((9, 11, 1), (7, 8, 1), planar_rotation()),
    "one-voxel-source": ((4, 6, 64), (1, 1, 1), affine((0.2, 0.1, 0.01), (-0.3, 0.0, -0.2))),
    "identity": ((4, 6, 64), (4, 6, 64), EYE),
    "integer-translation": ((4, 6, 64), (4, 6, 64), affine(offset=(1.0, -2.0, 5.0))),
    "flip-and-permute": ((6, 4, 64), (4, 6, 64), flip_and_permute((4, 6, 64))),
    "zoom-2": ((8, 12, 32), (4, 6, 16), affine((0.5, 0.5, 0.5))),
    "zoom-half": ((4, 6, 16), (8, 12, 32), affine((2.0, 2.0, 2.0))),
    "half-integer-translation": ((4, 6, 64), (4, 6, 64), affine(offset=(0.5, 0.5, 0.5))),
    "contraction-sensitive-axis": ((2, 3, 64), (2, 3, 20), contraction_axis()),
    "everything-outside": ((4, 6, 64), (4, 6, 64), affine(offset=(1000.0, 0.0, 0.0))),
    "border-band": ((5, 7, 70), (5, 7, 70), affine(offset=(-0.25, 0.3, -0.4))),
}
TYPES = [(np.uint8, ref.NEAREST), (np.uint16, ref.NEAREST), (np.uint32, ref.NEAREST), (np.uint8, ref.LINEAR), (np.uint16, ref.LINEAR)]
TYPE_IDS = ["u8-nearest", "u16-nearest", "u32-nearest", "u8-linear", "u16-linear"]
FILL = 0xA1B2C3D4          # (truncated to the type: 0xD4, 0xC3D4)


@functools.lru_cache(maxsize=None)
def source(shape, dtype):
    S = ref.random_source(shape, dtype)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def expected(name, dtype, mode):
    shape, sshape, A = CASES[name]
    out, filled = ref.resample(source(sshape, dtype), A, shape, mode, FILL)
    out.setflags(write=False)
    return out, ref.outside(filled)


@pytest.fixture(scope="module")
def ctx():
    c = _capi.Context(0)
    yield c
    c.close()


def labels_of(shape, dtype):
    return (np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape) % 37).astype(dtype)


def run(ctx, S, A, mode, fill=FILL):
    ctx.set_resample_source(S)
    ctx.resample_extract(A, mode, fill)
    return ctx.resample_get().reshape(ctx._vol_layout[0]), ctx.resample_outside()


@pytest.mark.parametrize("dtype,mode", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_output_and_outside_equal_the_restatement(ctx, name, dtype, mode):
    shape, sshape, A = CASES[name]
    ctx.set_volume(labels_of(shape, np.uint16))
    got, outside = run(ctx, source(sshape, dtype), A, mode)
    want, want_outside = expected(name, dtype, mode)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert outside == want_outside
    d = ctx.resample_debug()
    mdims = tuple(shape[a] for a in ctx.memory_axes())            # (a size-1 axis is the slowest in memory: the 2-D image is 1 x 9 x 11)
    assert d["vector"] == (mdims[2] % (16 // np.dtype(dtype).itemsize) == 0) and d["mode"] == mode
    assert (d["tiles_per_group"], d["groups"]) == ref.plan(mdims, np.dtype(dtype).itemsize)[4:]
    assert ctx.resample_timing() >= 0.0


def test_the_cases_hold_what_they_are_named_for():
    """(no GPU work: the restatement's outputs have the properties the case names promise, so no case passes vacuously)"""
    S = source((4, 6, 64), np.uint16)
    out, n = expected("identity", np.uint16, ref.NEAREST)
    assert np.array_equal(out, S) and n == 0
    out, n = expected("identity", np.uint16, ref.LINEAR)
    assert np.array_equal(out, S) and n == 0
    out, n = expected("everything-outside", np.uint16, ref.NEAREST)
    assert (out == 0xC3D4).all() and n == 4 * 6 * 64
    out, n = expected("half-integer-translation", np.uint16, ref.NEAREST)
    assert np.array_equal(out[:-1, :-1, :-1], S[1:, 1:, 1:]) and n == 4 * 6 * 64 - 3 * 5 * 63          # ties go up
    out, _ = expected("integer-translation", np.uint16, ref.NEAREST)
    assert np.array_equal(out[:3, 2:, :59], S[1:, :4, 5:])
    out, n = expected("flip-and-permute", np.uint16, ref.NEAREST)
    assert np.array_equal(out, np.transpose(S, (1, 0, 2))[::-1, :, ::-1]) and n == 0
    out, _ = expected("contraction-sensitive-axis", np.uint16, ref.NEAREST)
    Sc = source((2, 3, 20), np.uint16)
    assert np.array_equal(out[1, :, 18], Sc[1, :, 5]) and np.array_equal(out[1, :, 48], Sc[1, :, 14])
    assert not np.array_equal(Sc[1, :, 5], Sc[1, :, 6]) and not np.array_equal(Sc[1, :, 14], Sc[1, :, 15])   # a fused kernel differs
    s = ref.source_index(CASES["border-band"][2], (5, 7, 70))
    assert (s[0] < 0).any() and (s[1] > 6).any() and (s[2] < 0).any()            # the clamped corners are used on both sides
    assert expected("border-band", np.uint8, ref.LINEAR)[1] == 0
    assert 0 < expected("one-voxel-source", np.uint8, ref.LINEAR)[1] < 4 * 6 * 64


@pytest.mark.parametrize("label_dtype", [np.uint16, np.uint32])
def test_label_type_of_the_target_does_not_matter(ctx, label_dtype):
    shape, sshape, A = CASES["rotation-scalar"]
    ctx.set_volume(labels_of(shape, label_dtype))
    for dtype, mode in TYPES:
        got, outside = run(ctx, source(sshape, dtype), A, mode)
        want, want_outside = expected("rotation-scalar", dtype, mode)
        assert np.array_equal(got, want) and outside == want_outside


def test_permuted_layouts_of_target_and_source(ctx):
    """A label volume and a source stored in other axis orders: the map speaks array axes whatever the memory order."""
    shape, sshape, A = CASES["rotation-scalar"]
    V = np.asfortranarray(labels_of(shape, np.uint16))
    S = np.ascontiguousarray(np.transpose(source(sshape, np.uint16), (1, 2, 0))).transpose(2, 0, 1)
    assert np.array_equal(S, source(sshape, np.uint16)) and not S.flags.c_contiguous
    rv = ResidentVolume(V)
    try:
        for mode in (ref.NEAREST, ref.LINEAR):
            r = rv.resample(S, A, order=mode, fill=FILL)
            want, want_outside = expected("rotation-scalar", np.uint16, mode)
            assert np.array_equal(r.image(), want) and r.outside == want_outside
    finally:
        rv.close()


def einval(call, *args):
    with pytest.raises(_capi.TissueScanError) as e:
        call(*args)
    assert e.value.code == _capi.TA_EINVAL
    return str(e.value)


def test_error_answers(ctx):
    shape = (4, 6, 64)
    ctx.set_volume(labels_of(shape, np.uint16))
    ctx.set_resample_source(source(shape, np.uint32))
    for bad in (np.nan, np.inf, -np.inf):
        A = EYE.copy()
        A[1, 3] = bad
        assert "finite" in einval(ctx.resample_extract, A, ref.NEAREST)
    einval(ctx.resample_extract, EYE, ref.LINEAR)                 # linear mode on a 4-byte source
    einval(ctx.resample_extract, EYE, 2)
    ctx.resample_extract(EYE, ref.NEAREST)
    einval(ctx.resample_as_signal)                                # a 4-byte result is no signal
    ctx.resample_as_overlap()
    ctx.set_resample_source(source(shape, np.uint8))
    einval(ctx.resample_outside)                                  # a new source: the old result is gone
    ctx.resample_extract(EYE, ref.NEAREST)
    einval(ctx.resample_as_overlap)                               # a 1-byte result is no label volume
    ctx.resample_as_signal()
    ctx.resample_extract(EYE, ref.LINEAR)
    einval(ctx.resample_as_overlap)                               # an interpolated volume is no label volume
    assert ctx.resample_outside() == 0
    ctx.set_volume(labels_of((4, 6, 60), np.uint16))              # a new volume of other dims drops source and result
    for getter in (ctx.resample_outside, ctx.resample_timing, ctx.resample_debug, ctx.resample_device, ctx.resample_as_signal):
        einval(getter)
    assert "source" in einval(ctx.resample_extract, EYE, ref.NEAREST)
    lib = _capi.load()
    assert lib.ta_resample_get(ctx._h, None, 0, 1) == _capi.TA_EINVAL
    fresh = _capi.Context(0)
    try:
        fresh.set_resample_source(source(shape, np.uint16))        # (a source needs no label volume; a pass does)
        assert "label volume" in einval(fresh.resample_extract, EYE, ref.NEAREST)
    finally:
        fresh.close()


# ---- composition with the existing passes

@functools.lru_cache(maxsize=None)
def frames():
    A, B, truth = overlap_reference.division_fixture(dims=(40, 44, 48), n_cells=30, seed=7)
    return A, B, truth


def test_overlap_with_a_matrix_equals_overlap_of_the_restated_volume():
    A, B, _ = frames()
    Bsrc = np.ascontiguousarray(B[2:37, :40, 3:45])               # another shape: a crop, seen through a rotation with scales
    c, s = np.cos(0.2), np.sin(0.2)
    M = np.array([[0.95 * c, -0.95 * s, 0.0, 1.5], [0.95 * s, 0.95 * c, 0.0, -4.0], [0.0, 0.0, 0.9, -2.25]])
    restated, filled = ref.resample(Bsrc, M, A.shape, ref.NEAREST, fill=1)
    rv = ResidentVolume(A)
    try:
        got = rv.overlap(Bsrc, matrix=M, fill=1)
        want = rv.overlap(restated)
    finally:
        rv.close()
    assert len(got) == len(want) > 30
    assert np.array_equal(got.a, want.a) and np.array_equal(got.b, want.b) and np.array_equal(got.n, want.n)
    assert got.outside == ref.outside(filled) > 0 and int(got.n.sum()) == A.size
    a, b, n = overlap_reference.table(A, restated)
    assert np.array_equal(got.a, a) and np.array_equal(got.b, b) and np.array_equal(got.n, n)


def test_a_second_resample_invalidates_the_adopted_overlap_table(ctx):
    A, B, _ = frames()
    ctx.set_volume(A)
    ctx.set_resample_source(B)
    ctx.resample_extract(EYE, ref.NEAREST)
    ctx.resample_as_overlap()
    ctx.overlap_extract()
    a, b, n = ctx.overlap_get()
    want = overlap_reference.table(A, B)
    assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(n, want[2])
    shift = affine(offset=(1.0, 2.0, 1.0))
    ctx.resample_extract(shift, ref.NEAREST, 1)                   # new contents in the adopted buffer
    einval(ctx.overlap_size)
    einval(ctx.overlap_get)
    ctx.overlap_extract()                                         # B is still adopted: the table of the new contents
    a, b, n = ctx.overlap_get()
    want = overlap_reference.table(A, ref.resample(B, shift, A.shape, ref.NEAREST, 1)[0])
    assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(n, want[2])
    ctx.set_resample_source(B.astype(np.uint16) if B.max() < 65536 else (B & 0xFFFF).astype(np.uint16))
    ctx.resample_extract(EYE, ref.NEAREST)                        # another item size: the adopted B is gone
    assert "second label volume" in einval(ctx.overlap_extract)


def test_cell_signal_with_a_transform_equals_cell_signal_of_the_restated_image():
    V = synth.voronoi_labels((24, 28, 40), 20, 3, dtype=np.uint16)
    vs_t, vs_s = (0.5, 0.5, 1.0), (0.4, 0.6, 1.5)
    S = source((33, 25, 30), np.uint8)
    T = np.eye(4)
    c, s = np.cos(0.15), np.sin(0.15)
    T[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = (0.7, -1.1, 2.0)
    M = index_matrix(T, vs_t, vs_s)
    restated, filled = ref.resample(S, M, V.shape, ref.LINEAR, 0)
    assert 0 < ref.outside(filled) < V.size // 2
    sia = SpatialImageAnalysis(SpatialImage(V, voxelsize=vs_t), background=1, return_type=DICT)
    same = np.testing.assert_equal               # (exact, NaN equal to NaN, through the dicts)
    for stat in ("mean", "sum", "max"):
        want = sia.cell_signal(restated, statistic=stat)
        assert len(want) > 10
        same(sia.cell_signal(SpatialImage(S, voxelsize=vs_s), statistic=stat, transform=T), want)
        same(sia.cell_signal(S, statistic=stat, transform=T, voxelsize=vs_s), want)
    same(sia.signal_median(S, transform=T, voxelsize=vs_s), sia.signal_median(restated))
    same(sia.wall_signal(S, transform=T, voxelsize=vs_s), sia.wall_signal(restated))
    on_grid = sia.resample_onto_grid(SpatialImage(S, voxelsize=vs_s), transform=T, order=1)
    assert np.array_equal(np.asarray(on_grid), restated) and tuple(on_grid.voxelsize) == vs_t
    same(sia.cell_signal(on_grid), sia.cell_signal(restated, statistic="mean"))


def test_lineage_from_images_recovers_the_lineage_through_a_translation():
    A, B, truth = frames()
    want = lineage_from_images(A, B)
    assert dict((d, m) for m, ds in want.items() for d in ds) == truth
    # frame t+1 on a larger grid of voxels half as wide along axis 2, the tissue moved by (1, 2, 3) voxels of frame t
    pad = np.pad(B, ((1, 2), (2, 0), (3, 5)), constant_values=1)
    wide = np.repeat(pad, 2, axis=2)
    assert wide.shape != A.shape
    T = np.eye(4)
    T[:3, 3] = (1.0, 2.0, 3.0 + 0.25)            # (+ 0.25: index 2 i + 6.5, the second of the two half-voxels, not a tie)
    got = lineage_from_images(A, wide, transform=T, voxelsize_t0=(1.0, 1.0, 1.0), voxelsize_t1=(1.0, 1.0, 0.5))
    assert got == want


def test_tensor_is_a_view_of_the_result_on_the_device():
    import torch
    shape, sshape, A = CASES["rotation-vector"]
    rv = ResidentVolume(labels_of(shape, np.uint32))
    try:
        S = torch.from_numpy(source(sshape, np.uint16).view(np.int16).copy()).to("cuda:0")
        r = rv.resample(S, A, order=0, fill=FILL)
        want, want_outside = expected("rotation-vector", np.uint16, ref.NEAREST)
        t = r.tensor()
        assert t.is_cuda and tuple(t.shape) == shape and t.data_ptr() == rv.ctx.resample_device()[0]
        assert np.array_equal(t.cpu().numpy().view(np.uint16), want) and np.array_equal(r.image(), want)
        assert r.outside == want_outside and r.ms >= 0.0
        rv.resample(S, A, order=1)
        with pytest.raises(ValueError):
            r.image()                            # resampled again: the first object is stale
    finally:
        rv.close()


# ---- slabs, a misaligned source, the launch plan

def test_slabs_concatenate_to_the_whole_volume(ctx):
    import torch
    shape, sshape = (9, 7, 70), (6, 9, 24)
    A = ref.rotation_with_scales()
    A[0, 0], A[0, 3] = 0.55, -0.8                # (the source spans the nine planes, and plane 0 lies outside it)
    V = labels_of(shape, np.uint16)
    for dtype, mode in ((np.uint16, ref.NEAREST), (np.uint8, ref.LINEAR)):
        S = source(sshape, dtype)
        whole, filled = ref.resample(S, A, shape, mode, FILL)
        cut = 4
        parts, outside = [], []
        for lo, hi, halo in ((0, cut, False), (cut, shape[0], True)):
            buf = np.ascontiguousarray(V[lo - (1 if halo else 0):hi])
            dev = torch.from_numpy(buf.view(np.int16)).to("cuda:0")
            ctx.set_volume_device(dev.data_ptr(), 2, buf.shape, a0_origin=lo, has_low_halo=halo, keep=dev)
            got, n = run(ctx, S, A, mode)
            assert got.shape == buf.shape
            if halo:
                assert np.array_equal(got[0], whole[lo - 1])          # the halo plane is written ...
                got = got[1:]
            parts.append(got)
            outside.append(n)
            assert n == ref.outside(filled[lo:hi])                      # ... and not counted
        assert np.array_equal(np.concatenate(parts), whole)
        assert sum(outside) == ref.outside(filled) and filled[cut - 1].any()
    ctx.set_volume(labels_of((2, 2, 2), np.uint16))                     # (lets go of the tensors)


@pytest.mark.parametrize("dtype,mode,off", [(np.uint16, ref.NEAREST, 2), (np.uint32, ref.NEAREST, 1), (np.uint8, ref.LINEAR, 4),
                                            (np.uint16, ref.LINEAR, 2), (np.uint16, ref.NEAREST, 0)],
                         ids=["u16-nearest+4B", "u32-nearest+4B", "u8-linear+4B", "u16-linear+4B", "u16-nearest+0B"])
def test_device_source_off_a_16_byte_boundary(ctx, dtype, mode, off):
    """A device source 4 bytes past a 16-byte boundary (a view into a larger tensor) gives the same answer; offset 0 is the control."""
    import torch
    shape, sshape, A = CASES["rotation-vector"]
    S = source(sshape, dtype)
    host = np.zeros(off + S.size + 5, dtype=dtype)
    host[off:off + S.size] = S.reshape(-1)
    flat = torch.from_numpy(host.view(TORCH_VIEW[np.dtype(dtype)])).to("cuda:0")
    ptr = int(flat.data_ptr()) + off * S.dtype.itemsize
    assert int(flat.data_ptr()) % 256 == 0 and ptr % 16 == (4 if off else 0)
    ctx.set_volume(labels_of(shape, np.uint16))
    ctx.set_resample_source_device(ptr, S.dtype.itemsize, sshape, keep=flat)
    ctx.resample_extract(A, mode, FILL)
    want, want_outside = expected("rotation-vector", dtype, mode)
    assert np.array_equal(ctx.resample_get().reshape(shape), want) and ctx.resample_outside() == want_outside
    assert ctx.resample_debug()["vector"]
    ctx.set_resample_source(S)                                          # (lets go of the tensor)


def test_launch_plan_covers_every_tile_once(ctx):
    """200 x 400 x 4 uint16 is 5000 tiles of 4 planes x 4 rows, more than the 4096 workgroups of a launch: every workgroup takes
    two.  The plan the device reports is the restatement's, it covers every tile once, and every voxel has its value."""
    shape = (200, 400, 4)
    ncb, nrb, npb, tiles, per, groups = ref.plan(shape, 2)
    assert (tiles, per, groups) == (5000, 2, 2500)
    ctx.set_volume(labels_of(shape, np.uint16))
    S = source((90, 170, 9), np.uint16)
    A = affine((0.45, 0.43, 2.1), (-0.3, -0.2, 0.2))
    got, outside = run(ctx, S, A, ref.NEAREST)
    d = ctx.resample_debug()
    assert (d["tiles_per_group"], d["groups"]) == (per, groups) and not d["vector"]
    assert (d["groups"] - 1) * d["tiles_per_group"] < tiles <= d["groups"] * d["tiles_per_group"]
    want, filled = ref.resample(S, A, shape, ref.NEAREST, FILL)
    assert np.array_equal(got, want) and outside == ref.outside(filled) > 0
    # the same volume with a halo plane in front: the halo plane is tiled too (201 planes: 51 plane blocks)
    import torch
    buf = labels_of((201, 400, 4), np.uint16)
    dev = torch.from_numpy(buf.view(np.int16)).to("cuda:0")
    ctx.set_volume_device(dev.data_ptr(), 2, buf.shape, a0_origin=1, has_low_halo=True, keep=dev)
    got, outside = run(ctx, S, A, ref.NEAREST)
    d = ctx.resample_debug()
    assert (d["tiles_per_group"], d["groups"]) == ref.plan(buf.shape, 2)[4:] == (2, 2550)
    want, filled = ref.resample(S, A, buf.shape, ref.NEAREST, FILL)      # (buffer plane 0 is global plane 0)
    assert np.array_equal(got, want) and outside == ref.outside(filled, first_owned=1)
    ctx.set_volume(labels_of((2, 2, 2), np.uint16))
