"""Oriented extents without a GPU: include/tissue_scan_extents.h against the binding and the library, the constants of
tests/extent_reference.py against the sources, the restatement against a fused evaluation, and `CellExtents` on rows injected from
the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

import extent_reference as ref
import range_tiles as rt
from tissue_analysis_amd import CellExtents, _capi, build
from tissue_analysis_amd.cell_extents import complete_frame, extent_weights, unit_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tissue_analysis_amd", "csrc")


def _header():
    return open(os.path.join(ROOT, "include", "tissue_scan_extents.h")).read()


def test_header_and_binding_declare_the_same_symbols():
    text = _header()
    declared = sorted(re.findall(r"TA_API\s+int\s+(ta_\w+)\s*\(", text))
    assert declared == sorted(_capi.EXTENT_SYMBOLS) and len(declared) == 4
    assert not set(_capi.EXTENT_SYMBOLS) & set(_capi.SYMBOLS)
    assert re.search(r"TA_API\s+int\s+ta_extents_debug\s*\(ta_ctx\*\s*ctx,\s*uint32_t\s+out\[4\]\)", text)
    assert [h for h, names in _capi.DECLARED.items() if "ta_extents_get" in names] == ["tissue_scan_extents.h"]


def test_library_exports_the_symbols_and_keeps_its_version():
    lib = _capi.load()
    for name in _capi.EXTENT_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.ta_version() == 5 == _capi.ABI_VERSION


def test_null_context_is_refused():
    lib = _capi.load()
    w = (ctypes.c_double * 9)(*([1.0] * 9))
    assert lib.ta_extents_extract(None, w, 1) == _capi.TA_EINVAL
    assert b"NULL" in lib.ta_last_error()
    assert lib.ta_extents_get(None, None, None) == _capi.TA_EINVAL
    out = (ctypes.c_uint32 * 4)()
    assert lib.ta_extents_debug(None, out) == _capi.TA_EINVAL and list(out) == [0, 0, 0, 0]
    ms = ctypes.c_double(-1.0)
    assert lib.ta_extents_timing(None, ctypes.byref(ms)) == _capi.TA_EINVAL and ms.value == -1.0


def _constant(path, name):
    return int(re.search(r"\b%s\s*=\s*(\d+)" % name, open(os.path.join(CSRC, path)).read()).group(1))


def test_restated_constants_are_those_of_the_sources():
    assert _constant("ta_extents.h", "EX_SLOTS") == ref.LABEL_SLOTS == _capi.EXTENT_SLOTS
    assert _constant("ta_extents.h", "EX_MAX_GROUPS") == ref.MAX_GROUPS == _capi.EXTENT_MAX_GROUPS
    assert _constant("kernels_extents.hip", "EX_WAVES") == ref.WAVES == rt.WAVES
    assert _constant("kernels_extents.hip", "EX_PLANES") == ref.PLANES == rt.PLANES
    kernel = open(os.path.join(CSRC, "kernels_extents.hip")).read()
    shape = re.search(r"RangeShape\s+EX_RANGE\s*=\s*\{EX_WAVES,\s*EX_PLANES,\s*EX_MAX_GROUPS,\s*(\d+)\}", kernel)
    assert shape and int(shape.group(1)) == ref.VOXEL_CAP_LOG2
    assert len(re.findall(r"RangeShape\s+EX_RANGE", kernel)) == 1
    # the table fits four workgroups a CU: key u32 + six u64 a slot
    assert 4 * 52 * ref.LABEL_SLOTS <= 160 * 1024


def test_restated_plan_at_the_shapes_of_the_gpu_tests():
    # one tile; 3 x 3 partial tiles; the multi-tile ranges of range_tiles with clipped last groups
    assert ref.plan((16, 4, 64), 2)[3:6] == (1, 1, 1)
    assert ref.plan((33, 9, 70), 4)[3:6] == (9, 1, 9)
    for name in ("a_u16", "b_u32_scalar", "c_u16", "c_u32_vector"):
        case = rt.CASE[name]
        p = ref.plan(case.dims, case.dtype.itemsize)
        assert p.per >= 2 and p.groups <= ref.MAX_GROUPS and 0 < p.tiles_in_last_group <= p.per, (name, p)
        assert p == rt.plan(case.dims, 0, case.dtype.itemsize, "sigmoments"), name     # (same tile, same 1024 groups; no cap binds here)
    assert any(ref.plan(rt.CASE[n].dims, rt.CASE[n].dtype.itemsize).tiles_in_last_group
               < ref.plan(rt.CASE[n].dims, rt.CASE[n].dtype.itemsize).per for n in ("a_u16", "b_u32_scalar", "c_u16", "c_u32_vector"))


def test_the_kernel_file_is_built_without_contraction():
    assert build.EXTRA_FLAGS["kernels_extents.hip"] == ["-ffp-contract=off"]
    assert "kernels_extents.hip" in build.SOURCES and "ta_api_extents.hip" in build.SOURCES
    assert "ta_extents.h" in build.dependencies("kernels_extents.hip")          # (a change of the header rebuilds the feature)
    host = build.dependencies("ta_api_extents.hip")
    assert "ta_extents.h" in host and any(h.endswith("tissue_scan_extents.h") for h in host)


def test_a_fused_evaluation_differs_from_the_restatement():
    """The case `one tile` of the GPU tests: a kernel whose products were contracted into fused multiply-adds cannot pass it."""
    V = rt.block_labels((16, 4, 64), np.uint16, 11)
    w = ref.weights(int(V.max()) + 1, 12)
    lo, hi = ref.rows(V, w)
    flo, fhi = ref.rows_fused(V, w)
    present = np.isfinite(lo[:, 0])
    assert present.sum() > 10
    differ = int((lo[present] != flo[present]).sum() + (hi[present] != fhi[present]).sum())
    assert differ > 0, "fused and unfused projections agree on every extreme: the case proves nothing"
    np.testing.assert_allclose(flo[present], lo[present], rtol=1e-13, atol=1e-13)     # (one rounding apart, not another quantity)
    np.testing.assert_allclose(fhi[present], hi[present], rtol=1e-13, atol=1e-13)


def test_restatement_against_brute_force_and_signed_zero():
    V = rt.block_labels((5, 6, 7), np.uint16, 3, nlabels=6, block=(2, 3, 2))
    w = ref.weights(int(V.max()) + 1, 4)
    w[1] = [[0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [0.0, 0.0, 0.0]]
    lo, hi = ref.rows(V, w)
    for l in range(w.shape[0]):
        x = np.argwhere(V == l).astype(np.float64)
        if not x.size:
            assert np.isposinf(lo[l]).all() and np.isneginf(hi[l]).all()
            continue
        for k in range(3):
            p = (x[:, 0] * w[l, k, 0] + x[:, 1] * w[l, k, 1]) + x[:, 2] * w[l, k, 2]
            assert lo[l, k] == p.min() and hi[l, k] == p.max()
    assert not np.signbit(lo[1]).any() and not np.signbit(hi[1]).any() and not lo[1].any() and not hi[1].any()


# ---- CellExtents from injected rows ---------------------------------------------------------------------------------------------
def _inject(V, axes, vs, perm=(0, 1, 2)):
    """CellExtents of the label image V (array axes) whose memory order is V.transpose(perm), rows from the restatement."""
    nrows = int(V.max()) + 1
    frames = unit_frames(axes, nrows)
    lo, hi = ref.rows(np.ascontiguousarray(V.transpose(perm)), extent_weights(frames, vs, perm))
    return CellExtents(None, lo, hi, frames, vs, count=np.bincount(V.reshape(-1), minlength=nrows))


def _cuboid_image():
    V = np.zeros((12, 11, 10), dtype=np.uint16)
    V[2:9, 3:8, 4:7] = 2                     # 7 x 5 x 3
    V[10, 9, 1] = 4                          # one voxel; labels 1 and 3 are absent
    return V


@pytest.mark.parametrize("vs", [(0.5, 0.25, 2.0), (0.37, 0.53, 1.1)], ids=["dyadic", "plain"])
def test_cuboid_single_voxel_and_absent_rows(vs):
    e = _inject(_cuboid_image(), np.eye(3), vs)
    L, fill, fp = e.lengths(), e.fill(), e.footprint()
    want = np.array([7, 5, 3]) * np.array(vs)
    if vs == (0.5, 0.25, 2.0):               # binary fractions: every step is exact
        assert np.array_equal(L[2], want) and fill[2] == 1.0
    np.testing.assert_allclose(L[2], want, rtol=1e-12, atol=0)
    assert abs(fill[2] - 1.0) <= 4e-12 and fill[2] <= 1.0
    assert np.array_equal(fp[4], np.array(vs)) and np.array_equal(L[4], fp[4])          # hi == lo
    assert fill[4] == 1.0
    for absent in (1, 3):
        assert np.isnan(L[absent]).all() and np.isnan(fill[absent]) and np.isnan(e.lo[absent]).all() and np.isnan(e.hi[absent]).all()
        assert np.isnan(e.center()[absent]).all() and np.isnan(e.corners()[absent]).all()
    np.testing.assert_allclose(e.center(real=False)[2], [5.0, 5.0, 5.0], rtol=1e-12)
    np.testing.assert_allclose(e.box_volume()[2], np.prod(want), rtol=1e-12)
    np.testing.assert_allclose(e.aspect_ratio()[2], want.max() / want.min(), rtol=1e-12)
    c = e.corners(real=False)[2]
    assert c.shape == (8, 3)
    np.testing.assert_allclose(c.min(axis=0), [1.5, 2.5, 3.5], rtol=1e-12)
    np.testing.assert_allclose(c.max(axis=0), [8.5, 7.5, 6.5], rtol=1e-12)
    got = e.of_labels([2, 99, 4], "lengths")
    assert np.array_equal(got[0], L[2]) and np.isnan(got[1]).all() and np.array_equal(got[2], L[4])
    with pytest.raises(ValueError):
        e.of_labels([2], "length")


def test_fortran_ordered_permutation_gives_the_same_extents():
    V = _cuboid_image()
    frame = complete_frame([1.0, 2.0, -0.5])
    vs = (0.37, 0.53, 1.1)
    c = _inject(V, frame, vs)
    f = _inject(V, frame, vs, perm=(2, 1, 0))                    # what a Fortran-ordered image is on the device
    assert np.array_equal(extent_weights(unit_frames(frame, 1), vs, (2, 1, 0))[0], (unit_frames(frame, 1)[0] * vs)[:, ::-1])
    np.testing.assert_allclose(f.lengths()[[2, 4]], c.lengths()[[2, 4]], rtol=1e-12)
    np.testing.assert_allclose(f.center()[[2, 4]], c.center()[[2, 4]], rtol=1e-12)
    assert (c.fill()[[2]] < 1.0).all()                            # a cuboid in a frame that is not its own


def test_non_finite_axes_and_weights_raise_value_error():
    lo = hi = np.zeros((2, 3))
    bad = np.eye(3)
    bad[1, 2] = np.nan
    with pytest.raises(ValueError):
        CellExtents(None, lo, hi, bad, count=[1, 1])
    with pytest.raises(ValueError):
        CellExtents(None, lo, hi, np.full((3, 3), np.inf), count=[1, 1])
    with pytest.raises(ValueError):
        extent_weights(np.broadcast_to(bad, (2, 3, 3)))
    with pytest.raises(ValueError):
        extent_weights(np.broadcast_to(np.eye(3), (2, 3, 3)), voxelsize=(1.0, np.inf, 1.0))
    with pytest.raises(ValueError):
        unit_frames(np.zeros((3, 3)), 2)                          # a zero direction
    with pytest.raises(ValueError):
        CellExtents(None, lo, hi, np.eye(3))                      # no counts


@pytest.mark.parametrize("vs", [(1.0, 1.0, 1.0), (0.37, 0.53, 1.1)], ids=["unit", "anisotropic"])
def test_digitised_ball(vs):
    """A ball of radius r digitised centre-inside, along given directions: the extreme voxel centre lies in [r - |vs|, r] on each
    side and the footprint is at most |vs| (Cauchy-Schwarz), so |length - 2 r| <= 2 |vs|."""
    r, vs = 9.0, np.asarray(vs)
    n = [int(np.ceil(2 * r / s)) + 5 for s in vs]
    centre = [(m - 1) / 2.0 * s + 0.21 * s for m, s in zip(n, vs)]
    g = np.meshgrid(*[np.arange(m) * s - c for m, s, c in zip(n, vs, centre)], indexing="ij")
    V = ((g[0] ** 2 + g[1] ** 2 + g[2] ** 2) <= r * r).astype(np.uint16)
    rng = np.random.default_rng(2)
    for d in list(np.eye(3)) + list(rng.normal(size=(5, 3))):
        e = _inject(V, complete_frame(d), tuple(vs))
        assert (np.abs(e.lengths()[1] - 2 * r) <= 2 * np.linalg.norm(vs)).all(), (d, e.lengths()[1])
    assert 0.4 < _inject(V, np.eye(3), tuple(vs)).fill()[1] < 0.65             # pi / 6 for the ball itself
