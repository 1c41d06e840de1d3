"""The nearest-label pass on the MI355X past its launch caps (csrc/kernels_nearest.hip): more rows than the row pass has waves and more
voxels than the counting and the apply kernel have threads, in one volume of (1026, 257, 17) voxels whose number is no multiple of 64,
so the last wave of the counting kernel's second trip is partly past the volume.  The sites come from nearest_cases.cap_sites (checked
without a GPU by test_launch_limits_cpu.py), the plan from tests/launch_limits.py; the test asserts from the reference that sites,
ties, filled and unfilled voxels lie in the second trips, then compares what the device launched (ta_nearest_debug) with the plan and
N, D2, the counts and the filled volume bit for bit with nearest_reference.brute_sites.  One small volume takes the plan of the
column batches, which this pass shares with the distance pass (csrc/ta_separable.h), through an explicit batch that is no whole wave."""
import functools

import numpy as np
import pytest

import distance_reference as dref
import launch_limits as ll
import nearest_cases as cases
import nearest_reference as ref
from test_gpu_nearest import device, same
from tissue_analysis_amd import _capi
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def answer(dims):
    """(V uint16, N, D2, ways, max_d2): the limit is the median D2 of the last six planes, where the row pass's second trip is."""
    V = cases.cap_sites(dims)
    n, d2, ways = ref.brute_sites(V, 0, cases.CAP_SPACING)
    out = (V, n, d2, ways)
    for a in out:
        a.setflags(write=False)
    return out + (float(np.median(d2[-6:])),)


def run(V, spacing, n, d2, limit, memory_dims):
    """One pass and the fill; the plan the device followed."""
    rv = ResidentVolume(V)
    try:
        got = device(rv, 0, spacing, None, limit)
        debug = rv.ctx.nearest_debug()
        image = same(got, V, n, d2, 0, limit)
        x = rv.apply_nearest(_capi.F_VOLUME)
        assert np.array_equal(rv.host, image)
        assert np.array_equal(np.asarray(x.count[:17]).astype(np.int64), np.bincount(image.reshape(-1), minlength=17))
    finally:
        rv.close()
    p = ll.nearest_plan(memory_dims)
    assert debug == dict(row_groups=p.row_groups, count_groups=p.voxel_groups, apply_groups=p.voxel_groups,
                         column_launches=ll.nearest_column_launches(memory_dims))
    return p


def second_trips_hold_sites_ties_and_limit(dims):
    """From the reference alone: what the second trips have to get right is there."""
    V, n, d2, ways, limit = answer(dims)
    row, voxel = ll.nearest_second_trip(dims)
    assert row == 262144 and voxel == 4194304 and V.size % 64 == 34
    sites = np.flatnonzero(V.reshape(-1))
    assert sites.size == 16 and (sites >= row * dims[2]).sum() >= 3 and ((sites >= voxel) & (sites < row * dims[2])).sum() >= 3
    assert (sites < voxel).sum() >= 3
    filled = ref.filled(V, d2, 0, limit).reshape(-1)
    left = (V.reshape(-1) == 0) & ~filled
    assert 0.0 < limit < np.inf
    for cut in (voxel, row * dims[2]):                     # filled and unfilled voxels in both trips of both kinds of kernel
        assert filled[:cut].any() and filled[cut:].any() and left[:cut].any() and left[cut:].any()
    assert left[-34:].any() or filled[-34:].any()          # the partial last wave has work
    tied = (ways >= 2).reshape(-1)
    assert tied[row * dims[2]:].sum() > 1000 and tied[voxel:row * dims[2]].sum() > 1000
    for a, b in cases.CAP_PAIRS:                           # the voxel between the two sites of every pair is equally near to both
        mid = tuple((x + y) // 2 for x, y in zip(a, b))
        assert ways[mid] == 2 and n[mid] == min(V[a], V[b]) and np.ravel_multi_index(mid, dims) >= voxel
    assert sum(np.ravel_multi_index(tuple((x + y) // 2 for x, y in zip(a, b)), dims) >= row * dims[2] for a, b in cases.CAP_PAIRS) == 2


def test_past_both_caps():
    dims = cases.CAP_DIMS
    V, n, d2, ways, limit = answer(dims)
    second_trips_hold_sites_ties_and_limit(dims)
    p = run(V, cases.CAP_SPACING, n, d2, limit, dims)
    assert p.row_groups == ll.NEAR_ROW_MAX_GROUPS < (p.rows + 3) // 4 and p.row_trips == 2                 # fewer waves than rows
    assert p.voxel_groups == ll.NEAR_VOXEL_MAX_GROUPS < (p.voxels + 255) // 256 and p.voxel_trips == 2     # fewer threads than voxels


def test_past_both_caps_in_a_permuted_layout_of_32_bit_labels():
    """The same memory, seen as a (257, 1026, 17) array whose axis 1 is the slowest."""
    dims = cases.CAP_DIMS
    V, n, d2, ways, limit = answer(dims)
    second_trips_hold_sites_ties_and_limit(dims)
    W = V.astype(np.uint32).transpose(1, 0, 2)
    s = cases.CAP_SPACING
    assert W.shape == (257, 1026, 17) and not W.flags.c_contiguous
    p = run(W, (s[1], s[0], s[2]), n.transpose(1, 0, 2), d2.transpose(1, 0, 2), limit, dims)
    assert (p.row_groups, p.row_trips, p.voxel_groups, p.voxel_trips) == (ll.NEAR_ROW_MAX_GROUPS, 2, ll.NEAR_VOXEL_MAX_GROUPS, 2)


def test_an_explicit_batch_rounds_up_to_whole_waves_in_both_passes():
    """ta_distance_set_batch and ta_nearest_set_batch go through one plan: 100 columns a launch are rounded up to two waves, which
    the 3 * 70 = 210 columns along memory axis 1 take in 2 launches and the 5 * 70 = 350 along axis 0 in 3.  What both passes
    answer does not depend on the batch, and is the references'."""
    V = np.random.default_rng(11).integers(0, 5, (3, 5, 70)).astype(np.uint16)
    assert (V == 0).any() and int(V.max()) == 4
    spacing = (0.5, 1.0, 2.0)
    want_d2 = dref.scipy_d2(V, spacing)
    n, d2 = ref.brute(V, 0, spacing)
    answers = []
    rv = ResidentVolume(V)
    try:
        for batch, launches in ((100, 2 + 3), (0, 1 + 1)):
            rv.ctx.distance_set_batch(batch)
            rv.ctx.nearest_set_batch(batch)
            near = device(rv, 0, spacing)
            rv.ctx.distance_extract(_capi.DIST_OWN_WALL, 0, spacing, 0)
            dist = (np.array(rv.distance_image()),) + rv.ctx.distance_get()
            assert rv.ctx.distance_debug()["column_launches"] == rv.ctx.nearest_debug()["column_launches"] == launches
            answers.append((near, dist))
    finally:
        rv.close()
    (near, dist), (near_auto, dist_auto) = answers
    assert near[3:] == near_auto[3:]
    for a, b in zip(near[:3] + dist, near_auto[:3] + dist_auto):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    same(near, V, n, d2)
    assert dist[0].dtype == np.float64 and np.array_equal(dist[0], want_d2)
    for g, w in zip(dist[1:], dref.table(V, want_d2, 5)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def test_just_below_both_caps():
    """The same sites in a volume that is a little smaller: the plan changes, the grids are below their caps."""
    dims = cases.CAP_CONTROL_DIMS
    V, n, d2, ways, limit = answer(dims)
    assert (ways >= 2).any() and ref.filled(V, d2, 0, limit).any() and ((V == 0) & (d2 > limit)).any()
    p = run(V, cases.CAP_SPACING, n, d2, limit, dims)
    assert p.row_groups == (p.rows + 3) // 4 < ll.NEAR_ROW_MAX_GROUPS and p.voxel_groups == (p.voxels + 255) // 256 < ll.NEAR_VOXEL_MAX_GROUPS
    assert (p.row_trips, p.voxel_trips) == (1, 1)
