"""The tie rule of the nearest-label maps on the MI355X (csrc/kernels_nearest.hip) where many sites are equally near, and the chunk
carry of its row pass.  test_gpu_nearest.py meets ties in noise only, where an envelope is two or three entries deep; a column
kernel that loses a boundary label when the entry that holds it is popped at the same boundary in its turn passes it
(test_nearest_cpu.py shows that, and that the volumes here catch it).  The volumes come from tests/nearest_cases.py: sites on all
lattice points of a sphere or an ellipsoid, every site with its own label and the smallest label on every site in turn, and rows
built around the 64-voxel chunks.

Every test first asserts, from the reference, that its volume has the ties it is named for (`ways`, the labels at exactly the minimal
distance), then compares N and D2 (ta_nearest_image), the counts (ta_nearest_get) and the volume after ta_nearest_apply bit for bit
with nearest_reference.brute_sites: every spacing is a power of two."""
import functools

import numpy as np
import pytest

import nearest_cases as cases
import nearest_reference as ref
from test_gpu_nearest import device, same
from tissue_analysis_amd import _capi
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu

DTYPES = [np.uint16, np.uint32]


def frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def shell_answers(name, shape=None, centre=None, kinds=("random", "down", "up")):
    """[(labels, N, D2, ways)] of every label assignment of a shell: computed once, shared by the dtypes and the layouts."""
    spacing, sh = cases.SHELLS[name][0], cases.shell(name)
    return [frozen((labels,) + ref.brute_sites(cases.shell_volume(sh, labels, np.uint16, shape, centre), 0, spacing))
            for kind, labels in cases.assignments(len(sh.sites)) if kind.rstrip("0123456789") in kinds]


def both_batches_and_apply(rv, V, spacing, n, d2, not_from=None, max_d2=np.inf):
    """The pass with a wave of columns a launch and with the automatic batch, then the fill; the device's answer of the last pass."""
    rv.ctx.nearest_set_batch(64)
    same(device(rv, 0, spacing, not_from, max_d2), V, n, d2, 0, max_d2)
    assert rv.ctx.nearest_debug()["column_launches"] > 2
    rv.ctx.nearest_set_batch(0)
    got = device(rv, 0, spacing, not_from, max_d2)
    image = same(got, V, n, d2, 0, max_d2)
    assert rv.ctx.nearest_debug()["column_launches"] == 2
    rv.apply_nearest(_capi.F_VOLUME)
    assert rv.host.dtype == V.dtype and np.array_equal(rv.host, image)
    return got, image


def every_assignment(answers, volume, layouts, spacing):
    """One resident volume per layout, a new upload per label assignment."""
    for perm in layouts:
        rv = None
        try:
            for labels, n, d2, ways in answers:
                V = volume(labels)
                if rv is None:
                    rv = ResidentVolume(cases.in_layout(V, perm))
                else:
                    rv.upload(cases.in_layout(V, perm))
                both_batches_and_apply(rv, V, spacing, n, d2)
        finally:
            if rv is not None:
                rv.close()


# ---- a shell in the middle of its volume ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(cases.SHELLS))
def test_shells_with_the_smallest_label_on_every_site(name, dtype):
    spacing, _, _, _, count = cases.SHELLS[name]
    sh = cases.shell(name)
    answers = shell_answers(name)
    assert len(answers) == 4 + 2 * count
    for labels, n, d2, ways in answers:
        assert ways[sh.centre] == count and n[sh.centre] == 1 and d2[sh.centre] == cases.shell_d2(name)      # every site equally near
        assert (ways >= 3).sum() >= (100 if name[0] == "r" else 19)
    every_assignment(answers, lambda labels: cases.shell_volume(sh, labels, dtype), cases.shell_layouts(name), spacing)


# ---- the shell around the end of a chunk of the row pass --------------------------------------------------------------------------
@pytest.mark.parametrize("column", cases.OFF_CENTRE_COLUMNS)
def test_off_centre_shells(column):
    """The r9 shell in rows of 140 voxels with its centre at column 64 and at column 127: the seven parabolas that meet at the centre
    lie along the row pass in the layouts that keep axis 2 fastest and along a column pass in the others, and the ties of the row
    pass lie on both sides of a chunk's end."""
    sh = cases.shell("r9")
    shape, centre = cases.OFF_CENTRE_SHAPE, (5, 5, column)
    answers = shell_answers("r9", shape, centre, ("random", "down"))
    assert len(answers) == 4 + 30 and column % cases.ROW_CHUNK in (0, cases.ROW_CHUNK - 1)
    for labels, n, d2, ways in answers:
        assert ways[centre] == 30 and n[centre] == 1 and (ways[:, :, column - 1:column + 2] >= 2).any(axis=(0, 1)).all()
    every_assignment(answers, lambda labels: cases.shell_volume(sh, labels, np.uint16, shape, centre), cases.PERMS, cases.UNIT)


# ---- sites that do not count, and the limit at exactly the shell --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["r9", "half36", "mixed144"])
def test_not_from_the_smallest_label_of_the_shell(name):
    spacing, _, _, _, count = cases.SHELLS[name]
    sh = cases.shell(name)
    for _, labels in list(cases.assignments(count))[:6]:
        V = cases.shell_volume(sh, labels, np.uint16)
        n, d2, ways = ref.brute_sites(V, 0, spacing, 1)
        assert ways[sh.centre] == count - 1 and n[sh.centre] == 2 and not (n == 1).any()
        for perm in cases.shell_layouts(name):
            rv = ResidentVolume(cases.in_layout(V, perm))
            try:
                got, image = both_batches_and_apply(rv, V, spacing, n, d2, 1)
                assert got[2][1] == 0 and got[0][sh.centre] == 2 and int((image == 1).sum()) == 1
            finally:
                rv.close()


@pytest.mark.parametrize("name", ["r9", "r26", "half36", "mixed144"])
def test_max_distance_of_exactly_the_shell(name):
    spacing, _, _, _, count = cases.SHELLS[name]
    sh = cases.shell(name)
    limit = cases.shell_d2(name)
    below = float(np.nextafter(limit, 0.0))
    labels = next(cases.assignments(count))[1]
    V = cases.shell_volume(sh, labels, np.uint16)
    n, d2, ways = ref.brute_sites(V, 0, spacing)
    at_limit = int(((V == 0) & (d2 == limit)).sum())
    assert ways[sh.centre] == count and d2[sh.centre] == limit and at_limit >= 1 and (d2 > limit).any()
    for perm in cases.shell_layouts(name):
        rv = ResidentVolume(cases.in_layout(V, perm))
        try:
            under = device(rv, 0, spacing, None, below)
            left = same(under, V, n, d2, 0, below)
            rv.apply_nearest(_capi.F_VOLUME)
            assert left[sh.centre] == 0 and np.array_equal(rv.host, left)                  # just below the shell the centre stays empty
            rv.upload(cases.in_layout(V, perm))
            got, image = both_batches_and_apply(rv, V, spacing, n, d2, None, limit)
            assert image[sh.centre] == 1 and got[3] - under[3] == at_limit == under[4] - got[4] and (image == 0).any()
        finally:
            rv.close()


# ---- the carry of the row pass ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_around_the_chunks_of_the_row_pass(dtype):
    """In C order the row pass sees the rows; in the layouts that put their axis on memory axis 1 or 0 a column pass sees them as
    envelopes of parabolas of height zero that are 1 .. 186 voxels apart."""
    V = cases.row_carry_rows().astype(dtype)
    n, d2, ways = ref.brute_sites(V, 0, cases.ROW_SPACING)
    assert ways[0, :4, 64].tolist() == [2, 2, 2, 2] and n[0, :4, 64].tolist() == [2, 2, 3, 3]          # ties on the first lane of a chunk
    assert ways[0, 4:6, 96].tolist() == [2, 2] and not V[0, 4:6, 64:128].any()                          # a carry over a chunk without a site
    assert ways[0, 8, 96] == 2 and np.isfinite(d2).all() and (d2[0, 9] > 0).all() and not d2[0, 10].any()
    for perm in cases.PERMS:
        rv = ResidentVolume(cases.in_layout(V, perm))
        try:
            both_batches_and_apply(rv, V, cases.ROW_SPACING, n, d2)
        finally:
            rv.close()
