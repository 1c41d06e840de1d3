"""The mesh pass (csrc/kernels_mesh.hip) groups its face and corner records by cell with the stable radix sort of
kernels_wallsort.hip on uint32 keys as wide as max_label: here at every pass count and digit width a dense extraction can
reach, against tests/mesh_reference.py through assert_identical -- bit-identical, order included, so a cell's vertices in
corner order and its faces in voxel-then-direction order are what checks the sort's stability.

Dense rows (sparse=False: rows 0 .. max_label), voronoi cells relabelled to random ids below 2^w with 2^w - 1 (= max_label)
and 0 among them, so the low and the high digit both vary.  Bit length w of max_label -> passes x digit bits, read off
rs_passes / rs_digit_bits as they stand:

     w   1      8      9      10      11     16     17     20      21
         1 x 8  1 x 8  1 x 9  1 x 10  2 x 8  2 x 8  2 x 9  2 x 10  3 x 8

3 x 9 and 3 x 10 need max_label of 25 to 28 bits, i.e. row tables of gigabytes: left out here; the same kernels run those classes
on wall keys in tests/test_gpu_radix_widths.py.  Widths 16, 17 and 20 (one per digit width) also run on a volume whose face
and corner records both pass 262 144, one segment of the sort's offset scan; the rest on (24, 28, 40)."""
import functools

import numpy as np
import pytest

import mesh_reference as ref
import radix_cases as rc
from helpers import voronoi
from test_gpu_cell_meshes import assert_identical, check, device_meshes
from tissue_analysis_amd import device as dev

pytestmark = pytest.mark.gpu

WIDTHS = (1, 8, 9, 10, 11, 16, 17, 20, 21)
BIG_WIDTHS = (16, 17, 20)
SEGMENT = 64 * 4096


def relabelled(base, w, seed, dtype):
    """`base` with its cells given random ids below 2^w (cells folded together where there are more cells than ids)."""
    u, inv = np.unique(base, return_inverse=True)
    n = min(int(u.size), 1 << w)
    table = rc.id_table(w, n, seed)
    V = table[inv.reshape(base.shape) % n].astype(dtype)
    ids = np.unique(V)
    assert int(ids[-1]).bit_length() == w and ids[-1] == (1 << w) - 1 and ids[0] < 256 and ids.size == n
    return V


@functools.lru_cache(maxsize=None)
def small_base():
    return voronoi((24, 28, 40), 20, 11, np.uint16)


@functools.lru_cache(maxsize=None)
def big_base():
    ctx = dev.torch_context(0)
    try:
        v, _ = dev.synth_slab(ctx, (96, 80, 128), np.uint16, 150, 4)
        return v.cpu().numpy().view(np.uint16).copy()
    finally:
        ctx.close()


@pytest.mark.parametrize("w", WIDTHS)
def test_sort_widths_small(w):
    V = relabelled(small_base(), w, 700 + w, np.uint32)
    want = ref.mesh(V)
    assert len(want["points"]) > 4096 and len(want["triangles"]) > 2 * 4096          # more than one tile of each stream
    assert_identical(device_meshes(V, sparse=False), want)
    if w <= 16:
        assert_identical(device_meshes(V.astype(np.uint16), sparse=False), want)


@pytest.mark.parametrize("w", BIG_WIDTHS)
def test_sort_widths_with_more_than_one_segment(w):
    V = relabelled(big_base(), w, 800 + w, np.uint32)
    want = ref.mesh(V)
    assert len(want["points"]) > SEGMENT and len(want["triangles"]) // 2 > SEGMENT      # corner and face records
    assert_identical(device_meshes(V, sparse=False), want)
    if w <= 16:
        assert_identical(device_meshes(V.astype(np.uint16), sparse=False), want)


def test_a_subset_with_the_highest_id_at_a_multi_pass_width():
    V = relabelled(small_base(), 17, 717, np.uint32)
    ids = np.unique(V)
    check(V, labels=ids[-1:].tolist() + ids[1::3].tolist(), sparse=False)
    check(V, labels=[int(ids[-1])], sparse=False)
