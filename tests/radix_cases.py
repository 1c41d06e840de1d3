"""Label volumes that put the wall grouping's radix sort (csrc/kernels_wallsort.hip) on a chosen key width: a base labelling
(voronoi tissue, or noise over a few labels so that every pair owns thousands of records, interleaved in memory) mapped through
an injective table of ids below 2^b.  The table always holds 2^b - 1 and 2^(b-1), so the OR of the ids is b bits wide, and 0.
NumPy only: tests/test_radix_cases_cpu.py checks every case against helpers.brute_wall_records without a GPU, and
tests/test_gpu_radix_widths.py runs the same cases on the device."""
import functools

import numpy as np

from helpers import voronoi

WIDTHS = tuple(range(1, 33))
SMALL_SHAPE = (6, 12, 140)
SEGMENT = 64 * 4096                       # records of one segment of the sort's offset scan: 64 tiles of 4096 keys
# (width b, digit width d) of the digit edge cases, and one width per (key type, digit width) class for the size classes
EDGE_WIDTHS = ((10, 10), (20, 10), (30, 10), (16, 8))
EDGE_KINDS = ("digit_zero", "digit_ones", "top_bit")
SIZE_WIDTHS = (16, 13, 15, 18, 32)
# record counts a size class must land in (asserted on the reference's output, by the CPU test and again by the GPU test)
SIZE_CLASSES = {"wave": (1, 1023), "two_tiles": (4097, 8191), "segments": (2 * SEGMENT + 1, 1 << 31)}
SIZE_SHAPES = {"wave": (2, 3, 12), "two_tiles": (3, 6, 50), "segments": (8, 24, 350)}
SIZE_IDS = 12                             # distinct ids of a size-class volume (noise)


def dtype_of(b):
    return np.uint16 if b <= 16 else np.uint32


def id_table(b, n, seed):
    """min(n, 2^b) distinct ids below 2^b in random order: 2^b - 1, 2^(b-1), 0, the rest random."""
    rng = np.random.default_rng(seed)
    n = min(int(n), 1 << b)
    ids = []
    for v in ((1 << b) - 1, 1 << (b - 1), 0):
        if v not in ids and len(ids) < n:
            ids.append(v)
    have = set(ids)
    while len(ids) < n:
        v = int(rng.integers(0, 1 << b))
        if v not in have:
            have.add(v)
            ids.append(v)
    return np.array(ids, dtype=np.uint32)[rng.permutation(n)]


def edge_table(b, d, kind, n, seed):
    """Ids of width b for one digit edge case (d = the digit width of that key width):
       digit_zero  every id a multiple of 2^d: the passes over the low digit of lo and of hi see digit 0 in every key;
       digit_ones  every id with its low d bits set: digit 2^d - 1 in every key of those passes;
       top_bit     two ids that differ in bit b - 1 only: one pair, every pass sees ONE digit in every key.
    With b = d an id is a single digit, so only 0 is a multiple of 2^d and only 2^b - 1 has the low d bits set: the two
    together ({0, 2^b - 1}: one pass all zeros, the other all ones) stand for both cases there."""
    rng = np.random.default_rng(seed)
    if kind == "top_bit":
        x = int(rng.integers(0, 1 << (b - 1)))
        return np.array([x, x | (1 << (b - 1))], dtype=np.uint32)
    if b == d:
        return np.array([0, (1 << b) - 1], dtype=np.uint32)
    high = id_table(b - d, n, seed).astype(np.uint64) << np.uint64(d)              # holds 2^(b-d) - 1: bit b - 1 is set
    low = np.uint64((1 << d) - 1 if kind == "digit_ones" else 0)
    return (high | low).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _voronoi_ranks(shape, n_cells, seed):
    v = voronoi(shape, n_cells, seed, np.uint16)
    ranks = np.unique(v, return_inverse=True)[1].reshape(v.shape)
    ranks.setflags(write=False)
    return ranks


def base_labels(kind, shape, n, seed):
    """A labelling in 0 .. k - 1, k <= n, every value present: voronoi tissue (cells folded modulo n) or uniform noise."""
    if kind == "voronoi":
        base = _voronoi_ranks(tuple(shape), 40, seed) % n
    else:
        base = np.random.default_rng(seed).integers(0, n, size=shape)
    u, inv = np.unique(base, return_inverse=True)
    return inv.reshape(base.shape), int(u.size)


def through(base, table, dtype):
    return np.ascontiguousarray(table[base].astype(dtype))


def small_case(b, kind, dtype=None):
    """(volume, id table) of width b on SMALL_SHAPE; kind "voronoi" (40 cells) or "noise" (6 labels)."""
    want = 40 if kind == "voronoi" else 6
    base, k = base_labels(kind, SMALL_SHAPE, min(want, 1 << b), 100 + b)
    table = id_table(b, k, 200 + b)
    return through(base, table, dtype or dtype_of(b)), table


def edge_case(b, d, kind):
    n = 2 if kind == "top_bit" or b == d else 6
    base, k = base_labels("noise", SMALL_SHAPE, n, 300 + b)
    table = edge_table(b, d, kind, k, 400 + b)
    return through(base, table[:k], dtype_of(b)), table[:k]


def size_case(b, size):
    """(volume, id table): noise over SIZE_IDS ids of width b, shaped for the record count of size class `size`."""
    base, k = base_labels("noise", SIZE_SHAPES[size], SIZE_IDS, 500 + b)
    table = id_table(b, k, 600 + b)
    return through(base, table, dtype_of(b)), table
