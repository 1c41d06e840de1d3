"""The stable radix sort of csrc/kernels_wallsort.hip at every key and digit width the wall grouping can give it, order-exact:
ctx.wall_voxels(by_pair=True) against helpers.brute_wall_records (the 18 offsets and np.unique over (lo, hi, voxel); no code
shared with the kernels), array for array.  A pair's coordinates coming out in memory order IS the stability check.

The sort key of the grouping is lo << b | hi, b = the bit length of the OR of the ids in the volume, so a volume whose ids are
drawn below 2^b (tests/radix_cases.py: 2^b - 1 and 2^(b-1) always among them) fixes the key type, the number of passes and the
digit width.  Read off rs_passes / rs_digit_bits and launch_wall_group_* as they stand (keys of 2b <= 32 bits are sorted as
uint32, wider ones as uint64; as few passes of at most 10 bits as it takes, all of one width, never below 8):

     b  key  passes x bits |   b  key  passes x bits |   b  key  passes x bits |   b  key  passes x bits
     1  u32    1 x 8       |   9  u32    2 x 9       |  17  u64    4 x 9       |  25  u64    5 x 10
     2  u32    1 x 8       |  10  u32    2 x 10      |  18  u64    4 x 9       |  26  u64    6 x 9
     3  u32    1 x 8       |  11  u32    3 x 8       |  19  u64    4 x 10      |  27  u64    6 x 9
     4  u32    1 x 8       |  12  u32    3 x 8       |  20  u64    4 x 10      |  28  u64    6 x 10
     5  u32    1 x 10      |  13  u32    3 x 9       |  21  u64    5 x 9       |  29  u64    6 x 10
     6  u32    2 x 8       |  14  u32    3 x 10      |  22  u64    5 x 9       |  30  u64    6 x 10
     7  u32    2 x 8       |  15  u32    3 x 10      |  23  u64    5 x 10      |  31  u64    7 x 9
     8  u32    2 x 8       |  16  u32    4 x 8       |  24  u64    5 x 10      |  32  u64    7 x 10

The wall grouping never sorts uint64 keys in 8-bit digits (the overlap and junction tables do, at their fixed widths), so the
(key type, digit width) classes are five: (u32, 8), (u32, 9), (u32, 10), (u64, 9), (u64, 10).

What runs here (nothing below computes the table above; the widths are asserted on the ids, the sizes on the reference):
  small cases   every b in 1 .. 32, both fetch modes (TA_WALL_KEYED 1 / 0), voronoi tissue and noise over six labels on
                (6, 12, 140): 2 000 .. 60 000 records, up to 15 tiles of 4096 keys in ONE segment of the offset scan;
                b <= 16 once more as a uint32 volume.
  digit edges   b = 10, 20, 30 (10-bit digits) and 16 (8-bit digits): ids that are all multiples of 2^d (a pass in which
                every key has digit 0: one run of 64 in every chunk), ids whose low d bits are all set (digit 2^d - 1 in every
                key), two ids that differ in their top bit only.  With b = d = 10 an id IS one digit, so the first two are
                the ids {0, 1023}: one pass of all zeros, one of all ones.  Every record count is not a multiple of 64 (the
                last chunk has lanes without a key).
  size classes  b = 16 (u32, 4 x 8), 13 (u32, 3 x 9), 15 (u32, 3 x 10), 18 (u64, 4 x 9), 32 (u64, 7 x 10), each at
                  wave        fewer than 1024 records: one wave of one tile,
                  two_tiles   between 4096 and 8192 records,
                  segments    more than 2 x 262 144 records: three segments or more, so the offset scan adds the totals of the
                              segments before it AND (9 / 10-bit digits) the digits below its workgroup's 256,
                both fetch modes.  With the small cases (one segment) every class has run with one segment and with three.
"""
import os

import numpy as np
import pytest

import radix_cases as rc
from helpers import brute_wall_records
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu


@pytest.fixture
def keyed():
    def set_to(mode):
        if mode is None:
            os.environ.pop("TA_WALL_KEYED", None)
        else:
            os.environ["TA_WALL_KEYED"] = mode
    yield set_to
    os.environ.pop("TA_WALL_KEYED", None)


def grouped(vol):
    rv = ResidentVolume(vol)
    try:
        return rv.ctx.wall_voxels(by_pair=True)[:3]
    finally:
        rv.close()


def check(vol, b, want=None):
    """The grouped fetch of `vol` equals the brute force, array for array; the ids of the records are b bits wide."""
    want_lo, want_hi, want_co = want if want is not None else brute_wall_records(vol)
    assert want_lo.size > 0
    assert int(np.bitwise_or.reduce(want_lo | want_hi)) >> (b - 1) == 1
    lo, hi, co = grouped(vol)
    assert lo.size > 0 and (int(np.bitwise_or.reduce(lo | hi)) >> (b - 1)) & 1
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
    assert np.array_equal(co, want_co)                               # within a pair: memory order, i.e. the sort is stable
    return int(lo.size)


@pytest.mark.parametrize("mode", ["1", "0"])
@pytest.mark.parametrize("b", rc.WIDTHS)
def test_every_label_width_small(keyed, b, mode):
    keyed(mode)
    for kind in ("voronoi", "noise"):
        vol, _ = rc.small_case(b, kind)
        assert vol.dtype == rc.dtype_of(b)
        assert 2000 <= check(vol, b) <= 60000


@pytest.mark.parametrize("b", [b for b in rc.WIDTHS if b <= 16])
def test_narrow_labels_in_a_uint32_volume(b):
    vol, _ = rc.small_case(b, "voronoi", np.uint32)
    assert vol.dtype == np.uint32
    check(vol, b)


@pytest.mark.parametrize("b,d", rc.EDGE_WIDTHS)
@pytest.mark.parametrize("kind", rc.EDGE_KINDS)
def test_digit_edge_cases(keyed, b, d, kind):
    vol, table = rc.edge_case(b, d, kind)
    low = table.astype(np.int64) & ((1 << d) - 1)
    if kind == "top_bit":
        assert table.size == 2 and int(table[0]) ^ int(table[1]) == 1 << (b - 1)
    elif b == d:
        assert sorted(table.tolist()) == [0, (1 << b) - 1]
    else:
        assert (low == (0 if kind == "digit_zero" else (1 << d) - 1)).all()
    want = brute_wall_records(vol)
    assert want[0].size % 64 != 0
    for mode in ("1", "0"):
        keyed(mode)
        check(vol, b, want)


@pytest.mark.parametrize("size", sorted(rc.SIZE_CLASSES))
@pytest.mark.parametrize("b", rc.SIZE_WIDTHS)
def test_size_classes(keyed, b, size):
    vol, _ = rc.size_case(b, size)
    want = brute_wall_records(vol)
    lo, hi = rc.SIZE_CLASSES[size]
    assert lo <= want[0].size <= hi
    for mode in ("1", "0"):
        keyed(mode)
        n = check(vol, b, want)
        assert lo <= n <= hi
        if size == "segments":
            assert n > 2 * 262144
