"""The inputs of tests/test_gpu_radix_widths.py, checked without a GPU: every id table is injective, below 2^b and has bit b - 1
set, the records of the volume (helpers.brute_wall_records alone) carry that bit, and every size-class case lands in its class.
That the classes are met is a property of the inputs, established here, not of the kernels."""
import numpy as np
import pytest

import radix_cases as rc
from helpers import brute_wall_records


def check_table(table, b):
    t = table.astype(np.int64)
    assert np.unique(t).size == t.size                               # injective
    assert t.max() < (1 << b) and (np.bitwise_or.reduce(t) >> (b - 1)) & 1 == 1


def records(vol, b):
    lo, hi, co = brute_wall_records(vol)
    assert lo.size > 0
    assert (int(np.bitwise_or.reduce(lo | hi)) >> (b - 1)) == 1    # the widest id of the records has exactly b bits
    return int(lo.size)


@pytest.mark.parametrize("b", rc.WIDTHS)
def test_small_cases_have_their_width(b):
    for kind in ("voronoi", "noise"):
        vol, table = rc.small_case(b, kind)
        check_table(table, b)
        top, half = (1 << b) - 1, 1 << (b - 1)
        assert top in table and half in table and 0 in table
        assert vol.dtype == (np.uint16 if b <= 16 else np.uint32) and vol.shape == rc.SMALL_SHAPE
        assert set(np.unique(vol).tolist()) == set(table.tolist())
        n = records(vol, b)
        assert 2000 <= n <= 60000
    if b <= 16:
        wide, _ = rc.small_case(b, "voronoi", np.uint32)
        assert wide.dtype == np.uint32 and np.array_equal(wide, rc.small_case(b, "voronoi")[0])


@pytest.mark.parametrize("b,d", rc.EDGE_WIDTHS)
@pytest.mark.parametrize("kind", rc.EDGE_KINDS)
def test_digit_edge_cases(b, d, kind):
    vol, table = rc.edge_case(b, d, kind)
    check_table(table, b)
    assert table.size >= 2
    t = table.astype(np.int64)
    low = t & ((1 << d) - 1)
    if kind == "top_bit":
        assert t.size == 2 and (t[0] ^ t[1]) == 1 << (b - 1)
    elif b == d:
        assert sorted(t.tolist()) == [0, (1 << b) - 1]
    elif kind == "digit_zero":
        assert not low.any()
    else:
        assert (low == (1 << d) - 1).all()
    n = records(vol, b)
    assert n % 64 != 0 and n > 4096                                  # a last chunk with lanes that hold no key; several tiles


@pytest.mark.parametrize("b", rc.SIZE_WIDTHS)
@pytest.mark.parametrize("size", sorted(rc.SIZE_CLASSES))
def test_size_classes_are_met_by_the_inputs(b, size):
    vol, table = rc.size_case(b, size)
    check_table(table, b)
    assert set(np.unique(vol).tolist()) == set(table.tolist())
    lo, hi = rc.SIZE_CLASSES[size]
    n = records(vol, b)
    assert lo <= n <= hi, (size, n)
    if size == "segments":
        assert n > 2 * 262144 and -(-n // 4096) > 2 * 64             # three segments of 64 tiles or more
