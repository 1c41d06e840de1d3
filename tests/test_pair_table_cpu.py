"""The CPU model of the adjacency hash table (pair_table_model.py) against known answers, the C oracle and a plain sequential
table -- and the record of why test_gpu_pair_table_limits.py exists: at the automatic table size none of the volumes the suite
had compared with the oracle makes a probe sequence cross the table's end, and none overflows it."""
import itertools
import os

import numpy as np
import pytest

from oracle import onepass, onepass_c

import pair_table_model as ptm
from helpers import assert_same_accumulators, voronoi

HERE = os.path.dirname(os.path.abspath(__file__))


def test_hash_known_answers():
    """hash_u32 and hash_pair of ta_device.h, the words worked out from the header's five steps in 32-bit unsigned arithmetic."""
    assert ptm.hash_u32(0) == 0                                   # every step maps 0 to 0
    # 1: x ^= x >> 16 -> 1; * 0x7feb352d -> 0x7feb352d; ^= >> 15 -> 0x7feb352d ^ 0xffd6 = 0x7febcafb; * 0x846ca68b; ^= >> 16
    assert (0x7feb352d ^ (0x7feb352d >> 15)) == 0x7febcafb
    assert ptm.hash_u32(1) == 0x688990c0
    assert ptm.hash_u32(2) == 0xd1132181
    assert ptm.hash_u32(0xFFFFFFFF) == 0x6768824a
    assert ptm.hash_u32(0x80000000) == 0xcc4b4124
    assert ptm.hash_u32(65535) == 0x33cad8ba
    assert ptm.hash_u32(1 << 32) == 0                             # arguments are taken modulo 2^32, as a uint32_t parameter does
    # lo = 0: lo * 0x9E3779B1 is 0, the pair hashes like hash_u32(hash_u32(hi))
    assert ptm.hash_pair(0, 1) == ptm.hash_u32(0x688990c0) == 0x58f54975
    assert ptm.hash_pair(0, 0xFFFFFFFF) == 0x2d8643b4
    assert ptm.hash_pair(1, 2) == ptm.hash_u32(0x9E3779B1 ^ 0xd1132181) == 0xbe477fa1
    assert ptm.hash_pair(65534, 65535) == 0xa66fd92b
    assert ptm.hash_pair(7, 9000) == 0x865a6d24
    assert ptm.hash_pair(1, 0) == 0x6d523710                      # not symmetric
    assert ptm.home(1, 2, 4) == 0x1 and ptm.home(1, 2, 16) == 0x7fa1 and ptm.home(0, 1, 9) == 0x175


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_chain_volumes_have_exactly_their_pairs(axis, dtype):
    for K in (16, 17, 64, 256, 512, 513):
        for width, other in ((2, (3, 4)), (3, (2, 5))):
            vol = ptm.chain_volume(K, axis, dtype, width=width, other=other)
            assert vol.dtype == dtype and vol.shape[axis] == (K + 1) * width and vol.size == (K + 1) * width * other[0] * other[1]
            want = onepass_c.extract(vol)
            lo, hi = ptm.chain_pairs(K)
            assert np.array_equal(want["pair_lo"], lo) and np.array_equal(want["pair_hi"], hi), (K, axis)
            faces = np.zeros((K, 3), dtype=np.uint64)
            faces[:, axis] = other[0] * other[1]
            assert np.array_equal(want["pair_faces"], faces), (K, axis)


FULL, ONE_MORE, VORONOI_GROWS = ptm.FULL, ptm.ONE_MORE, ptm.VORONOI_GROWS


def test_the_gpu_cases_wrap():
    for K, log2 in FULL:
        lo, hi = ptm.chain_pairs(K)
        assert (1 << log2) == K and ptm.wraps(lo, hi, log2), (K, log2)
    for K, log2 in ONE_MORE:                             # ... in the table they end in, too, where npairs <= 512 says which
        lo, hi = ptm.chain_pairs(K)
        assert ptm.wraps(lo, hi, log2)
    want = onepass_c.extract(voronoi(*VORONOI_GROWS, np.uint32))
    assert want["pair_lo"].size == 254 and ptm.grown_log2(254, 4) == 8
    assert ptm.wraps(want["pair_lo"], want["pair_hi"], 8)


def _auto_log2(max_label):                               # auto_pair_log2 of ta_api.hip: 16 slots a label, 2^16 at least
    log2 = 16
    while (1 << log2) < 16 * (max_label + 1) and log2 < 28:
        log2 += 1
    return log2


def _noise_volume():                                     # test_worst_case_noise_volume_spills_correctly
    return np.random.default_rng(5).permutation(16 * 16 * 256).astype(np.uint32).reshape(16, 16, 256) + 1


def test_the_volumes_the_suite_had_do_not_wrap():
    """The record: adjacency was compared with the oracle in hundreds of cases and none of these reaches the table's end."""
    golden = np.load(os.path.join(HERE, "golden", "config1_128x128x64_u16.npz"))
    cases = [("noise", onepass_c.extract(_noise_volume()), 188160, 21),
             ("two ranks, 20000 cells", onepass_c.extract(voronoi((37, 40, 264), 20000, 61, np.uint32)), 55797, 19),
             ("two ranks, 50 cells", onepass_c.extract(voronoi((37, 40, 264), 50, 61, np.uint32)), 212, 16),
             ("C1 golden (128, 128, 64)", dict(pair_lo=golden["pair_lo"], pair_hi=golden["pair_hi"], max_label=int(golden["max_label"])), 842, 16)]
    for name, want, npairs, log2 in cases:
        assert want["pair_lo"].size == npairs and _auto_log2(int(want["max_label"])) == log2, name
        assert not ptm.wraps(want["pair_lo"], want["pair_hi"], log2), name
        slots, overflow = ptm.probe_insert(zip(want["pair_lo"].tolist(), want["pair_hi"].tolist()), log2)
        assert not overflow, name                        # ... and none comes near the probe limit


def test_wraps_against_the_sequential_table():
    """wraps() is the suffix-count condition; a sequential table shows the same thing directly: some key sits below its home."""
    rng = np.random.default_rng(3)
    seen = set()
    for log2, n in itertools.product((4, 6, 8), (3, 9, 16, 40, 64, 200, 256)):
        if n > (1 << log2):
            continue
        for _ in range(6):
            keys = set()
            while len(keys) < n:
                a, b = sorted(int(x) for x in rng.integers(0, 5000, 2))
                if a != b:
                    keys.add((a, b))
            keys = sorted(keys)
            lo, hi = [k[0] for k in keys], [k[1] for k in keys]
            for order in (keys, keys[::-1], [keys[i] for i in rng.permutation(n)]):
                slots, overflow = ptm.probe_insert(order, log2)
                assert not overflow
                below = any(k is not None and s < ptm.home(k[0], k[1], log2) for s, k in enumerate(slots))
                assert below == ptm.wraps(lo, hi, log2), (log2, n)
                seen.add(below)
    assert seen == {True, False}


@pytest.mark.parametrize("start", [4, 5, 6, 8, 9])
def test_grown_log2_against_the_sequential_table(start):
    rng = np.random.default_rng(start)
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512):
        lo, hi = ptm.chain_pairs(n)
        keys = list(zip(lo.tolist(), hi.tolist()))
        for order in (keys, keys[::-1], [keys[i] for i in rng.permutation(n)], [keys[i] for i in rng.permutation(n)]):
            log2 = start
            while ptm.probe_insert(order, log2)[1]:          # finish_extract: overflow -> four times the slots -> again
                log2 += ptm.GROW_LOG2
            assert log2 == ptm.grown_log2(n, start), (n, start)
            slots, _ = ptm.probe_insert(order, log2)
            assert sorted(k for k in slots if k is not None) == sorted(keys)
    for n in (513, 600, -1):
        with pytest.raises(ValueError):
            ptm.grown_log2(n, start)
    assert [ptm.grown_log2(n, 4) for n in (16, 17, 64, 65, 256, 257, 512)] == [4, 6, 6, 8, 8, 10, 10]


EVERY_CUT, MORE_SLABS, exchange_volume = ptm.EVERY_CUT, ptm.MORE_SLABS, ptm.exchange_volume      # the slab cases of test_gpu_exchange_blocks.py


def test_the_exchange_volume_has_labels_on_both_sides_of_the_rule():
    vol = exchange_volume(np.uint32)
    want = onepass_c.extract(vol)
    assert want["pair_lo"].size == 46
    boxes = ptm.device_boxes(want["bbox"])
    from tissue_analysis_amd.distributed import slab_exclusive
    present = boxes[:, 0] != np.iinfo(np.int32).max
    first, last = boxes[:, 0].astype(np.int64), -boxes[:, 3].astype(np.int64)        # first and last plane of every label
    at_limit = just_above = 0
    for cuts in EVERY_CUT + MORE_SLABS:
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            excl = slab_exclusive(boxes, lo, hi)
            inside = present & (first >= lo)
            at_limit += int(np.sum(excl[inside & (last == hi - 2)]))          # ends at hi - 2: the last plane that is exclusive
            just_above += int(np.sum(inside & (last == hi - 1)))              # ends at hi - 1, in the next slab's halo: never
            assert excl[inside & (last == hi - 2)].all() and not excl[inside & (last == hi - 1)].any()
            if hi - 2 < lo:                              # a slab of one plane: nothing is exclusive
                assert not excl.any()
    assert at_limit > 0 and just_above > 0, (at_limit, just_above)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_slab_parts_merge_to_the_unsharded_oracle(dtype):
    vol = exchange_volume(dtype)
    want = onepass_c.extract(vol)
    L = int(want["max_label"])
    boxes = ptm.device_boxes(want["bbox"])
    for cuts in EVERY_CUT + MORE_SLABS:
        parts = [ptm.slab_local(vol, lo, hi, L) for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert_same_accumulators(onepass.merge(parts), want, "cuts=%s" % cuts)
        # private pairs are disjoint between the slabs; with every slab's travelling pairs they are the whole list again
        mine = [ptm.private(p, boxes, lo, hi) for p, lo, hi in zip(parts, cuts[:-1], cuts[1:])]
        sent = [ptm.travelling(p, boxes, lo, hi) for p, lo, hi in zip(parts, cuts[:-1], cuts[1:])]
        keys = [set(zip(m[0].tolist(), m[1].tolist())) for m in mine]
        assert sum(len(k) for k in keys) == len(set().union(*keys))
        for p, m, s in zip(parts, mine, sent):
            assert m[0].size + s[0].size == p["pair_lo"].size
        lo_, hi_, f_ = onepass.compact_pairs(np.concatenate([x[0] for x in mine + sent]), np.concatenate([x[1] for x in mine + sent]),
                                             np.concatenate([x[2] for x in mine + sent]))
        assert np.array_equal(lo_, want["pair_lo"]) and np.array_equal(hi_, want["pair_hi"]) and np.array_equal(f_, want["pair_faces"])
