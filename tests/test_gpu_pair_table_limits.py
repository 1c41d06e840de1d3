"""The device-global adjacency hash (PairTable, ta_device.h) at its limits: tables of 2^4 .. 2^9 slots (TA_OPT_PAIR_SLOTS) that
are exactly full, one pair short of room, grown several times inside one getter call, reused after they grew, filled by the
sweep's spill paths and by ta_adjacency_merge -- every result bit-exact against the C oracle in all seven integer arrays (a
re-run after an overflow must rebuild the per-label rows, not add to them).  pair_table_model.py says on the CPU which of these
tables have probe sequences that cross the table's end (all of the full ones) and what size a table must end at;
test_pair_table_cpu.py checks that model.  Every context here is the test's own: the options die with it."""
import numpy as np
import pytest

from oracle import onepass_c
from tissue_analysis_amd import _capi

import pair_table_model as ptm
from helpers import assert_same_accumulators, random_blocks, voronoi

pytestmark = pytest.mark.gpu

NO_ADJ = _capi.F_ALL & ~_capi.F_ADJACENCY


def _context(start, impl=0, shape=None, tile_planes=None):
    ctx = _capi.Context(0)
    ctx.set_option(_capi.OPT_PAIR_SLOTS, start)
    ctx.set_option(_capi.OPT_IMPL, impl)
    if shape is not None:
        ctx.set_option(_capi.OPT_SWEEP_SHAPE, shape)
    if tile_planes is not None:
        ctx.set_option(_capi.OPT_TILE_PLANES, tile_planes)
    return ctx


def _extract(ctx, vol, want, what, mask=_capi.F_ALL, shape=None):
    """set_volume + extract + every getter, compared with the oracle's `want`; answers the debug counters of the final run."""
    L = int(want["max_label"])
    ctx.set_volume(vol)
    ctx.extract(mask, L)
    count, bbox, sum1, sum2 = ctx.labels()
    w = dict(want)
    if mask & _capi.F_ADJACENCY:
        lo, hi, faces = ctx.adjacency()
    else:
        assert ctx.adjacency_size() == 0, what
        lo, hi, faces = np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 3), np.uint64)
        w.update(pair_lo=lo, pair_hi=hi, pair_faces=faces)
    got = dict(max_label=L, count=count, bbox=bbox, sum1=sum1, sum2=sum2, pair_lo=lo, pair_hi=hi, pair_faces=faces)
    assert_same_accumulators(got, w, what)
    d = ctx.debug_counters()
    assert d["range_flag"] == 0 and d["pair_overflow"] == 0, (what, d)      # (the flags of the LAST run: the one that fitted)
    if shape is not None:
        assert ctx.get_option(_capi.OPT_SWEEP_SHAPE_USED) == shape, what
    return d


# dtype, TA_OPT_IMPL, TA_OPT_SWEEP_SHAPE (uint32 sweep only; the rows are then wide enough for whole 512-column tiles)
VARIANTS = [(np.uint16, 0, None), (np.uint32, 0, 0), (np.uint32, 0, 1), (np.uint16, 1, None), (np.uint32, 1, None)]
VARIANT_IDS = ["u16-sweep", "u32-sweep-narrow", "u32-sweep-wide", "u16-naive", "u32-naive"]


def _chain(K, axis, dtype, shape):
    return ptm.wide_chain_volume(K, axis) if shape is not None else ptm.chain_volume(K, axis, dtype)


@pytest.mark.parametrize("dtype,impl,shape", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_table_exactly_full_does_not_grow(axis, dtype, impl, shape):
    """As many pairs as slots, 16 .. 512: every slot is taken, every one of these tables has probe sequences that cross its end,
    the last inserts probe (nearly) the whole table.  Exact, no overflow, no growth."""
    for K, start in ptm.FULL:
        vol = _chain(K, axis, dtype, shape)
        want = onepass_c.extract(vol)
        assert want["pair_lo"].size == K == 1 << start
        ctx = _context(start, impl, shape)
        try:
            what = "full K=%d axis=%d %s impl=%d shape=%s" % (K, axis, np.dtype(dtype).name, impl, shape)
            _extract(ctx, vol, want, what, shape=shape)
            assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == start, what
            _extract(ctx, vol, want, what + " again", shape=shape)           # (the collect left the full table clean)
            assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == start, what
        finally:
            ctx.close()


@pytest.mark.parametrize("dtype,impl,shape", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_pair_more_than_slots_grows_once(axis, dtype, impl, shape):
    """One pair more: the overflow flag, a table of four times the slots, a second sweep that rebuilds rows and table -- inside
    the first getter, without an error."""
    for K, start in ptm.ONE_MORE:
        vol = _chain(K, axis, dtype, shape)
        want = onepass_c.extract(vol)
        assert want["pair_lo"].size == K == (1 << start) + 1
        ctx = _context(start, impl, shape)
        try:
            what = "one more K=%d axis=%d %s impl=%d shape=%s" % (K, axis, np.dtype(dtype).name, impl, shape)
            _extract(ctx, vol, want, what, shape=shape)
            slots = ctx.get_option(_capi.OPT_PAIR_SLOTS)
            if K <= ptm.PROBES:
                assert slots == ptm.grown_log2(K, start) == start + 2, (what, slots)
            else:
                assert slots >= 11, (what, slots)
        finally:
            ctx.close()


def _voronoi_grows():
    vol = voronoi(*ptm.VORONOI_GROWS, np.uint32)
    vol.setflags(write=False)
    return vol, onepass_c.extract(vol)


@pytest.mark.parametrize("impl", [0, 1], ids=["sweep", "naive"])
def test_several_growth_steps_in_one_getter_call(impl):
    """2^4 -> 2^6 -> 2^8 for the 254 pairs of a Voronoi volume (and at 2^8 the table is nearly full and wraps), 2^4 -> 2^6 ->
    2^8 -> 2^10 for the 513-pair chain: three and four sweeps behind one call of ta_get_labels."""
    vol, want = _voronoi_grows()
    ctx = _context(4, impl)
    try:
        _extract(ctx, vol, want, "voronoi from 2^4 impl=%d" % impl)
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == ptm.grown_log2(254, 4) == 8
    finally:
        ctx.close()
    lo, hi = ptm.chain_pairs(513)
    assert ptm.final_log2(lo, hi, 4) == 10               # (no cluster of the 513 keys in 1024 slots is near the probe limit)
    for axis, dtype in ((2, np.uint16), (0, np.uint32)):
        chain = ptm.chain_volume(513, axis, dtype)
        ctx = _context(4, impl)
        try:
            _extract(ctx, chain, onepass_c.extract(chain), "chain 513 from 2^4 impl=%d" % impl)
            assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == 10
        finally:
            ctx.close()


def test_a_context_after_its_table_grew():
    vol, want = _voronoi_grows()
    small = voronoi((9, 12, 40), 6, 43, np.uint32)
    chain = ptm.chain_volume(17, 1, np.uint32)
    ctx = _context(4)
    try:
        _extract(ctx, vol, want, "first")
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == 8
        _extract(ctx, vol, want, "the same volume again")
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == 8
        for other in (small, chain):                      # fewer pairs than before: nothing of the old list may be left
            _extract(ctx, other, onepass_c.extract(other), "a smaller volume on the grown table")
            assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == 8
        _extract(ctx, vol, want, "without adjacency", mask=NO_ADJ)
        _extract(ctx, vol, want, "with adjacency again")
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == 8
        ctx.set_option(_capi.OPT_PAIR_SLOTS, 4)           # a starting size, never a way to shrink
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == 8
        _extract(ctx, vol, want, "after TA_OPT_PAIR_SLOTS = 4")
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == 8
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_the_sort_of_a_pair_list_with_one_bucket_more_than_a_scan_block(dtype):
    """ta_adjacency_get sorts the pairs by counting them into max_label + 3 buckets and scanning the counts, 2048 a workgroup
    (SCAN_PER_BLOCK of csrc/ta_counted.h): max_label = 2046 gives 2049 buckets, and the pairs of the largest label lie in the
    second scan block."""
    vol = voronoi((9, 12, 40), 6, 43, dtype)
    top = int(vol.max())
    vol[vol == top] = 2046
    want = onepass_c.extract(vol)
    assert int(want["max_label"]) + 3 == 2048 + 1 and int((want["pair_hi"] == 2046).sum()) > 0 and want["pair_lo"].size > 5
    ctx = _context(8)
    try:
        _extract(ctx, vol, want, "2049 buckets %s" % np.dtype(dtype).name)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype,shape", [(np.uint16, None), (np.uint32, 0), (np.uint32, 1)], ids=["u16", "u32-narrow", "u32-wide"])
def test_the_spill_paths_insert_into_a_tiny_table(dtype, shape):
    """Thousands of cells of 30 voxels: a tile holds more labels and more pairs than its LDS tables, so the tile flush and both
    spill paths insert into the global table -- which starts at 16 slots and grows six times under them."""
    dims, n_labels, seed = ptm.SPILL_VOLUME
    vol = random_blocks(dims, n_labels, seed, dtype)
    want = onepass_c.extract(vol)
    ctx = _context(4, 0, shape, tile_planes=16)
    try:
        d = _extract(ctx, vol, want, "spills %s shape=%s" % (np.dtype(dtype).name, shape), shape=shape)
        assert d["label_spills"] > 0 and d["pair_spills"] > 0, d
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == ptm.final_log2(want["pair_lo"], want["pair_hi"], 4) == 16
        d = _extract(ctx, vol, want, "spills again", shape=shape)
        assert d["label_spills"] > 0 and d["pair_spills"] > 0, d
    finally:
        ctx.close()


def _keys(lo, hi):
    return (np.asarray(lo).astype(np.uint64) << np.uint64(32)) | np.asarray(hi).astype(np.uint64)


def _merge(ctx, keys, faces):
    keys, faces = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(faces, dtype=np.uint64)
    kp, fp = ctx.malloc(keys.nbytes), ctx.malloc(faces.nbytes)
    try:
        ctx.h2d(kp, keys)
        ctx.h2d(fp, faces)
        ctx.adjacency_merge(kp, fp, keys.size)
    finally:
        ctx.free(kp)
        ctx.free(fp)


def _einval(call):
    with pytest.raises(_capi.TissueScanError) as e:
        call()
    assert e.value.code == _capi.TA_EINVAL, e.value


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32], ids=["u16", "u32"])
def test_merge_on_a_full_table_and_the_merge_that_does_not_fit(dtype):
    """ta_adjacency_merge with the 16-pair chain in 16 slots.  Its own 16 keys again: every insert probes a full table and
    finds its key (faces doubled, same keys), the EMPTY_KEY padding of a gathered list is skipped.  One new key: TA_ECAPACITY --
    and the extraction is gone (the merge wrote over its list): TA_EINVAL from every getter until the next ta_extract."""
    vol = ptm.chain_volume(16, 2, dtype)
    want = onepass_c.extract(vol)
    L = int(want["max_label"])
    own = _keys(want["pair_lo"], want["pair_hi"])
    ctx = _context(4)
    try:
        _extract(ctx, vol, want, "chain 16")
        rng = np.random.default_rng(7)
        order = rng.permutation(16)
        extra_faces = rng.integers(1, 1000, size=(16, 3)).astype(np.uint64)
        _merge(ctx, own[order], extra_faces[order])
        lo, hi, faces = ctx.adjacency()
        assert np.array_equal(lo, want["pair_lo"]) and np.array_equal(hi, want["pair_hi"])
        assert np.array_equal(faces, want["pair_faces"] + extra_faces)
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == 4 and ctx.adjacency_scope() == _capi.ADJ_LOCAL
        # ... the same with padding in between, on top of the merged list
        padded = np.full(24, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        padded[::3] = own[:8]
        pad_faces = np.full((24, 3), 5, dtype=np.uint64)
        _merge(ctx, padded, pad_faces)
        lo, hi, faces = ctx.adjacency()
        expect = want["pair_faces"] + extra_faces
        expect[:8] += np.uint64(5)
        assert np.array_equal(lo, want["pair_lo"]) and np.array_equal(hi, want["pair_hi"]) and np.array_equal(faces, expect)
        # one new key (labels 1 and 17 do not touch) does not fit; the key of the list that the table does hold is merged all the
        # same, so what the collect then writes over the extraction's list is neither that list nor the merged one
        with pytest.raises(_capi.TissueScanError) as e:
            _merge(ctx, np.concatenate([own[3:4], _keys([1], [17])]), np.full((2, 3), 7, dtype=np.uint64))
        assert e.value.code == _capi.TA_ECAPACITY, e.value
        for getter in (ctx.adjacency_size, ctx.adjacency, ctx.labels, ctx.adjacency_device, ctx.adjacency_scope,
                       lambda: _merge(ctx, own[:1], np.ones((1, 3), dtype=np.uint64))):
            _einval(getter)
        # the next extraction is whole again, on the same 16 slots
        _extract(ctx, vol, want, "after the failed merge")
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == 4 and ctx.adjacency_scope() == _capi.ADJ_LOCAL
        other = ptm.chain_volume(9, 0, dtype)
        _extract(ctx, other, onepass_c.extract(other), "a smaller volume after the failed merge")
    finally:
        ctx.close()
