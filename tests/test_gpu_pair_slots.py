"""The adjacency hash as ONE array of 32-byte slots {key, f0, f1, f2} (PairSlot, csrc/ta_device.h): every path that reads or
writes a slot -- the tile flush, the spill paths, the per-voxel cross-check kernel, the collect with its self-clean, the clear
before a re-run, pack_shared / insert_blocks -- against the numpy oracle (oracle/onepass.py), bit for bit.

Three volumes, each computed once with its oracle and left unchanged:
  cells  16 x 16 x 1024 uint32 of 2 x 2 x 2 cells: 90 048 pairs, far more than a tile's LDS tables hold and more than the
         2^14 slots the table starts with -- it regrows (2^14 -> 2^16 -> 2^18), each time cleared and refilled;
  chain  56 pairs in a table fixed at 64 slots (7/8 full), the labels shifted until some probe sequence MUST run past the last
         slot and wrap (pair_table_model.wraps says so on the CPU, whatever the insertion order);
  wall   64 x 64 x 1024 uint32, two labels, one pair: flat walls across each of the three axes, swept with 8-plane tiles so
         that the pair's counts arrive from dozens of tiles and meet in one slot."""
import numpy as np
import pytest

from oracle import onepass
from tissue_analysis_amd import _capi

import pair_table_model as ptm
from helpers import assert_same_accumulators
from test_gpu_exchange_blocks import _assert_global, _assert_rows, _exchange

pytestmark = pytest.mark.gpu

CHAIN_PAIRS, CHAIN_LOG2 = 56, 6                  # 56 of 64 slots: 7/8
CELLS_START_LOG2 = 14
_CACHE = {}


def _cells():
    a, b, c = np.meshgrid(np.arange(16) // 2, np.arange(16) // 2, np.arange(1024) // 2, indexing="ij")
    return (1 + (a * 8 + b) * 512 + c).astype(np.uint32)


def _chain():
    """The wide chain of 56 pairs along axis 2, its labels shifted by the smallest offset at which the table must wrap."""
    base = ptm.wide_chain_volume(CHAIN_PAIRS, 2)
    lo, hi = ptm.chain_pairs(CHAIN_PAIRS)
    for shift in range(0, 4096):
        if ptm.wraps(lo + np.uint32(shift), hi + np.uint32(shift), CHAIN_LOG2):
            return base + np.uint32(shift)
    raise AssertionError("no shift of the chain's labels makes a table of 2^%d slots wrap" % CHAIN_LOG2)


def _wall():
    vol = np.ones((64, 64, 1024), dtype=np.uint32)
    vol[:, 32:, :] = 2                           # across axis 1, through the whole volume
    vol[40:, :, 512:] = 2                        # ... and a corner block: faces across axes 0 and 2 too
    return vol


def _volume(name):
    if name not in _CACHE:
        vol = {"cells": _cells, "chain": _chain, "wall": _wall}[name]()
        vol.setflags(write=False)
        _CACHE[name] = (vol, onepass.extract(vol))
    return _CACHE[name]


def _context(pair_log2, impl=0, shape=None, tile_planes=None):
    ctx = _capi.Context(0)
    ctx.set_option(_capi.OPT_PAIR_SLOTS, pair_log2)
    ctx.set_option(_capi.OPT_IMPL, impl)
    if shape is not None:
        ctx.set_option(_capi.OPT_SWEEP_SHAPE, shape)
    if tile_planes is not None:
        ctx.set_option(_capi.OPT_TILE_PLANES, tile_planes)
    return ctx


def _extract(ctx, vol, want, what, new_volume=True):
    if new_volume:
        ctx.set_volume(vol)
    ctx.extract(_capi.F_ALL, int(want["max_label"]))
    count, bbox, sum1, sum2 = ctx.labels()
    lo, hi, faces = ctx.adjacency()
    got = dict(count=count, bbox=bbox, sum1=sum1, sum2=sum2, pair_lo=lo, pair_hi=hi, pair_faces=faces)
    assert_same_accumulators(got, want, what)
    d = ctx.debug_counters()
    assert d["range_flag"] == 0 and d["pair_overflow"] == 0, (what, d)
    return d


SWEEPS = [(0, 0), (0, 1), (1, None)]             # TA_OPT_IMPL, TA_OPT_SWEEP_SHAPE: both uint32 tile shapes, the cross-check kernel
SWEEP_IDS = ["narrow", "wide", "naive"]


@pytest.mark.parametrize("impl,shape", SWEEPS, ids=SWEEP_IDS)
def test_cells_regrow_a_small_table(impl, shape):
    vol, want = _volume("cells")
    assert want["pair_lo"].size == 90048 > 1 << (CELLS_START_LOG2 + 2)
    final = ptm.final_log2(want["pair_lo"], want["pair_hi"], CELLS_START_LOG2)
    assert final == CELLS_START_LOG2 + 4                                   # two growth steps, three sweeps
    ctx = _context(CELLS_START_LOG2, impl, shape)
    try:
        d = _extract(ctx, vol, want, "cells %s" % (shape,))
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == final
        if impl == 0:
            assert d["pair_spills"] > 0, d                                 # (a tile holds more pairs than its LDS table)
    finally:
        ctx.close()


@pytest.mark.parametrize("impl,shape", SWEEPS, ids=SWEEP_IDS)
def test_a_table_seven_eighths_full_wraps(impl, shape):
    vol, want = _volume("chain")
    assert want["pair_lo"].size == CHAIN_PAIRS == (1 << CHAIN_LOG2) * 7 // 8
    assert ptm.wraps(want["pair_lo"], want["pair_hi"], CHAIN_LOG2)
    ctx = _context(CHAIN_LOG2, impl, shape)
    try:
        _extract(ctx, vol, want, "chain %s" % (shape,))
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == CHAIN_LOG2            # it fitted: no growth
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", [0, 1], ids=["narrow", "wide"])
def test_one_pair_from_many_tiles(shape):
    """8-plane tiles: 8 tile layers along axis 0, and the wall across axis 1 crosses at least two tiles of every layer (a tile
    is at most 512 columns wide): the one slot of pair (1, 2) takes the adds of 16 tiles or more."""
    vol, want = _volume("wall")
    assert want["pair_lo"].tolist() == [1] and want["pair_hi"].tolist() == [2]
    assert want["pair_faces"].tolist() == [[32 * 512, 40 * 1024 + 24 * 512, 24 * 32]]       # (the oracle agrees with the closed form)
    ctx = _context(4, 0, shape, tile_planes=8)
    try:
        _extract(ctx, vol, want, "wall shape %d" % shape)
        assert ctx.get_option(_capi.OPT_TILE_PLANES_USED) == 8
    finally:
        ctx.close()


@pytest.mark.parametrize("name,cuts", [("cells", [0, 8, 16]), ("chain", [0, 2, 3]), ("wall", [0, 32, 64])])
def test_two_slabs_through_pack_shared_and_insert_blocks(name, cuts):
    vol, want = _volume(name)
    lists, sent, info = _exchange(vol, cuts, True)
    _assert_rows(info, want)
    assert all(s <= n for s, n in zip(sent, info["npairs"]))
    _assert_global(lists, True, info["boxes"], cuts, want)


def test_the_collect_leaves_every_slot_free_and_zero():
    """No clear runs between two extractions of a context: whatever the collect left in a slot -- a key, a count -- would be in
    the next list.  The same volume twice (every key finds its old slot: a stale count would be added to), then another volume
    (stale keys would be extra pairs), then the first again."""
    cells, want_cells = _volume("cells")
    chain, want_chain = _volume("chain")
    ctx = _context(CELLS_START_LOG2 + 4)
    try:
        _extract(ctx, cells, want_cells, "first")
        _extract(ctx, cells, want_cells, "the same volume again", new_volume=False)
        _extract(ctx, chain, want_chain, "another volume on the used table")
        _extract(ctx, cells, want_cells, "and back")
        assert ctx.get_option(_capi.OPT_PAIR_SLOTS) == CELLS_START_LOG2 + 4
    finally:
        ctx.close()
