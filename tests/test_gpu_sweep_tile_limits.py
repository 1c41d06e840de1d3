"""The sweep at its tallest tiles, with labels that fill them: bit-exact against the C oracle.

A label's ten tile-local sums live in four packed u64 words whose fields are exactly as wide as the largest value a tile of
P x B x C voxels can give them (SumPack, ta_sweep_common.h); in four of the five kernel families a word ends at bit 64.  A
field one bit short, a clamp that disagrees with the kernel, or a tile constant changed on one side only gives no fault and
no flag: one sum carries into its neighbour, for a label that nearly fills a tile and for no other.  The volumes of
sweep_tiles.py put labels there, TA_OPT_TILE_PLANES_USED proves the tile really ran at its cap, and the same tall tiles
reach the plane field of the run records, the closed form for leading uniform rows at nlead = P x rows-of-a-wave, whole-tile
face counts of one pair and the shift to global coordinates from non-zero tile origins."""
import numpy as np
import pytest

from oracle import onepass_c
from tissue_analysis_amd import _capi

import sweep_tiles as st
from helpers import assert_same_accumulators

pytestmark = pytest.mark.gpu


def _restore(ctx):
    ctx.set_option(_capi.OPT_TILE_PLANES, 0)
    ctx.set_option(_capi.OPT_SWEEP_SHAPE, -1)


def _setup(ctx, fam, tile_planes):
    ctx.set_option(_capi.OPT_IMPL, 0)
    ctx.set_option(_capi.OPT_SWEEP_SHAPE, -1 if fam.shape is None else fam.shape)
    ctx.set_option(_capi.OPT_TILE_PLANES, tile_planes)


def _sweep(ctx, fam, mask, want, what, used=None):
    """One sweep of the resident volume with `mask`, compared with the oracle's `want`; answers TA_OPT_TILE_PLANES_USED."""
    L = int(want["max_label"])
    ctx.extract(mask, L)
    count, bbox, sum1, sum2 = ctx.labels()
    if mask & _capi.F_ADJACENCY:
        lo, hi, faces = ctx.adjacency()
    else:
        assert ctx.adjacency_size() == 0, what
        lo, hi, faces = np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros((0, 3), np.uint64)
    got = dict(max_label=L, count=count, bbox=bbox, sum1=sum1, sum2=sum2, pair_lo=lo, pair_hi=hi, pair_faces=faces)
    w = dict(want)
    if not mask & _capi.F_MOMENT2:
        w["sum2"] = np.zeros_like(want["sum2"])              # not asked for: the columns stay zero
    if not mask & _capi.F_ADJACENCY:
        w.update(pair_lo=lo, pair_hi=hi, pair_faces=faces)   # ... and the pair arrays empty (asserted above)
    planes = ctx.get_option(_capi.OPT_TILE_PLANES_USED)
    if used is not None:
        assert planes == used, "%s: ran %d-plane tiles, the table says %d" % (what, planes, used)
    if fam.shape is not None:
        assert ctx.get_option(_capi.OPT_SWEEP_SHAPE_USED) == fam.shape, what
    assert_same_accumulators(got, w, what)
    d = ctx.debug_counters()
    assert d["label_spills"] == 0 and d["pair_spills"] == 0, "%s: the packed tables were bypassed: %s" % (what, d)
    assert d["range_flag"] == 0 and d["pair_overflow"] == 0, (what, d)
    return planes


_LAST = {}         # the volume and the oracle's answer of the last (family, pattern, extent): the two masks of a case share them


def _volume_and_oracle(fam, pattern, extent):
    key = (fam.name, pattern, extent)
    if _LAST.get("key") != key:
        vol = st.make_volume(fam, pattern, extent)
        vol.setflags(write=False)
        _LAST.update(key=key, vol=vol, want=onepass_c.extract(vol))
    return _LAST["vol"], _LAST["want"]


@pytest.mark.parametrize("moment2", [True, False], ids=["moment2", "moment1"])
@pytest.mark.parametrize("extent", st.EXTENTS)
@pytest.mark.parametrize("pattern", st.PATTERNS)
@pytest.mark.parametrize("fam", st.FAMILIES, ids=repr)
def test_tiles_at_the_cap_match_the_oracle(gpu_ctx, fam, pattern, extent, moment2):
    """Every family, with and without TA_F_MOMENT2 (four packed words a label slot, or two), every pattern, whole and ragged
    extents, 64 planes asked for: the launch must clamp to the family's cap and give the oracle's integers."""
    vol, want = _volume_and_oracle(fam, pattern, extent)
    mask = fam.mask_mom2 if moment2 else fam.mask_mom1
    try:
        _setup(gpu_ctx, fam, 64)
        gpu_ctx.set_volume(vol)
        _sweep(gpu_ctx, fam, mask, want, "%s %s %s mask=0x%x" % (fam, pattern, extent, mask), used=fam.P)
    finally:
        _restore(gpu_ctx)


@pytest.mark.parametrize("pattern", ["all_but_origin", "notch_first"])
@pytest.mark.parametrize("fam", st.FAMILIES, ids=repr)
def test_one_plane_below_the_cap_and_the_default_height(gpu_ctx, fam, pattern):
    """The same volume in tiles of cap - 1 planes (no tile boundary where the pattern has one) and of the automatic height:
    the same integers, and never a tile above the cap."""
    vol = st.make_volume(fam, pattern, "whole")
    want = onepass_c.extract(vol)
    try:
        for tile_planes in (fam.P - 1, 0):
            _setup(gpu_ctx, fam, tile_planes)
            gpu_ctx.set_volume(vol)
            for mask in (fam.mask_mom2, fam.mask_mom1):
                what = "%s %s tile_planes=%d mask=0x%x" % (fam, pattern, tile_planes, mask)
                planes = _sweep(gpu_ctx, fam, mask, want, what, used=fam.P - 1 if tile_planes else None)
                assert 1 <= planes <= fam.P, what
    finally:
        _restore(gpu_ctx)


EDGE_FAMILIES = [("u16_adj", 9), ("narrow_u32_adj", 3), ("u32_moments", 3), ("u16_moments", 9)]


@pytest.mark.parametrize("pattern", ["all_but_origin", "notch_last"])
@pytest.mark.parametrize("name,row_extra", EDGE_FAMILIES, ids=[f[0] for f in EDGE_FAMILIES])
def test_guarded_load_kernels_at_the_cap(name, row_extra, pattern):
    """Rows that are no multiple of 16 bytes in an adopted buffer with nothing readable behind it: every tile, the full ones
    too, runs the plain edge kernel (guarded scalar loads) -- the same packed tables at the same cap."""
    import torch
    fam = st.FAMILY[name]
    vol = st.make_volume(fam, pattern, "ragged", row_extra=row_extra)
    assert (vol.shape[2] * vol.dtype.itemsize) % 16 != 0
    want = onepass_c.extract(vol)
    t = torch.from_numpy(vol.view({2: np.int16, 4: np.int32}[vol.dtype.itemsize]).copy()).to("cuda:0")
    ctx = _capi.Context(0)
    try:
        _setup(ctx, fam, 64)
        ctx.set_volume_device(t.data_ptr(), vol.dtype.itemsize, vol.shape, keep=t)
        assert ctx.get_option(_capi.OPT_VOLUME_SLACK) == 0
        for mask in (fam.mask_mom2, fam.mask_mom1):
            _sweep(ctx, fam, mask, want, "edge %s %s mask=0x%x" % (fam, pattern, mask), used=fam.P)
    finally:
        ctx.close()


@pytest.mark.parametrize("pattern", ["notch_first", "label_per_plane"])
@pytest.mark.parametrize("name", ["u16_adj", "narrow_u32_adj", "wide_u32_adj"])
def test_a_slab_far_from_the_origin_at_the_cap(gpu_ctx, name, pattern):
    """A slab with a low halo plane whose first owned plane is plane 2000 of its volume: the box and the n * A0^2 terms of the
    shift to global coordinates at a full-size volume's coordinates, from tiles at the cap."""
    fam = st.FAMILY[name]
    slab = st.make_slab(fam, pattern)
    want = onepass_c.extract(slab, origin=(1999, 0, 0), own_first_plane=False)
    ptr = gpu_ctx.malloc(slab.nbytes)
    try:
        gpu_ctx.h2d(ptr, slab)
        _setup(gpu_ctx, fam, 64)
        gpu_ctx.set_volume_device(ptr, slab.dtype.itemsize, slab.shape, a0_origin=2000, has_low_halo=True)
        for mask in (fam.mask_mom2, fam.mask_mom1):
            _sweep(gpu_ctx, fam, mask, want, "slab %s %s mask=0x%x" % (fam, pattern, mask), used=fam.P)
    finally:
        _restore(gpu_ctx)
        gpu_ctx.set_volume(np.zeros((1, 1, 8), dtype=np.uint16))     # (the context lets go of the buffer before it is freed)
        gpu_ctx.free(ptr)
