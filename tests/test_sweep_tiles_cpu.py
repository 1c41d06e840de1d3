"""sweep_tiles.py does what it claims, with no GPU: its volumes put a label's tile-local sums exactly at the values SumPack
(ta_sweep_common.h) sizes its packed fields for, and its restated field widths are the ones the header computes today."""
import numpy as np
import pytest

import sweep_tiles as st

# The widths of w0 .. w3 at each family's cap, recomputed on the CPU from the header's formulas: the RECORD of what the header
# computes today.  A changed tile constant (rows, columns, cap) must change this table deliberately.
WIDTHS_TODAY = {
    "narrow_u32_adj": (48, 8, 256, (57, 56, 63, 63)),
    "wide_u32_adj": (32, 8, 512, (61, 55, 64, 64)),
    "u16_adj": (32, 8, 512, (61, 55, 64, 64)),
    "u32_moments": (16, 16, 256, (57, 49, 59, 64)),
    "u16_moments": (32, 8, 512, (61, 55, 64, 64)),
}


@pytest.mark.parametrize("fam", st.FAMILIES, ids=repr)
def test_restated_widths_are_the_recorded_ones(fam):
    P, B, C, words = WIDTHS_TODAY[fam.name]
    assert (fam.P, fam.B, fam.C) == (P, B, C)
    assert fam.words == words
    assert st.word_widths(P, B, C) == words


@pytest.mark.parametrize("fam", st.FAMILIES, ids=repr)
def test_the_four_words_fit_64_bits(fam):
    assert all(w <= 64 for w in st.word_widths(fam.P, fam.B, fam.C))


def test_how_far_each_cap_is_from_the_first_height_that_no_longer_fits():
    """What makes the cap a cap: the 8 x 512 tiles overflow a word with one more plane, the moments-only uint32 tiles (a word
    that ends at bit 64 as well) with two more; only the narrow tiles have room, up to 58 planes."""
    first_too_tall = {}
    for f in st.FAMILIES:
        p = f.P
        while max(st.word_widths(p, f.B, f.C)) <= 64:
            p += 1
        first_too_tall[f.name] = p
    assert first_too_tall == {"narrow_u32_adj": 59, "wide_u32_adj": 33, "u16_adj": 33, "u32_moments": 18, "u16_moments": 33}


def test_closed_forms():
    for n in (1, 2, 7, 48, 512):
        i = np.arange(n, dtype=np.int64)
        assert st.tri(n) == int(i.sum()) and st.sq(n) == int((i * i).sum())
    assert [st.bits(x) for x in (0, 1, 2, 255, 256, 2 ** 63)] == [0, 1, 2, 8, 9, 64]


@pytest.mark.parametrize("extent", st.EXTENTS)
@pytest.mark.parametrize("pattern", ["all_but_origin", "notch_first"])
@pytest.mark.parametrize("fam", st.FAMILIES, ids=repr)
def test_the_big_label_sits_at_the_field_maxima_in_tile_0(fam, pattern, extent):
    vol = st.make_volume(fam, pattern, extent)
    assert vol.dtype == fam.dtype and vol.flags.c_contiguous
    assert vol.shape == st.extent_dims(fam, extent)
    assert vol.flat[0] != st.X                      # X is not the hot label: its tile sums take the record path
    tile = vol[:fam.P, :fam.B, :fam.C]
    got = st.local_sums(tile == st.X)
    want = st.field_maxima(fam.P, fam.B, fam.C)
    assert got["n"] == want["n"] - 1 == fam.P * fam.B * fam.C - 1
    for k in st.SUM_NAMES[1:]:                      # the missing voxel has coordinates (0, 0, 0): nine sums at their maxima
        assert got[k] == want[k], k
        assert st.bits(got[k]) == st.field_bits(fam.P, fam.B, fam.C)[k], k


@pytest.mark.parametrize("fam", st.FAMILIES, ids=repr)
def test_patterns_do_what_they_say(fam):
    P, B, C = fam.P, fam.B, fam.C
    for extent in st.EXTENTS:
        dims = st.extent_dims(fam, extent)
        origins = st.tile_origins(fam, dims)
        assert len(origins) == (8 if extent == "whole" else 27)
        v = st.make_volume(fam, "all_but_origin", extent)
        assert int((v != st.X).sum()) == 1 and v[0, 0, 0] == st.H
        v = st.make_volume(fam, "notch_first", extent)
        firsts = [int(v[o]) for o in origins]
        assert firsts[0] == st.H and len(set(firsts)) == len(origins) and st.X not in firsts
        assert int((v != st.X).sum()) == len(origins)
        for name, off in (("notch_last", (P - 1, B - 1, C - 1)), ("notch_centre", (P // 2, B // 2, C // 2))):
            v = st.make_volume(fam, name, extent)
            inside = [tuple(o[d] + off[d] for d in range(3)) for o in origins]
            inside = [p for p in inside if all(p[d] < dims[d] for d in range(3))]
            assert len(inside) >= 8 and int((v != st.X).sum()) == len(inside)
            assert all(v[p] != st.X for p in inside) and v[0, 0, 0] == st.X
        v = st.make_volume(fam, "halves", extent)
        assert set(np.unique(v)) == {st.X, st.Y}
        assert (v[:, :, :C // 2] == st.X).all() and (v[:, :, C // 2:C] == st.Y).all() and (v[:, :, C:C + C // 2] == st.X).all()
        # P * B axis-2 faces of the pair inside each whole tile, P * (B - 1) * C / (P - 1) * B * C on the other axes
        t = v[:P, :B, :C]
        assert int((t[:, :, 1:] != t[:, :, :-1]).sum()) == P * B
        t = st.make_volume(fam, "planes_alternate", extent)[P:2 * P, :B, C:2 * C]
        assert int((t[1:] != t[:-1]).sum()) == (P - 1) * B * C and not (t[:, 1:] != t[:, :-1]).any()
        t = st.make_volume(fam, "rows_alternate", extent)[:P, B:2 * B, :C]
        assert int((t[:, 1:] != t[:, :-1]).sum()) == P * (B - 1) * C and not (t[1:] != t[:-1]).any()
        v = st.make_volume(fam, "label_per_plane", extent)
        assert v[0, 0, 0] == st.H and v[0, 0, 1] == st.PLANE0
        assert all((v[a] == st.PLANE0 + a).all() for a in range(1, dims[0]))
    slab = st.make_slab(fam, "notch_first")
    assert slab.shape == (P + 1 + P, 2 * B, 2 * C) and (slab[0] == st.Y).all() and slab[1, 0, 0] == st.H
    assert slab.flags.c_contiguous and slab.dtype == fam.dtype


def test_unaligned_rows_of_the_guarded_load_cases():
    for fam, extra in ((st.FAMILY["u16_adj"], 9), (st.FAMILY["narrow_u32_adj"], 3), (st.FAMILY["u32_moments"], 3),
                       (st.FAMILY["u16_moments"], 9)):
        v = st.make_volume(fam, "notch_last", "ragged", row_extra=extra)
        assert v.shape == (2 * fam.P + 3, 2 * fam.B + 1, 2 * fam.C + extra)
        assert (v.shape[2] * fam.dtype.itemsize) % 16 != 0
