"""The sweep's tiles at their tallest, and label volumes that fill them.

kernels_scan.hip keeps the ten tile-local sums of a label in four packed u64 words (SumPack<P, B, C> in
ta_sweep_common.h): every sum gets exactly the bits its largest possible value takes in a tile of P planes x B rows x
C columns.  This file restates, in plain NumPy and without the library, (1) the tile each family of sweep kernels is
packed for, (2) the field widths that follow, and (3) volumes in which a label reaches those largest values.
test_sweep_tiles_cpu.py checks the restatement; test_gpu_sweep_tile_limits.py runs the volumes through the kernels.
"""
import numpy as np

# feature bits of include/tissue_scan.h: volume 1, bbox 2, moment1 4, moment2 8, adjacency 16
MASK_ADJ_MOM2, MASK_ADJ = 0x1f, 0x17
MASK_MOM2, MASK_MOM1 = 0x0f, 0x07


class Family(object):
    """One family of sweep kernels: how it is reached and the tile (P planes at the cap, B rows, C columns) it packs for.
    `shape` is the TA_OPT_SWEEP_SHAPE that selects it (None: the option does not apply), `words` the widths of its four
    packed words as ta_sweep_common.h computes them today."""

    def __init__(self, name, dtype, mask_mom2, mask_mom1, shape, P, B, C, words):
        self.name, self.dtype = name, np.dtype(dtype)
        self.mask_mom2, self.mask_mom1, self.shape = mask_mom2, mask_mom1, shape
        self.P, self.B, self.C, self.words = P, B, C, words

    @property
    def adjacency(self):
        return bool(self.mask_mom2 & 16)

    def __repr__(self):
        return self.name


FAMILIES = [
    Family("narrow_u32_adj", np.uint32, MASK_ADJ_MOM2, MASK_ADJ, 0, 48, 8, 256, (57, 56, 63, 63)),
    Family("wide_u32_adj", np.uint32, MASK_ADJ_MOM2, MASK_ADJ, 1, 32, 8, 512, (61, 55, 64, 64)),
    Family("u16_adj", np.uint16, MASK_ADJ_MOM2, MASK_ADJ, None, 32, 8, 512, (61, 55, 64, 64)),
    Family("u32_moments", np.uint32, MASK_MOM2, MASK_MOM1, None, 16, 16, 256, (57, 49, 59, 64)),
    Family("u16_moments", np.uint16, MASK_MOM2, MASK_MOM1, None, 32, 8, 512, (61, 55, 64, 64)),
]
FAMILY = dict((f.name, f) for f in FAMILIES)


# ---- SumPack, restated ------------------------------------------------------------------------------------------------------
def tri(n):
    """sum of i, i < n"""
    return n * (n - 1) // 2


def sq(n):
    """sum of i^2, i < n"""
    return (n - 1) * n * (2 * n - 1) // 6


def bits(x):
    return int(x).bit_length()


SUM_NAMES = ("n", "a", "b", "c", "aa", "ab", "ac", "bb", "bc", "cc")


def field_maxima(P, B, C):
    """The value each of the ten tile-local sums takes for a label that fills the tile: what SumPack sizes its fields for."""
    return dict(n=P * B * C,
                a=B * C * tri(P), b=P * C * tri(B), c=P * B * tri(C),
                aa=B * C * sq(P), ab=C * tri(P) * tri(B), ac=B * tri(P) * tri(C),
                bb=P * C * sq(B), bc=P * tri(B) * tri(C), cc=P * B * sq(C))


def field_bits(P, B, C):
    return dict((k, bits(v)) for k, v in field_maxima(P, B, C).items())


def word_widths(P, B, C):
    """w0 = cc | bc,  w1 = ac | aa,  w2 = c | a | n,  w3 = ab | bb | b"""
    b = field_bits(P, B, C)
    return (b["cc"] + b["bc"], b["ac"] + b["aa"], b["c"] + b["a"] + b["n"], b["ab"] + b["bb"] + b["b"])


def local_sums(mask):
    """The ten sums of the voxels of a boolean tile, in tile-local coordinates, as Python integers (int64 arithmetic)."""
    a, b, c = (x.astype(np.int64) for x in np.nonzero(mask))
    return dict(n=int(a.size), a=int(a.sum()), b=int(b.sum()), c=int(c.sum()),
                aa=int((a * a).sum()), ab=int((a * b).sum()), ac=int((a * c).sum()),
                bb=int((b * b).sum()), bc=int((b * c).sum()), cc=int((c * c).sum()))


# ---- the volumes --------------------------------------------------------------------------------------------------------------
X, Y, H = 7, 5, 3                  # the big label, the other big label, the label of voxel (0, 0, 0) where a pattern sets it
NOTCH0 = 20                        # the notch of tile t is NOTCH0 + t (tiles numbered in memory order)
PLANE0 = 10                        # label_per_plane: plane a holds PLANE0 + a
PATTERNS = ("all_but_origin", "notch_first", "notch_last", "notch_centre", "halves", "planes_alternate", "rows_alternate",
            "label_per_plane")
EXTENTS = ("whole", "ragged")


def extent_dims(fam, extent, row_extra=None):
    """"whole": 2 x 2 x 2 interior tiles, three of four tile columns with a non-zero origin.  "ragged": a short last band and
    a partial tile row and column; `row_extra` replaces the 8 extra columns (a row length that is no multiple of 16 bytes)."""
    P, B, C = fam.P, fam.B, fam.C
    if extent == "whole":
        return (2 * P, 2 * B, 2 * C)
    if extent == "ragged":
        return (2 * P + 3, 2 * B + 1, 2 * C + (8 if row_extra is None else row_extra))
    raise ValueError(extent)


def tile_origins(fam, dims):
    return [(i, j, k) for i in range(0, dims[0], fam.P) for j in range(0, dims[1], fam.B) for k in range(0, dims[2], fam.C)]


def make_volume(fam, pattern, extent="whole", row_extra=None, dims=None):
    """A C-contiguous volume of fam.dtype.  Where a pattern writes into every tile it writes relative to every tile origin
    (iP, jB, kC) of the volume; a voxel that falls outside a partial tile is left alone."""
    P, B, C = fam.P, fam.B, fam.C
    dims = extent_dims(fam, extent, row_extra) if dims is None else tuple(dims)
    vol = np.full(dims, X, dtype=fam.dtype)
    origins = tile_origins(fam, dims)

    def notch(offset, first=None):
        for t, (i, j, k) in enumerate(origins):
            p = (i + offset[0], j + offset[1], k + offset[2])
            if all(q < d for q, d in zip(p, dims)):
                vol[p] = first if (t == 0 and first is not None) else NOTCH0 + t

    if pattern == "all_but_origin":
        vol[0, 0, 0] = H
    elif pattern == "notch_first":
        notch((0, 0, 0), first=H)
    elif pattern == "notch_last":
        notch((P - 1, B - 1, C - 1))
    elif pattern == "notch_centre":
        notch((P // 2, B // 2, C // 2))
    elif pattern == "halves":
        vol[:, :, (np.arange(dims[2]) % C) >= C // 2] = Y
    elif pattern == "planes_alternate":
        vol[1::2, :, :] = Y
    elif pattern == "rows_alternate":
        vol[:, 1::2, :] = Y
    elif pattern == "label_per_plane":
        vol[:] = (PLANE0 + np.arange(dims[0])).astype(fam.dtype)[:, None, None]
        vol[0, 0, 0] = H
    else:
        raise ValueError(pattern)
    return vol


def make_slab(fam, pattern):
    """(1 + 2P, 2B, 2C): one low halo plane (of Y: every voxel of the first owned plane has a face into it) in front of the
    "whole" volume of the pattern -- the owned planes start at buffer plane 1, and so do the tiles."""
    owned = make_volume(fam, pattern, "whole")
    halo = np.full((1,) + owned.shape[1:], Y, dtype=fam.dtype)
    return np.ascontiguousarray(np.concatenate([halo, owned], axis=0))
