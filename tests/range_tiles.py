"""The tile ranges of the six range passes (csrc/ta_range_plan.h), and label volumes that exercise them.

kernels_signal, _overlap, _wallgeo, _profile, _sighist and _sigmoments.hip share one scheme: a tile is WAVES rows x 64 * VPL columns
x PLANES planes (VPL = 16 / sizeof(label) voxels a lane), a workgroup takes `per` consecutive tiles (column blocks first, then row
blocks, then plane blocks), keeps open-addressed LDS tables for the whole range, and a record that finds no LDS slot goes to the
global rows.  This file restates, in plain Python and without the library, (1) the plan range_tiles / plan_ranges of
ta_range_plan.h compute, (2) which workgroup walks which voxel, and from it the spills no hash can avoid, and (3) label volumes
that are cheap to make at the shapes that reach multi-tile ranges.  test_range_tiles_cpu.py checks the restatement, also against
the header itself (tests/native/range_plan.cpp); test_gpu_tile_ranges.py and test_gpu_feature_table_spills.py run the volumes
through the kernels and compare the plan with the one the device reports.
"""
import collections

import numpy as np

WAVES, PLANES = 4, 16                                     # rows and planes of a tile, all six passes
MAX_GROUPS = {"signal": 1024, "overlap": 1024, "wallgeo": 4096, "profile": 4096, "sighist": 65536, "sigmoments": 1024}
# a workgroup's LDS rows count in u32
VOXEL_CAP_LOG2 = {"signal": 31, "overlap": 31, "wallgeo": 30, "profile": 30, "sighist": 31, "sigmoments": 31}
# LDS slots of a workgroup: a record spills only when the table it goes to is out of reach
LABEL_SLOTS = {"signal": 512, "sigmoments": 448}
KEY_SLOTS = {"profile": 1024, "sighist": 39}              # (row, shell) keys; rows of 256 digit counters
PAIR_SLOTS = {"signal": 2048, "overlap": 2048, "wallgeo": 512}

Plan = collections.namedtuple("Plan", "ncb nrb npb tiles per groups tiles_in_last_group")


def _ceil(a, b):
    return (a + b - 1) // b


def columns(label_itemsize):
    return 64 * (16 // int(label_itemsize))


def plan(dims, first_owned, label_itemsize, which):
    """dims: the buffer dims in memory order (the halo plane included when first_owned == 1)."""
    n0, n1, n2 = (int(d) for d in dims)
    cols = columns(label_itemsize)
    ncb, nrb, npb = _ceil(n2, cols), _ceil(n1, WAVES), _ceil(n0 - int(first_owned), PLANES)
    tiles = ncb * nrb * npb
    most = (1 << VOXEL_CAP_LOG2[which]) // (WAVES * cols * PLANES)
    per = min(_ceil(tiles, MAX_GROUPS[which]), most)
    groups = _ceil(tiles, per)
    return Plan(ncb, nrb, npb, tiles, per, groups, tiles - (groups - 1) * per)


def vector_path(dims, label_itemsize):
    """Whole 16-byte strips (of an aligned buffer): the kernels take the vector loads."""
    return int(dims[2]) % (16 // int(label_itemsize)) == 0


def group_image(dims, first_owned, label_itemsize, which, p=None):
    """int64 image of the buffer: the workgroup that walks each voxel, -1 in the halo plane (p: a plan other than the pass's plain one)."""
    n0, n1, n2 = (int(d) for d in dims)
    p = p or plan(dims, first_owned, label_itemsize, which)
    pb = (np.arange(n0) - int(first_owned)) // PLANES
    rb = np.arange(n1) // WAVES
    cb = np.arange(n2) // columns(label_itemsize)
    tile = (pb[:, None, None] * p.nrb + rb[None, :, None]) * p.ncb + cb[None, None, :]
    g = tile // p.per
    g[:int(first_owned)] = -1
    return g


def _distinct_per_group(groups, keys, ngroups):
    """Distinct keys among the records of each group."""
    if not keys.size:
        return np.zeros(ngroups, dtype=np.int64)
    uniq, inv = np.unique(keys, return_inverse=True)
    both = np.unique(groups.astype(np.int64) * int(uniq.size) + np.asarray(inv).reshape(-1).astype(np.int64))
    return np.bincount(both // int(uniq.size), minlength=ngroups)


def _unavoidable(distinct, slots):
    return int(np.maximum(distinct - slots, 0).sum())


def label_spill_bound(V, first_owned, which="signal"):
    """A workgroup's label table holds LABEL_SLOTS labels: of the D distinct labels of its range at least D - slots never get a
    slot, and each of them hands over at least one record.  Summed over the workgroups: a lower bound of the spill counter that
    holds whatever the hash does."""
    g = group_image(V.shape, first_owned, V.dtype.itemsize, which)
    own = g >= 0
    ngroups = plan(V.shape, first_owned, V.dtype.itemsize, which).groups
    return _unavoidable(_distinct_per_group(g[own], V[own].astype(np.uint64), ngroups), LABEL_SLOTS[which])


def wall_spill_bound(V, first_owned, which):
    """The same for the pair table of the signal or wall-geometry pass: a face is walked with its HIGHER voxel (the halo plane's
    faces with plane 1 belong to plane 1, the faces inside it to nobody)."""
    g = group_image(V.shape, first_owned, V.dtype.itemsize, which)
    gs, ks = [], []
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, V.shape[ax] - 1), slice(1, V.shape[ax])
        a, b, gb = V[tuple(lo)].astype(np.uint64), V[tuple(hi)].astype(np.uint64), g[tuple(hi)]
        m = (a != b) & (gb >= 0)
        gs.append(gb[m])
        ks.append((np.minimum(a[m], b[m]) << np.uint64(32)) | np.maximum(a[m], b[m]))
    ngroups = plan(V.shape, first_owned, V.dtype.itemsize, which).groups
    return _unavoidable(_distinct_per_group(np.concatenate(gs), np.concatenate(ks), ngroups), PAIR_SLOTS[which])


def overlap_spill_bound(A, B, first_owned):
    g = group_image(A.shape, first_owned, A.dtype.itemsize, "overlap")
    own = g >= 0
    keys = (A[own].astype(np.uint64) << np.uint64(32)) | B[own].astype(np.uint64)
    ngroups = plan(A.shape, first_owned, A.dtype.itemsize, "overlap").groups
    return _unavoidable(_distinct_per_group(g[own], keys, ngroups), PAIR_SLOTS["overlap"])


# ---- the shapes -----------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name dims dtype first_owned")


def _case(name, dims, dtype, first_owned=0):
    return Case(name, tuple(dims), np.dtype(dtype), first_owned)


# Buffer dims (the halo cases hold one low plane more: their owned planes are the other cases').  What each one is for is
# asserted by test_range_tiles_cpu.py.
CASES = [
    _case("a_u16", (257, 259, 24), np.uint16),                    # signal / overlap: 2 tiles a group, the last group 1; vector loads
    _case("a_u32", (257, 259, 24), np.uint32),
    _case("a_u16_scalar", (257, 259, 23), np.uint16),
    _case("b_u32", (17, 1025, 260), np.uint32),                   # a group = the two column blocks of a row block, the second 4 wide
    _case("b_u32_scalar", (17, 1025, 259), np.uint32),
    _case("c_u16", (257, 1025, 9), np.uint16),                    # 5 tiles a group (wall geometry: 2), scalar loads
    _case("c_u32", (257, 1025, 9), np.uint32),
    _case("c_u16_vector", (257, 1025, 8), np.uint16),
    _case("c_u32_vector", (257, 1025, 8), np.uint32),
    _case("a_u16_halo", (258, 259, 24), np.uint16, 1),
    _case("c_u32_halo", (258, 1025, 9), np.uint32, 1),
]
CASE = dict((c.name, c) for c in CASES)

SPILL_DIMS = (16, 4, 64)              # uint16: exactly one tile, one workgroup
SPILL_DIMS_WIDE = (33, 9, 70)         # uint32: 3 x 3 tiles, partial ones, rows that are no whole strips


# ---- the volumes ----------------------------------------------------------------------------------------------------------------
def block_labels(dims, dtype, seed, nlabels=300, block=(5, 7, 3)):
    """A coarse random grid of labels 1 .. nlabels, every cell repeated into a block of odd size: runs cross the tiles, the column
    blocks and the ranges.  Made in milliseconds."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(1, nlabels, size=[_ceil(d, b) for d, b in zip(dims, block)], endpoint=True)
    v = coarse
    for ax, b in enumerate(block):
        v = np.repeat(v, b, axis=ax)
    return np.ascontiguousarray(v[:dims[0], :dims[1], :dims[2]].astype(dtype))


def random_image(dims, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dtype).max, size=dims, endpoint=True).astype(dtype)


def permutation_labels(dims, dtype, seed):
    """Every voxel its own label: a permutation of 0 .. nvox - 1.  Every face is its own pair."""
    n = int(np.prod(dims))
    assert n - 1 <= np.iinfo(dtype).max
    return np.random.default_rng(seed).permutation(n).astype(dtype).reshape(dims)


def noise_box(V, box, seed, top):
    """A copy of V with the voxels of box = (slice, slice, slice) replaced by labels drawn from 0 .. top: more labels and pairs
    in the workgroups that walk the box than their LDS tables hold."""
    out = V.copy()
    rng = np.random.default_rng(seed)
    out[box] = rng.integers(0, top, size=out[box].shape, endpoint=True).astype(V.dtype)
    return out


def half_space(dims, dtype, axis, lo=2, hi=5, swap=False):
    """Label lo below the middle of `axis`, hi above (swap: the other way round): one pair, every face on one side."""
    v = np.full(dims, hi if swap else lo, dtype=dtype)
    idx = [slice(None)] * 3
    idx[axis] = slice(dims[axis] // 2, None)
    v[tuple(idx)] = lo if swap else hi
    return v
