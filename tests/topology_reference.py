"""A NumPy-only restatement of include/tissue_scan_topology.h: the twelve block counts per label over the 2 x 2 x 2 blocks of a label
volume padded by one layer of "no label", what the host derives from them, the launch plan of the pass (csrc/kernels_topology.hip
over csrc/ta_range_plan.h) and shapes whose Euler numbers are known.  Nothing here loads the library."""
import collections

import numpy as np

import range_tiles as rt

MAX_GROUPS = 1024                       # TP_MAX_GROUPS of csrc/ta_topology.h
LABEL_SLOTS = 768                       # TP_SLOTS
VOXEL_CAP_LOG2 = 31
COLUMNS = ("n0", "n1", "n2", "n3", "v", "e")
UPPER = ((4, 5, 6, 7), (2, 3, 6, 7), (1, 3, 5, 7))      # the upper half of a block along memory axis 0, 1, 2
LOWER_OF_7 = (3, 5, 6)                                    # the lower neighbour of voxel 7 along axis 0, 1, 2

Plan = collections.namedtuple("Plan", "ncb nrb npb tiles per groups tiles_in_last_group")


def blocks(V, rows=None):
    """int64 [B, 8]: the rows of the eight voxels of every block of V (3-D, memory order), column 4a + 2b + c; -1 outside the
    volume.  rows: the row of every voxel when that is not its label (a compacted context)."""
    V = np.asarray(V)
    n = V.shape
    P = np.full((n[0] + 2, n[1] + 2, n[2] + 2), -1, dtype=np.int64)
    P[1:-1, 1:-1, 1:-1] = V.astype(np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    views = [P[a:a + n[0] + 1, b:b + n[1] + 1, c:c + n[2] + 1].reshape(-1) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    return np.stack(views, axis=1)


def _count(rows_of_blocks, nrows):
    r = rows_of_blocks[rows_of_blocks >= 0]
    assert not r.size or int(r.max()) < nrows
    return np.bincount(r, minlength=nrows).astype(np.uint64)


def _all_equal(X, cols):
    first = X[:, cols[0]]
    same = first >= 0
    for c in cols[1:]:
        same &= X[:, c] == first
    return np.where(same, first, -1)


def _distinct(X, cols):
    """The distinct rows among the columns `cols` of every block, once each (flat)."""
    S = np.sort(X[:, cols], axis=1)
    head = np.ones(S.shape, dtype=bool)
    head[:, 1:] = S[:, 1:] != S[:, :-1]
    return S[head & (S >= 0)]


def counts(V, nrows, rows=None):
    """The twelve columns of the header for the volume V: a dict of uint64 arrays n0, n3, v [nrows] and n1, n2, e [nrows, 3]."""
    X = blocks(V, rows)
    out = {"n0": _count(X[:, 7], nrows), "n3": _count(_all_equal(X, list(range(8))), nrows), "v": _count(_distinct(X, list(range(8))), nrows)}
    out["n1"] = np.stack([_count(_all_equal(X, [7, LOWER_OF_7[a]]), nrows) for a in range(3)], axis=1)
    out["n2"] = np.stack([_count(_all_equal(X, list(UPPER[a])), nrows) for a in range(3)], axis=1)
    out["e"] = np.stack([_count(_distinct(X, list(UPPER[a])), nrows) for a in range(3)], axis=1)
    return out


def faces(c):
    """int64 [R, 3]: F_a = 2 n0 - n1[a]."""
    return 2 * c["n0"].astype(np.int64)[:, None] - c["n1"].astype(np.int64)


def euler(c, connectivity):
    i = dict((k, c[k].astype(np.int64)) for k in COLUMNS)
    if connectivity == 6:
        return i["n0"] - i["n1"].sum(axis=1) + i["n2"].sum(axis=1) - i["n3"]
    assert connectivity == 26
    return i["v"] - i["e"].sum(axis=1) + faces(c).sum(axis=1) - i["n0"]


def intrinsic(c, s):
    """(V1, V2) float64 [R] with the voxel size s per memory axis."""
    F = faces(c)
    n0, e = c["n0"].astype(np.int64), c["e"].astype(np.int64)
    area = (s[1] * s[2], s[0] * s[2], s[0] * s[1])
    v1 = sum(s[a] * (e[:, a] - (F.sum(axis=1) - F[:, a]) + n0).astype(np.float64) for a in range(3))
    v2 = sum(area[a] * (F[:, a] - n0).astype(np.float64) for a in range(3))
    return v1, v2


def euler_of_mask(mask):
    """(chi6, chi26) of a boolean volume."""
    c = counts(np.asarray(mask).astype(np.uint8), 2)
    return int(euler(c, 6)[1]), int(euler(c, 26)[1])


def exposed_faces(V, nrows):
    """uint64 [nrows]: the voxel faces of every label that do not lie between two of its voxels, the image border included --
    by looking at the six neighbours of every voxel."""
    V = np.asarray(V)
    P = np.full(tuple(d + 2 for d in V.shape), -1, dtype=np.int64)
    P[1:-1, 1:-1, 1:-1] = V
    inner = P[1:-1, 1:-1, 1:-1]
    out = np.zeros(nrows, dtype=np.uint64)
    for ax in range(3):
        for d in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[ax] = slice(d, d + V.shape[ax])
            out += np.bincount(inner[P[tuple(sl)] != inner], minlength=nrows).astype(np.uint64)
    return out


# ---- the launch plan ------------------------------------------------------------------------------------------------------------
def plan(dims, label_itemsize):
    """Tiles over the block positions [0, n0] x [0, n1] x [0, n2): one plane and one row of positions more than there are voxels."""
    n0, n1, n2 = (int(d) for d in dims)
    cols = rt.columns(label_itemsize)
    ncb, nrb, npb = rt._ceil(n2, cols), rt._ceil(n1 + 1, rt.WAVES), rt._ceil(n0 + 1, rt.PLANES)
    tiles = ncb * nrb * npb
    most = (1 << VOXEL_CAP_LOG2) // (rt.WAVES * cols * rt.PLANES)
    per = min(rt._ceil(tiles, MAX_GROUPS), most)
    groups = rt._ceil(tiles, per)
    return Plan(ncb, nrb, npb, tiles, per, groups, tiles - (groups - 1) * per)


def label_spill_bound(V):
    """Every label with a voxel at a position of a workgroup's range has a record there (its n0): of the D distinct ones at least
    D - LABEL_SLOTS find no slot.  A lower bound of the spill counter that holds whatever the hash does."""
    p = plan(V.shape, V.dtype.itemsize)
    n0, n1, n2 = V.shape
    tile = ((np.arange(n0) // rt.PLANES)[:, None, None] * p.nrb + (np.arange(n1) // rt.WAVES)[None, :, None]) * p.ncb \
        + (np.arange(n2) // rt.columns(V.dtype.itemsize))[None, None, :]
    g = (tile // p.per).reshape(-1).astype(np.int64)
    top = int(V.max()) + 1
    both = np.unique(g * top + V.reshape(-1).astype(np.int64))
    distinct = np.bincount(both // top, minlength=p.groups)
    return int(np.maximum(distinct - LABEL_SLOTS, 0).sum())


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) - (n - 1) / 2.0 for n in shape], indexing="ij")


def ball(r=5):
    x, y, z = _grid((2 * r + 3,) * 3)
    return x * x + y * y + z * z <= r * r


def shell(r_out=7, r_in=3):
    x, y, z = _grid((2 * r_out + 3,) * 3)
    d2 = x * x + y * y + z * z
    return (d2 <= r_out * r_out) & (d2 > r_in * r_in)


def torus(R=8, r=3, shape=None, centre=(0.0, 0.0)):
    """A solid torus around axis 0 (its circle in the plane of axes 1 and 2, about `centre`)."""
    n = 2 * (R + r) + 3
    x, y, z = _grid(shape or (2 * r + 3, n, n))
    return (np.sqrt((y - centre[0]) ** 2 + (z - centre[1]) ** 2) - R) ** 2 + x * x <= r * r


def double_torus(R=8, r=3):
    """Two solid tori side by side whose tubes merge where the circles touch: a handlebody of genus 2."""
    shape = (2 * r + 3, 2 * (R + r) + 3, 4 * R + 2 * r + 3)
    return torus(R, r, shape, (0.0, -float(R))) | torus(R, r, shape, (0.0, float(R)))


def eight_corners(shape=(5, 6, 7), label=3, dtype=np.uint16):
    V = np.zeros(shape, dtype=dtype)
    for i in (0, -1):
        for j in (0, -1):
            for k in (0, -1):
                V[i, j, k] = label
    return V


def voronoi(dims, n_cells, seed, dtype=np.uint16):
    """An exact Voronoi volume: every voxel takes the label 1 .. n_cells of the nearest of n_cells random sites (the smaller label
    among equally near ones).  Its cells are digitised convex polyhedra."""
    rng = np.random.default_rng(seed)
    sites = rng.uniform(0.0, 1.0, size=(n_cells, 3)) * (np.asarray(dims, dtype=np.float64) - 1.0)
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing="ij"), axis=-1)
    best = np.full(dims, np.inf)
    V = np.zeros(dims, dtype=dtype)
    for l, site in enumerate(sites, 1):
        d2 = ((grid - site) ** 2).sum(axis=-1)
        closer = d2 < best
        best[closer] = d2[closer]
        V[closer] = l
    return V


def drilled_voronoi(V, box=(3, 4, 5)):
    """A copy of the label volume V (convex cells: a Voronoi volume) with three edits, and what they are: a dict of
        tunnel    the label of the cell at the centre of V, through whose barycentre a line of voxels along axis 0, from one
                  side of the cell to the other, is handed to the cell before it
        cavity    the label of another cell, one voxel of which (all 26 neighbours in the cell) is handed to the new label `speck`
        box       a new label that fills the box [0, a) x [0, b) x [0, c) at the corner of V; `box_dims` = (a, b, c)."""
    V = np.array(V)
    n0, n1, n2 = V.shape
    top = int(V.max())
    V[:box[0], :box[1], :box[2]] = top + 1
    core = V[1:-1, 1:-1, 1:-1]
    solid = np.ones(core.shape, dtype=bool)                  # voxels whose 3 x 3 x 3 neighbourhood is their own cell
    for a in range(3):
        for b in range(3):
            for c in range(3):
                solid &= V[a:a + n0 - 2, b:b + n1 - 2, c:c + n2 - 2] == core
    tunnel = int(V[n0 // 2, n1 // 2, n2 // 2])
    _, j, k = (int(round(x)) for x in np.argwhere(V == tunnel).mean(axis=0))
    run = np.flatnonzero(V[:, j, k] == tunnel)
    assert run.size and run[0] > 0 and run[-1] < n0 - 1 and np.array_equal(run, np.arange(run[0], run[-1] + 1))
    thread = int(V[run[0] - 1, j, k])
    V[run, j, k] = thread
    at = np.argwhere(solid & (core != tunnel) & (core != thread) & (core != top + 1))[0] + 1
    cavity = int(V[tuple(at)])
    V[tuple(at)] = top + 2
    return V, dict(tunnel=tunnel, cavity=cavity, box=top + 1, box_dims=tuple(box), speck=top + 2, thread=thread)
