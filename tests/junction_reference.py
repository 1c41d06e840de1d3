"""NumPy restatement of the junction tables (include/tissue_scan_junctions.h), independent of the product code.

A block at origin o holds the voxels o + d, d in {0, 1} along every axis with two voxels or more (d = 0 along an axis of one);
its order is the number of distinct labels in it, its position 2 o + 1 per axis (0 along an axis of one voxel).  Blocks of order 3
give the edge table, blocks of order 4 the vertex table: rows (labels ascending, n blocks, sum of positions), sorted by labels;
blocks of order 5 or more are counted."""
import numpy as np


def _as3d(V):
    V = np.asarray(V)
    return V[:, :, None] if V.ndim == 2 else V


def _blocks(V):
    """(mixed bool [B0, B1, B2], values [M, 2^k] sorted along the last axis, order [M]) of the blocks of the 3-D array V: `mixed`
    marks the blocks of more than one label, and only those (M of them) are stacked and sorted."""
    shifts = [(0, 1) if n >= 2 else (0,) for n in V.shape]
    nb = [max(n - 1, 1) for n in V.shape]
    views = []
    for d0 in shifts[0]:
        for d1 in shifts[1]:
            for d2 in shifts[2]:
                views.append(V[d0:d0 + nb[0], d1:d1 + nb[1], d2:d2 + nb[2]])
    mixed = np.zeros(nb, dtype=bool)
    for v in views[1:]:
        mixed |= v != views[0]
    vals = np.sort(np.stack([v[mixed] for v in views], axis=-1), axis=-1)
    order = 1 + (vals[:, 1:] != vals[:, :-1]).sum(axis=-1)
    return mixed, vals, order


def _rows(vals, order, want, pos):
    """The table of the blocks of order `want`: (labels int64 [R, want], n uint64 [R], sums uint64 [R, 3])."""
    sel = order == want
    if not sel.any():
        return np.zeros((0, want), dtype=np.int64), np.zeros(0, dtype=np.uint64), np.zeros((0, 3), dtype=np.uint64)
    v = vals[sel].astype(np.int64)                           # [N, 2^k] sorted
    first = np.ones(v.shape, dtype=bool)
    first[:, 1:] = v[:, 1:] != v[:, :-1]
    sets = v[first].reshape(-1, want)                        # the distinct labels of every block, ascending
    labels, inv, n = np.unique(sets, axis=0, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    sums = np.zeros((labels.shape[0], 3), dtype=np.uint64)
    np.add.at(sums, inv, pos[sel])
    return labels, n.astype(np.uint64), sums


def tables(V, first_owned=0, a0_origin=0):
    """((edge labels, n, sums), (vertex labels, n, sums), degenerate) of the label image V (2-D or 3-D, any layout).

    first_owned = 1: plane 0 of V is the low halo of a slab whose first owned plane has the global coordinate a0_origin along
    axis 0.  A block belongs to the slab that owns its upper plane, so every block of V counts either way; only the positions
    shift."""
    V = _as3d(V)
    mixed, vals, order = _blocks(V)
    idx = np.stack(np.nonzero(mixed), axis=-1).astype(np.int64)          # origins of the mixed blocks, [M, 3]
    idx[:, 0] += int(a0_origin) - int(first_owned)
    pos = (2 * idx + 1) * (np.array(V.shape) >= 2)
    pos = pos.astype(np.uint64)
    return _rows(vals, order, 3, pos), _rows(vals, order, 4, pos), int((order >= 5).sum())


def tables_by_plane_pairs(V, planes=1):
    """tables(V) of a large 3-D volume, `planes` layers of blocks at a time (one: a pair of planes; bounded memory), merged."""
    V = _as3d(V)
    if V.shape[0] < 2:
        return tables(V)
    return merge([tables(V[p:p + planes + 1], first_owned=1, a0_origin=p + 1) for p in range(0, V.shape[0] - 1, planes)])


def merge(parts):
    """Tables of the slabs of one volume as one: n and sums added over equal label sets, degenerate counts added."""
    out = []
    for k, width in ((0, 3), (1, 4)):
        labels = np.concatenate([p[k][0] for p in parts]).reshape(-1, width)
        n = np.concatenate([p[k][1] for p in parts])
        sums = np.concatenate([p[k][2] for p in parts]).reshape(-1, 3)
        if labels.shape[0]:
            uniq, inv = np.unique(labels, axis=0, return_inverse=True)
            inv = np.asarray(inv).reshape(-1)
            tn = np.zeros(uniq.shape[0], dtype=np.uint64)
            ts = np.zeros((uniq.shape[0], 3), dtype=np.uint64)
            np.add.at(tn, inv, n)
            np.add.at(ts, inv, sums)
            labels, n, sums = uniq, tn, ts
        out.append((labels, n, sums))
    return out[0], out[1], sum(int(p[2]) for p in parts)
