"""NumPy / SciPy restatement of the component table (include/tissue_scan_components.h), independent of the product code.

The voxels are the nodes of a graph, the pairs of face neighbours of equal label its edges;
scipy.sparse.csgraph.connected_components labels the nodes.  A row per component: (label, n voxels, first voxel, bounding box
min / max + 1, sum of coordinates), rows sorted by (label, first); the row image names every voxel's row."""
import numpy as np
from scipy import sparse
from scipy.sparse import csgraph

NONE = 0xFFFFFFFF


def _as3d(V):
    V = np.asarray(V)
    return V[:, :, None] if V.ndim == 2 else V


def component_ids(V):
    """(number of components, int64 image of a component id per voxel) of the 3-D array V."""
    V = _as3d(V)
    idx = np.arange(V.size, dtype=np.int64).reshape(V.shape)
    src, dst = [], []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        same = V[tuple(lo)] == V[tuple(hi)]
        src.append(idx[tuple(lo)][same])
        dst.append(idx[tuple(hi)][same])
    src, dst = np.concatenate(src), np.concatenate(dst)
    graph = sparse.coo_matrix((np.ones(src.size, dtype=np.int8), (src, dst)), shape=(V.size, V.size))
    count, ids = csgraph.connected_components(graph, directed=False)
    return int(count), ids.astype(np.int64).reshape(V.shape)


def table(V, first_owned=0, a0_origin=0):
    """((label int64 [R], n uint64 [R], first int64 [R, 3], bbox int64 [R, 6], sum1 uint64 [R, 3]), row image uint32 of V's shape)
    of the label image V (2-D or 3-D, any layout; coordinates are array axes).

    first_owned = 1: plane 0 of V is the low halo of a slab whose first owned plane has the global coordinate a0_origin along
    axis 0.  Connectivity runs over all of V; the rows count the owned voxels only, a component without one has no row and its
    voxels read NONE in the row image."""
    V = _as3d(V)
    count, ids = component_ids(V)
    owned = np.zeros(V.shape, dtype=bool)
    owned[first_owned:] = True
    coords = np.stack(np.nonzero(owned), axis=1).astype(np.int64)         # C order: ascending lexicographically
    comp = ids[owned]
    labels_of = np.zeros(count, dtype=np.int64)
    labels_of[ids.reshape(-1)] = V.reshape(-1)
    coords[:, 0] += int(a0_origin) - int(first_owned)
    n = np.bincount(comp, minlength=count).astype(np.uint64)
    sum1 = np.zeros((count, 3), dtype=np.uint64)
    np.add.at(sum1, comp, coords.astype(np.uint64))
    lo = np.full((count, 3), np.iinfo(np.int64).max, dtype=np.int64)
    hi = np.full((count, 3), np.iinfo(np.int64).min, dtype=np.int64)
    np.minimum.at(lo, comp, coords)
    np.maximum.at(hi, comp, coords)
    first = np.zeros((count, 3), dtype=np.int64)
    seen, where = np.unique(comp, return_index=True)                       # the first occurrence in C order
    first[seen] = coords[where]
    have = np.flatnonzero(n > 0)
    order = have[np.lexsort((first[have, 2], first[have, 1], first[have, 0], labels_of[have]))]
    row_of = np.full(count, NONE, dtype=np.uint32)
    row_of[order] = np.arange(order.size, dtype=np.uint32)
    rows = (labels_of[order], n[order], first[order], np.concatenate([lo[order], hi[order] + 1], axis=1), sum1[order])
    return rows, row_of[ids]


def slabs(V, cuts):
    """The per-slab tables of V cut along axis 0 at `cuts`, each slab but the first with a low halo plane, and the seams between
    them: ([rows of slab k], [(row image of slab k's top owned plane, row image of slab k + 1's halo plane)])."""
    V = _as3d(V)
    edges = [0] + [int(c) for c in cuts] + [V.shape[0]]
    parts, images = [], []
    for lo, hi in zip(edges[:-1], edges[1:]):
        halo = 1 if lo > 0 else 0
        rows, image = table(V[lo - halo:hi], first_owned=halo, a0_origin=lo)
        parts.append(rows)
        images.append(image)
    seams = [(images[k][-1], images[k + 1][0]) for k in range(len(parts) - 1)]
    return parts, seams


def split(V):
    """(V with every component but the largest of its label renamed to a new id above the largest label, in row order;
    {new id: old label}).  Largest: most voxels, then the smaller first voxel."""
    V = _as3d(V)
    (label, n, first, bbox, sum1), image = table(V)
    new = split_labels(label, n)
    out = new[image.astype(np.int64)].astype(np.int64)
    changed = new != label
    return out, dict(zip(new[changed].tolist(), label[changed].tolist()))


def largest_rows(label, n):
    keep = np.zeros(label.size, dtype=bool)
    for l in np.unique(label):
        rows = np.flatnonzero(label == l)
        keep[rows[np.argmax(n[rows])]] = True                             # (argmax: the first of equal ones, the smaller first voxel)
    return keep


def split_labels(label, n, next_label=None):
    new = label.copy()
    other = ~largest_rows(label, n)
    start = int(label.max()) + 1 if next_label is None else int(next_label)
    new[other] = start + np.arange(int(other.sum()))
    return new


def erase_labels(label, n, min_voxels, erase_value=0):
    new = label.copy()
    new[~largest_rows(label, n) & (n < min_voxels)] = erase_value
    return new


def erase(V, min_voxels, erase_value=0):
    V = _as3d(V)
    (label, n, first, bbox, sum1), image = table(V)
    return erase_labels(label, n, min_voxels, erase_value)[image.astype(np.int64)].astype(np.int64)
