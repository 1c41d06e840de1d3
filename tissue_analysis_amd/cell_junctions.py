"""Cell junctions of a label image: the lines where three cells meet (edges of the cell complex) and the points where four cells
meet (its vertices), from the exact integer tables of the junction pass (include/tissue_scan_junctions.h,
csrc/kernels_junctions.hip), and what follows from them on the host: positions, per-cell and per-wall lookups, incidence.

A block is a 2 x 2 x 2 set of voxels (2 x 2 in a 2-D image); its order is the number of distinct labels in it.  The edge table
has one row per set of three labels that share a block of order 3, the vertex table one row per set of four labels that share a
block of order 4: the number n of such blocks and the sum of their centres in doubled voxel-centre coordinates (exact
integers; sum / (2 n) is the mean centre in voxel units, the frame of `center_of_mass(real=False)`).  No label is special in the
tables: 0 and a background are labels like the others, and the methods take an `exclude`."""
from __future__ import annotations

import numpy as np

from ._tables import voxelsize3


def _member(values, chosen):
    chosen = np.asarray(list(chosen), dtype=np.int64).reshape(-1)
    return np.isin(values, chosen) if chosen.size else np.zeros(values.shape, dtype=bool)


def _table(labels, n, sums, width, what):
    labels, sums = np.asarray(labels).astype(np.int64), np.asarray(sums).astype(np.uint64)
    if labels.size == 0:                                   # (an empty list has no second dimension to check)
        labels = labels.reshape(0, width)
    if sums.size == 0:
        sums = sums.reshape(0, 3)
    n = np.asarray(n).astype(np.uint64).reshape(-1)
    if labels.ndim != 2 or labels.shape[1] != width:
        raise ValueError("%s_labels must have shape (rows, %d)" % (what, width))
    if n.shape != (labels.shape[0],) or sums.shape != (labels.shape[0], 3):
        raise ValueError("%s_n must have shape (rows,) and %s_sum shape (rows, 3)" % (what, what))
    if labels.size and (labels.min() < 0 or labels.max() > 0xFFFFFFFF):
        raise ValueError("labels must fit in uint32")
    return labels, n, sums


def _pack(labels):
    """One sortable key per row of at most four uint32 labels: a structured view would do as well; two uint64 words compare
    faster.  Returns (hi, lo) with the row's labels packed big-endian, missing leading columns as 0."""
    l = labels.astype(np.uint64)
    w = l.shape[1]
    pad = np.zeros((l.shape[0], 4 - w), dtype=np.uint64)
    l = np.concatenate([pad, l], axis=1)
    return (l[:, 0] << np.uint64(32)) | l[:, 1], (l[:, 2] << np.uint64(32)) | l[:, 3]


def _rank_keys(*tables):
    """Dense ranks of the rows of several label tables under one common order: equal rows get equal ranks."""
    his, los = zip(*[_pack(t) for t in tables])
    hi, lo = np.concatenate(his), np.concatenate(los)
    order = np.lexsort((lo, hi))
    shi, slo = hi[order], lo[order]
    new = np.ones(order.size, dtype=bool)
    new[1:] = (shi[1:] != shi[:-1]) | (slo[1:] != slo[:-1])
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.cumsum(new) - 1
    out, at = [], 0
    for t in tables:
        out.append(rank[at:at + t.shape[0]])
        at += t.shape[0]
    return out


class CellJunctions(object):
    """The junction tables of one label image.

        edge_labels     int64 (E, 3), a < b < c in every row, rows ascending; the label ids as stored in the image
        edge_n          uint64 (E,)   blocks of order 3 with exactly these labels
        edge_sum        uint64 (E, 3) sum of their doubled centres, array axes
        vertex_labels, vertex_n, vertex_sum     the same for the blocks of order 4: (V, 4), (V,), (V, 3)
        degenerate      blocks of five labels or more (they enter no row)
        voxelsize       three floats
        ms              (milliseconds of the walks over the volume, milliseconds after them) on the device; None for host tables
    """

    def __init__(self, edge_labels, edge_n, edge_sum, vertex_labels, vertex_n, vertex_sum, degenerate=0, voxelsize=(1.0, 1.0, 1.0),
                 ms=None):
        self.edge_labels, self.edge_n, self.edge_sum = _table(edge_labels, edge_n, edge_sum, 3, "edge")
        self.vertex_labels, self.vertex_n, self.vertex_sum = _table(vertex_labels, vertex_n, vertex_sum, 4, "vertex")
        self.degenerate = int(degenerate)
        self.voxelsize = voxelsize3(voxelsize)
        self.ms = ms

    # -- positions
    def _positions(self, sums, n, real):
        pos = sums.astype(np.float64) / (2.0 * n.astype(np.float64))[:, None]
        return pos * np.asarray(self.voxelsize, dtype=np.float64) if real else pos

    def edge_centroids(self, real=True):
        """float64 (E, 3): the mean centre of every edge's blocks, sum / (2 n), in voxel units or times the voxel size."""
        return self._positions(self.edge_sum, self.edge_n, real)

    def vertex_positions(self, real=True):
        """float64 (V, 3): the mean centre of every vertex's blocks."""
        return self._positions(self.vertex_sum, self.vertex_n, real)

    def cell_vertices(self, real=True, exclude=()):
        """{(a, b, c, d): xyz} of the vertices none of whose labels is in `exclude`."""
        keep = ~_member(self.vertex_labels, exclude).any(axis=1)
        pos = self.vertex_positions(real)[keep]
        return dict((tuple(l), p) for l, p in zip(self.vertex_labels[keep].tolist(), pos))

    def wall_edges(self, exclude=()):
        """{(a, b, c): (n, xyz in real units)} of the edges none of whose labels is in `exclude`."""
        keep = ~_member(self.edge_labels, exclude).any(axis=1)
        pos = self.edge_centroids(True)[keep]
        return dict((tuple(l), (int(n), p)) for l, n, p in zip(self.edge_labels[keep].tolist(), self.edge_n[keep].tolist(), pos))

    # -- lookups: indices of rows
    def edges_of_wall(self, a, b):
        """Rows of the edge table that hold both `a` and `b`: the edges that bound the wall between the two cells."""
        l = self.edge_labels
        return np.flatnonzero((l == int(a)).any(axis=1) & (l == int(b)).any(axis=1)) if int(a) != int(b) else np.zeros(0, dtype=np.int64)

    def edges_of_cell(self, label):
        return np.flatnonzero((self.edge_labels == int(label)).any(axis=1))

    def vertices_of_cell(self, label):
        return np.flatnonzero((self.vertex_labels == int(label)).any(axis=1))

    def incidence(self):
        """int64 (V, 4): for every vertex row (a, b, c, d) the rows of the edges (b, c, d), (a, c, d), (a, b, d) and (a, b, c)
        -- column k leaves the k-th label out -- and -1 where the edge table has no such row."""
        V, E = self.vertex_labels.shape[0], self.edge_labels.shape[0]
        out = np.full((V, 4), -1, dtype=np.int64)
        if not V or not E:
            return out
        subsets = [np.delete(self.vertex_labels, k, axis=1) for k in range(4)]
        ranks = _rank_keys(self.edge_labels, *subsets)
        edge_rank = ranks[0]                               # ascending already: the table is sorted and its rows are unique
        for k in range(4):
            at = np.searchsorted(edge_rank, ranks[k + 1])
            at_c = np.minimum(at, E - 1)
            out[:, k] = np.where(edge_rank[at_c] == ranks[k + 1], at_c, -1)
        return out

    # -- slabs
    @staticmethod
    def merge(parts, voxelsize=None):
        """The tables of the slabs of one volume (each a CellJunctions, positions in the volume's frame) as one: n and sums are
        added over equal label sets, and so are the degenerate counts."""
        parts = list(parts)
        if not parts:
            raise ValueError("nothing to merge")

        def fold(labels, n, sums, width):
            labels = np.concatenate(labels).reshape(-1, width)
            n, sums = np.concatenate(n), np.concatenate(sums).reshape(-1, 3)
            if not labels.shape[0]:
                return labels, n, sums
            uniq, inv = np.unique(labels, axis=0, return_inverse=True)
            inv = np.asarray(inv).reshape(-1)
            tn = np.zeros(uniq.shape[0], dtype=np.uint64)
            ts = np.zeros((uniq.shape[0], 3), dtype=np.uint64)
            np.add.at(tn, inv, n)
            np.add.at(ts, inv, sums)
            return uniq, tn, ts

        e = fold([p.edge_labels for p in parts], [p.edge_n for p in parts], [p.edge_sum for p in parts], 3)
        v = fold([p.vertex_labels for p in parts], [p.vertex_n for p in parts], [p.vertex_sum for p in parts], 4)
        return CellJunctions(e[0], e[1], e[2], v[0], v[1], v[2], sum(p.degenerate for p in parts),
                             parts[0].voxelsize if voxelsize is None else voxelsize)


def context_junctions(ctx, voxelsize=(1.0, 1.0, 1.0)):
    """The junction pass over the volume resident in the context `ctx`: a `CellJunctions`."""
    ctx.junctions_extract()
    (el, en, es), (vl, vn, vs), degenerate = ctx.junctions_get()
    return CellJunctions(el, en, es, vl, vn, vs, degenerate, voxelsize, ms=ctx.junctions_timing())


def cell_junctions(image, voxelsize=None, device=0):
    """The junction tables of a label image (a 2-D or 3-D integer array): a `CellJunctions`.  voxelsize: None = the image's own
    `voxelsize` attribute when it has one, else ones."""
    from .extraction import ResidentVolume
    if voxelsize is None:
        voxelsize = getattr(image, "voxelsize", None)
    if voxelsize is None:
        voxelsize = (1.0, 1.0, 1.0)
    rv = ResidentVolume(np.asarray(image), device=device)
    try:
        return rv.junctions(voxelsize)
    finally:
        rv.close()
