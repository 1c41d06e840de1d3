"""Connected components of the labels of an image: which labels are really several separate blobs, and the tables to give every
blob a label of its own or to erase the small ones (include/tissue_scan_components.h, csrc/kernels_components.hip).

A component is a maximal set of voxels of equal label joined through shared faces (the connectivity of `neighbors()` and of the
walls).  The table has one row per component, sorted by (label, first voxel); every number in it is an exact integer from the
GPU.  No label is special in the table: 0 and a background are labels like the others, and the methods take an `exclude`."""
from __future__ import annotations

import numpy as np

from . import _capi
from ._tables import voxelsize3

NONE = _capi.COMPONENT_NONE            # row image: a voxel whose component has no row (a slab's halo plane only)
TILE = (4, 4, 256)                     # voxels of the local pass's tile per memory axis (csrc/ta_components.h)


def _rows2d(a, width, dtype, what):
    a = np.asarray(a).astype(dtype)
    if a.size == 0:
        a = a.reshape(0, width)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError("%s must have shape (rows, %d)" % (what, width))
    return a


class LabelComponents(object):
    """The component table of one label image.

        label       int64 (R,)     the label of the component's voxels; rows ascend by (label, first)
        n           uint64 (R,)    its voxels
        first       int64 (R, 3)   its lexicographically smallest voxel, array axes
        bbox        int64 (R, 6)   min and max + 1 per array axis
        sum1        uint64 (R, 3)  the sum of its voxels' coordinates, array axes
        voxelsize   three floats
        ms          (milliseconds of the kernels that walk the volume, milliseconds after them) on the device; None for host tables
    """

    def __init__(self, label, n, first, bbox, sum1, voxelsize=(1.0, 1.0, 1.0), ms=None):
        self.label = np.asarray(label).astype(np.int64).reshape(-1)
        R = self.label.size
        self.n = np.asarray(n).astype(np.uint64).reshape(-1)
        self.first = _rows2d(first, 3, np.int64, "first")
        self.bbox = _rows2d(bbox, 6, np.int64, "bbox")
        self.sum1 = _rows2d(sum1, 3, np.uint64, "sum1")
        if self.n.shape != (R,) or self.first.shape[0] != R or self.bbox.shape[0] != R or self.sum1.shape[0] != R:
            raise ValueError("the columns of a component table have one entry per row")
        if R and (self.label.min() < 0 or self.label.max() > 0xFFFFFFFF):
            raise ValueError("labels must fit in uint32")
        self.voxelsize = voxelsize3(voxelsize)
        self.ms = ms

    def __len__(self):
        return int(self.label.size)

    # -- per label
    def per_label(self):
        """{label: number of components}."""
        labels, counts = np.unique(self.label, return_counts=True)
        return dict(zip(labels.tolist(), counts.tolist()))

    def fragmented(self, exclude=()):
        """{label: k} of the labels with k > 1 components, without those in `exclude`."""
        out = set(int(l) for l in exclude)
        return dict((l, k) for l, k in self.per_label().items() if k > 1 and l not in out)

    def rows_of(self, label):
        """Rows of the components of `label` (ascending; they are neighbours in the table)."""
        lo, hi = np.searchsorted(self.label, [int(label), int(label) + 1])
        return np.arange(lo, hi, dtype=np.int64)

    def largest(self):
        """bool (R,): the component with the most voxels of its label; of several such the one with the smaller `first`."""
        R = self.label.size
        out = np.zeros(R, dtype=bool)
        if R:
            # rows of a label ascend by first: among equal n the earliest row wins
            order = np.lexsort((np.arange(R), -self.n.astype(np.int64), self.label))
            head = np.ones(R, dtype=bool)
            head[1:] = self.label[order][1:] != self.label[order][:-1]
            out[order[head]] = True
        return out

    def centroid(self, real=True):
        """float64 (R, 3): sum1 / n, in voxel units or times the voxel size."""
        pos = self.sum1.astype(np.float64) / self.n.astype(np.float64)[:, None]
        return pos * np.asarray(self.voxelsize, dtype=np.float64) if real else pos

    # -- tables for relabel_components
    def split_map(self, next_label=None):
        """int64 (R,) new labels that make every component a label of its own: the largest component of a label keeps the label,
        every other row gets next_label, next_label + 1, ... in row order (default: the largest label + 1)."""
        new = self.label.copy()
        other = ~self.largest()
        if next_label is None:
            next_label = int(self.label.max()) + 1 if self.label.size else 0
        new[other] = int(next_label) + np.arange(int(other.sum()), dtype=np.int64)
        return new

    def erase_map(self, min_voxels, erase_value=0):
        """int64 (R,) new labels that erase the small fragments: rows that are not the largest of their label and have fewer
        than `min_voxels` voxels get `erase_value`, the rest keep their label."""
        new = self.label.copy()
        new[~self.largest() & (self.n < np.uint64(max(int(min_voxels), 0)))] = int(erase_value)
        return new

    # -- slabs
    @staticmethod
    def merge(parts, seams, voxelsize=None):
        """The tables of the slabs of one volume, cut along axis 0 and in order (each a LabelComponents in the volume's frame), as
        the whole volume's table.  seams[k] = (rows of the top owned plane of slab k, rows of the halo plane of slab k + 1): the
        row images of the same voxels in the two slabs; where both name a row, the two rows are one component."""
        parts, seams = list(parts), list(seams)
        if not parts:
            raise ValueError("nothing to merge")
        if len(seams) != len(parts) - 1:
            raise ValueError("%d slabs have %d seams, not %d" % (len(parts), len(parts) - 1, len(seams)))
        offset = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        total = int(offset[-1])
        parent = np.arange(total, dtype=np.int64)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for k, (below, above) in enumerate(seams):
            below, above = np.asarray(below).reshape(-1).astype(np.int64), np.asarray(above).reshape(-1).astype(np.int64)
            if below.shape != above.shape:
                raise ValueError("the two row images of seam %d differ in size" % k)
            both = (below != NONE) & (above != NONE)
            pairs = np.unique(np.stack([below[both] + offset[k], above[both] + offset[k + 1]], axis=1), axis=0)
            for a, b in pairs.tolist():
                a, b = find(a), find(b)
                if a != b:
                    parent[max(a, b)] = min(a, b)
        root = np.array([find(x) for x in range(total)], dtype=np.int64)
        label = np.concatenate([p.label for p in parts])
        n = np.concatenate([p.n for p in parts])
        first = np.concatenate([p.first for p in parts]).reshape(-1, 3)
        bbox = np.concatenate([p.bbox for p in parts]).reshape(-1, 6)
        sum1 = np.concatenate([p.sum1 for p in parts]).reshape(-1, 3)
        groups, inv = np.unique(root, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        G = groups.size
        if G and not np.array_equal(label[groups][inv], label):
            raise ValueError("a seam joins rows of different labels: these are not the slabs of one volume")
        gn = np.zeros(G, dtype=np.uint64)
        gs = np.zeros((G, 3), dtype=np.uint64)
        np.add.at(gn, inv, n)
        np.add.at(gs, inv, sum1)
        glo = np.full((G, 3), np.iinfo(np.int64).max, dtype=np.int64)
        ghi = np.full((G, 3), np.iinfo(np.int64).min, dtype=np.int64)
        np.minimum.at(glo, inv, bbox[:, :3])
        np.maximum.at(ghi, inv, bbox[:, 3:])
        # the lexicographic minimum of first: the first member of every group in (group, first) order
        order = np.lexsort((first[:, 2], first[:, 1], first[:, 0], inv))
        head = np.ones(total, dtype=bool)
        head[1:] = inv[order][1:] != inv[order][:-1]
        gfirst = first[order[head]]
        glabel = label[groups]
        rows = np.lexsort((gfirst[:, 2], gfirst[:, 1], gfirst[:, 0], glabel))
        return LabelComponents(glabel[rows], gn[rows], gfirst[rows], np.concatenate([glo, ghi], axis=1)[rows], gs[rows],
                               parts[0].voxelsize if voxelsize is None else voxelsize)


def context_components(ctx, voxelsize=(1.0, 1.0, 1.0)):
    """The component pass over the volume resident in the context `ctx`: a `LabelComponents`."""
    ctx.components_extract()
    label, n, first, bbox, sum1 = ctx.components_get()
    return LabelComponents(label, n, first, bbox, sum1, voxelsize, ms=ctx.components_timing())


def label_components(image, device=0):
    """The component table of a label image (a 2-D or 3-D integer array): a `LabelComponents`, with the image's own `voxelsize`
    attribute when it has one, else ones."""
    from .extraction import ResidentVolume
    voxelsize = getattr(image, "voxelsize", None)
    if voxelsize is None:
        voxelsize = (1.0, 1.0, 1.0)
    rv = ResidentVolume(np.asarray(image), device=device)
    try:
        return rv.components(voxelsize)
    finally:
        rv.close()
