"""The overlap table between two label volumes of one grid -- frame t against frame t+1 resampled onto it, or two segmentations
of one image -- from the exact voxel counts of the overlap pass (include/tissue_scan_overlap.h, csrc/kernels_overlap.hip), and
what follows from it on the host: the sizes of the labels of each side, the Jaccard index, best matches and cell lineage."""
from __future__ import annotations

import numpy as np

from . import _capi


def _member(values, chosen):
    chosen = np.asarray(list(chosen), dtype=np.int64).reshape(-1)
    return np.isin(values, chosen) if chosen.size else np.zeros(values.shape, dtype=bool)


class LabelOverlap(object):
    """Rows (a, b, n): n voxels carry label a in volume A and label b in volume B; sorted by (a, b), each pair once, n > 0.

        a, b            int64, the label ids as stored in the two volumes (no label is special: 0 and a background are rows)
        n               uint64
        size_a, size_b  (ids int64 ascending, voxels uint64) of every label of one side: the table's margins, exact
        ms              milliseconds of the pass kernel on the device (None for a table built on the host)
        outside         voxels of A where a B resampled from another grid had no voxel and reads as its fill label (None otherwise)
    """

    def __init__(self, a, b, n, ms=None):
        self.a = np.asarray(a).astype(np.int64)
        self.b = np.asarray(b).astype(np.int64)
        self.n = np.asarray(n).astype(np.uint64)
        if not (self.a.shape == self.b.shape == self.n.shape and self.a.ndim == 1):
            raise ValueError("a, b and n must be 1-D arrays of one length")
        self.ms = ms
        self.outside = None
        self._margins = {}

    def __len__(self):
        return int(self.a.size)

    def _keys(self):
        return (self.a.astype(np.uint64) << np.uint64(32)) | self.b.astype(np.uint64)

    def between(self, a, b):
        """Voxels with label `a` in A and `b` in B (0 when the two never meet)."""
        if not (0 <= int(a) <= 0xFFFFFFFF and 0 <= int(b) <= 0xFFFFFFFF) or not len(self):
            return 0
        keys = self._keys()
        want = np.uint64((int(a) << 32) | int(b))
        i = int(np.searchsorted(keys, want))
        return int(self.n[i]) if i < keys.size and keys[i] == want else 0

    def _margin(self, side):
        if side not in self._margins:
            ids, inv = np.unique(self.a if side == "a" else self.b, return_inverse=True)
            tot = np.zeros(ids.size, dtype=np.uint64)
            np.add.at(tot, inv, self.n)
            self._margins[side] = (ids, tot, inv)
        return self._margins[side]

    @property
    def size_a(self):
        ids, tot, _ = self._margin("a")
        return ids, tot

    @property
    def size_b(self):
        ids, tot, _ = self._margin("b")
        return ids, tot

    def row_sizes(self):
        """(|a|, |b|) of every row: the whole size of the row's label in A and in B (uint64)."""
        _, ta, ia = self._margin("a")
        _, tb, ib = self._margin("b")
        return ta[ia], tb[ib]

    def jaccard(self):
        """n / (|a| + |b| - n) of every row, float64."""
        sa, sb = self.row_sizes()
        return self.n.astype(np.float64) / (sa + sb - self.n).astype(np.float64)

    def best_match(self, side="b", exclude=()):
        """For every label of `side` ('a' or 'b') that meets a partner outside `exclude`: the partner of the other side with the
        largest n, ties to the smallest partner id.  Returns (labels int64 ascending, partners int64, n uint64)."""
        if side not in ("a", "b"):
            raise ValueError("side must be 'a' or 'b'")
        own, other = (self.a, self.b) if side == "a" else (self.b, self.a)
        keep = ~_member(other, exclude)
        own, other, n = own[keep], other[keep], self.n[keep]
        if own.size == 0:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint64)
        # per label: largest n first, then the smallest partner (lexsort: last key is the primary one)
        order = np.lexsort((other, np.iinfo(np.uint64).max - n, own))
        own, other, n = own[order], other[order], n[order]
        first = np.ones(own.size, dtype=bool)
        first[1:] = own[1:] != own[:-1]
        return own[first], other[first], n[first]

    def lineage(self, min_fraction=0.5, exclude=(0,)):
        """{mother: [daughters ascending]}: for every label b of B not in `exclude`, its mother is the label of A (not in
        `exclude`) that holds the most of its voxels, accepted when n(a, b) >= min_fraction * |b| (float64, |b| the whole
        size of b).  The mapping form lineage files use."""
        labels, mothers, n = self.best_match("b", exclude)
        ids_b, size_b = self.size_b
        whole = size_b[np.searchsorted(ids_b, labels)]
        ok = ~_member(labels, exclude) & (n.astype(np.float64) >= float(min_fraction) * whole.astype(np.float64))
        labels, mothers = labels[ok], mothers[ok]
        order = np.lexsort((labels, mothers))
        labels, mothers = labels[order], mothers[order]
        if mothers.size == 0:
            return {}
        starts = np.flatnonzero(np.concatenate(([True], mothers[1:] != mothers[:-1])))
        groups = np.split(labels, starts[1:])
        return dict((int(m), g.tolist()) for m, g in zip(mothers[starts].tolist(), groups))


def _cuda_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda") and bool(x.is_cuda)


def resident_overlap(resident, other, matrix=None, fill=0):
    """The overlap pass over the volume resident in `resident` (a ResidentVolume) and `other`: an integer array of the same
    shape (a 2-D one for a 2-D label image), or a CUDA tensor of it (int16 / int32 storage holding uint16 / uint32 labels,
    contiguous, on the volume's GPU).  With `matrix` (a 3 x 4 index matrix) `other` has any shape and is resampled onto the
    grid of the volume by nearest neighbour first, on the device, where the pass then reads it; the table's `.outside` is the
    number of voxels that fell outside `other` and count as its label `fill`."""
    from .extraction import _as_label_volume
    ctx = resident.ctx
    outside = None
    if matrix is not None:
        from .resample import resident_resample
        if not _cuda_tensor(other):
            other, _ = _as_label_volume(other)          # (uint16 / uint32: what the overlap pass takes)
        elif other.element_size() not in (2, 4):
            raise TypeError("label tensors must hold 2- or 4-byte integers")
        outside = resident_resample(resident, other, matrix, 0, fill).outside
        ctx.resample_as_overlap()
    elif _cuda_tensor(other):
        shape = tuple(int(d) for d in other.shape)
        if len(shape) == 2:
            shape = shape + (1,)
        if shape != tuple(resident.host.shape) or not resident.host.flags.c_contiguous or not other.is_contiguous():
            raise ValueError("a device-resident second volume must be C-contiguous and shaped like the (C-contiguous) label volume")
        if other.element_size() not in (2, 4):
            raise TypeError("label tensors must hold 2- or 4-byte integers")
        ctx.set_overlap_device(other.data_ptr(), other.element_size(), keep=other)
    else:
        b, _ = _as_label_volume(other)
        ctx.set_overlap(b)
    ctx.overlap_extract()
    a, b, n = ctx.overlap_get()
    ov = LabelOverlap(a, b, n, ms=ctx.overlap_timing())
    ov.outside = outside
    return ov


def label_overlap(image_a, image_b, device=0, matrix=None, fill=0):
    """The overlap table of two label images (2-D or 3-D integer arrays): a `LabelOverlap`.  They share one shape, or `matrix` (a
    3 x 4 index matrix, `resample.index_matrix`) takes a voxel index of image_a to the continuous index in image_b."""
    from .extraction import ResidentVolume
    rv = ResidentVolume(image_a, device=device)
    try:
        return rv.overlap(image_b, matrix, fill)
    finally:
        rv.close()


def lineage_from_images(image_t0, image_t1, min_fraction=0.5, background=1, device=0, transform=None, voxelsize_t0=None,
                        voxelsize_t1=None):
    """{mother in image_t0: [daughters in image_t1]} of two frames; 0 and `background` are nobody's mother or daughter.  The
    frames share one grid, or `transform` (a homogeneous matrix from physical coordinates of frame t0 to those of frame t1; with
    only the voxel sizes given, the identity) registers them: frame t1 is then resampled onto the grid of frame t0 on the
    device, and its voxels that fall outside count as the background."""
    exclude = (0,) if background is None else (0, int(background))
    matrix = None
    if transform is not None or voxelsize_t0 is not None or voxelsize_t1 is not None:
        from .resample import index_matrix
        matrix = index_matrix(transform, voxelsize_t0, voxelsize_t1)
    ov = label_overlap(image_t0, image_t1, device=device, matrix=matrix, fill=0 if background is None else int(background))
    return ov.lineage(min_fraction=min_fraction, exclude=exclude)
