"""How long, wide and thick every cell is: the extents of its voxels along three directions of its own -- by default its principal
axes --, the oriented box they span and how much of it the cell fills, from the exact minima and maxima of the extent pass
(include/tissue_scan_extents.h, csrc/kernels_extents.hip).  The pass projects voxel INDICES in memory-axis order onto a table of
weights; the directions, the voxel size and the axis permutation of an image that is not C-ordered become that table here, on the
host, and every float after the pass (float64) is the host's work too."""
from __future__ import annotations

import numpy as np

from ._tables import _ByLabel, voxelsize3

COLUMNS = ("lengths", "center", "box_volume", "fill", "aspect_ratio", "lo", "hi")


def _finite(a, what):
    a = np.asarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite" % what)
    return a


def complete_frame(direction):
    """float64 [3, 3]: the unit vector along `direction` and two unit vectors that complete it to a right-handed orthonormal frame."""
    d = _finite(direction, "the direction").reshape(-1)
    if d.size != 3 or not np.linalg.norm(d) > 0.0:
        raise ValueError("a direction is three numbers, not all zero")
    d = d / np.linalg.norm(d)
    e = np.zeros(3)
    e[int(np.argmin(np.abs(d)))] = 1.0                            # the array axis the direction leans on least
    b = np.cross(d, e)
    b /= np.linalg.norm(b)
    return np.stack([d, b, np.cross(d, b)])


def _frames(axes, rows):
    """float64 [rows, 3, 3], finite, from one direction (completed to a frame), one [3, 3] frame for every row, or [rows, 3, 3]."""
    a = _finite(axes, "the axes")
    if a.shape == (3,):
        a = complete_frame(a)
    if a.shape == (3, 3):
        a = np.broadcast_to(a, (int(rows), 3, 3))
    if a.shape != (int(rows), 3, 3):
        raise ValueError("axes must be [3], [3, 3] or [%d, 3, 3], not %s" % (rows, a.shape))
    return np.array(a)


def unit_frames(axes, rows):
    """float64 [rows, 3, 3] from one direction (completed to a frame), one [3, 3] frame for every row, or [rows, 3, 3]; every
    direction scaled to unit length.  ValueError for one that is not finite or zero."""
    a = _frames(axes, rows)
    norm = np.linalg.norm(a, axis=2, keepdims=True)
    if not (norm > 0.0).all():
        raise ValueError("a direction of the axes is zero")
    return a / norm


def principal_frames(extraction, voxelsize=(1.0, 1.0, 1.0)):
    """float64 [rows, 3, 3]: per row of `extraction` the principal axes (rows, by decreasing eigenvalue) of its PHYSICAL covariance
    D cov D, D = diag(voxelsize), cov the exact-integer covariance of the sweep; the identity for a row without voxels."""
    from .extraction import sym3_eig
    vs = np.asarray(voxelsize3(voxelsize), dtype=np.float64)
    R = extraction.nrows
    frames = np.broadcast_to(np.eye(3), (R, 3, 3)).copy()
    have = np.flatnonzero(extraction.count)
    if have.size:
        cov = extraction.covariances(extraction.labels_of(have)) * (vs[:, None] * vs[None, :])
        val, vec = sym3_eig(np.where(np.isfinite(cov), cov, 0.0))
        order = np.argsort(-val, axis=1, kind="stable")
        vec = np.take_along_axis(vec, order[:, None, :], axis=2)
        frames[have] = np.transpose(vec, (0, 2, 1))
    return frames


def extent_weights(axes, voxelsize=(1.0, 1.0, 1.0), perm=(0, 1, 2)):
    """The table of the pass, float64 [R, 3, 3]: weights[r, k, d] = axes[r, k, perm[d]] * voxelsize[perm[d]], direction k of row r
    per MEMORY axis d (`perm[d]` is the array axis of d)."""
    a = _finite(axes, "the axes")
    vs = _finite(voxelsize3(voxelsize), "the voxel size")
    perm = [int(p) for p in perm]
    if sorted(perm) != [0, 1, 2]:
        raise ValueError("perm must be a permutation of (0, 1, 2), not %r" % (perm,))
    return np.ascontiguousarray((a * vs)[:, :, perm])


class CellExtents(_ByLabel):
    """Oriented extents whose rows line up with an `Extraction`: rows 0..max_label, or one per id of `.ids` when the ids are sparse.

        axes  [R, 3, 3]   unit directions k = 0, 1, 2 of every row, in ARRAY-axis order, in physical space: the very numbers the
                          table of the pass was made from (`unit_frames` scales a caller's directions; they are not scaled again)
        lo, hi [R, 3]     the smallest and the largest projection sum_d axes[k, d] voxelsize[d] x_d of the row's voxel indices x;
                          NaN for a row without voxels
        count [R]         voxels per row (the extraction's)

    and what follows, float64, in the units of `voxelsize`:

        footprint()       sum_d |axes[k, d]| voxelsize[d]: the width of one voxel box along direction k
        lengths()         hi - lo + footprint: the exact extent of the union of the voxel boxes along every direction
        center()          the centre of the oriented box, array axes
        box_volume()      the volume of the oriented box; fill(): the cell's volume over it, at most 1
        aspect_ratio()    the longest of the three lengths over the shortest
        corners()         [R, 8, 3] the corners of the box
    """

    def __init__(self, extraction, lo, hi, axes, voxelsize=(1.0, 1.0, 1.0), count=None, ms=None):
        self.extraction = extraction
        self.ids = None if extraction is None else extraction.ids
        lo = np.array(lo, dtype=np.float64).reshape(-1, 3)
        hi = np.array(hi, dtype=np.float64).reshape(-1, 3)
        R = lo.shape[0]
        if hi.shape[0] != R:
            raise ValueError("lo and hi must have one row per label")
        self.axes = _frames(axes, R)
        self.voxelsize = voxelsize3(voxelsize)
        _finite(self.voxelsize, "the voxel size")
        if count is None:
            if extraction is None:
                raise ValueError("the voxel counts are needed: an extraction, or count")
            count = extraction.count
        self.count = np.asarray(count, dtype=np.uint64).reshape(-1)
        if self.count.size != R:
            raise ValueError("%d counts for %d rows" % (self.count.size, R))
        empty = ~((lo <= hi).all(axis=1))                          # the pass leaves +inf, -inf where a row has no voxel
        lo[empty] = np.nan
        hi[empty] = np.nan
        self.lo, self.hi = lo, hi
        self.ms = ms

    def __len__(self):
        return int(self.lo.shape[0])

    def _scale(self):
        return np.asarray(self.voxelsize, dtype=np.float64)

    def footprint(self):
        """float64 [R, 3]: the width of one voxel box along every direction."""
        return np.abs(self.axes) @ self._scale()

    def lengths(self):
        """float64 [R, 3]: the extent of the union of the row's voxel boxes along every direction; NaN without voxels."""
        return self.hi - self.lo + self.footprint()

    def _solve(self, coords):
        """Points [R, ..., 3] given by their coordinates along the three directions of every row -> array axes; NaN where a
        row's directions do not span the space."""
        out = np.full(coords.shape, np.nan, dtype=np.float64)
        ok = np.abs(np.linalg.det(self.axes)) > 1e-12
        if ok.any():
            rhs = coords[ok].reshape(int(ok.sum()), -1, 3)
            out[ok] = np.transpose(np.linalg.solve(self.axes[ok], np.transpose(rhs, (0, 2, 1))), (0, 2, 1)).reshape(coords[ok].shape)
        return out

    def center(self, real=True):
        """float64 [R, 3]: the centre of the oriented box in array axes, in the units of the voxel size (real) or in voxels."""
        c = self._solve(0.5 * (self.lo + self.hi))
        return c if real else c / self._scale()

    def corners(self, real=True):
        """float64 [R, 8, 3]: the corners of the oriented box in array axes; corner 4 a + 2 b + c takes the low (0) or high (1)
        face along directions 0, 1, 2."""
        half = 0.5 * self.footprint()
        ends = np.stack([self.lo - half, self.hi + half], axis=1)          # [R, 2, 3]
        pick = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
        coords = np.stack([ends[:, pick[:, k], k] for k in range(3)], axis=2)
        c = self._solve(coords)
        return c if real else c / self._scale()

    def volume(self):
        """float64 [R]: voxels times the volume of one."""
        return self.count.astype(np.float64) * float(np.prod(self._scale()))

    def box_volume(self):
        """float64 [R]: the volume of the oriented box (the product of the lengths for orthogonal directions)."""
        det = np.abs(np.linalg.det(self.axes))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.prod(self.lengths(), axis=1) / np.where(det > 1e-12, det, np.nan)

    def fill(self):
        """float64 [R]: the share of its oriented box the cell fills, at most 1 (a cuboid along its directions: 1)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.minimum(self.volume() / self.box_volume(), 1.0)

    def aspect_ratio(self):
        """float64 [R]: the longest length over the shortest."""
        l = self.lengths()
        return l.max(axis=1) / l.min(axis=1)

    def of_labels(self, labels, column="lengths"):
        """`column` of every label id in `labels`, NaN for an id without a row."""
        if column not in COLUMNS:
            raise ValueError("column must be one of %s, not %r" % ("|".join(COLUMNS), column))
        col = getattr(self, column)
        return self._pick(col() if callable(col) else col, labels, np.nan)


def resident_cell_extents(resident, axes=None, voxelsize=(1.0, 1.0, 1.0)):
    """The extent pass over the volume resident in `resident` (a ResidentVolume), with the rows of its current extraction -- swept
    first when the context holds none that fits.  axes: None = every row's principal axes (`principal_frames`), one direction, one
    [3, 3] frame, [rows, 3, 3], or {label: [3, 3]} (the other rows take the identity), in array axes and physical space."""
    ctx = resident.ctx
    frames = []

    def enqueue(x):
        if axes is None:
            f = principal_frames(x, voxelsize)
        elif isinstance(axes, dict):
            f = np.broadcast_to(np.eye(3), (x.nrows, 3, 3)).copy()
            labels = list(axes)
            if labels:
                f[x.rows_of(labels)] = np.stack([unit_frames(axes[l], 1)[0] for l in labels])
        else:
            f = unit_frames(axes, x.nrows)
        frames[:] = [f]
        ctx.extents_extract(extent_weights(f, voxelsize, ctx.memory_axes()))

    x, _ = resident.over_extraction(enqueue)
    lo, hi = ctx.extents_rows()
    return CellExtents(x, lo, hi, frames[0], voxelsize, ms=ctx.extents_timing())
