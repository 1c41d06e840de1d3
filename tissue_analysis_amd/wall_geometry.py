"""Geometry of the walls of a label image (the faces shared by two labels) from the exact integer rows of the wall-geometry
pass (include/tissue_scan_wallgeo.h, csrc/kernels_wallgeo.hip), and what follows from them on the host: a wall area that a
tilted wall's voxel staircase does not inflate, a wall normal, a wall centroid and a plane fit.

A face is a pair of 6-adjacent voxels of different labels lo < hi; its position c is the sum of the two voxel centres (doubled
voxel-centre coordinates, array axes: odd along the face's axis, even along the others; c / 2 is the frame of
`center_of_mass(real=False)`).  A row holds, per wall: fwd[d] / rev[d], the faces of axis d with lo / hi on the low-coordinate
side; sum1 = sum of c; sum2 = sum of c_x c_y for xx, xy, xz, yy, yz, zz.  fwd + rev is the pair's face count of the sweep.  No
label is special in the table: background walls have rows, and `as_dict` takes an `exclude`."""
from __future__ import annotations

import numpy as np

from ._tables import voxelsize3

PAIR_ORDER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _keys(lo, hi):
    return (np.asarray(lo).astype(np.uint64) << np.uint64(32)) | np.asarray(hi).astype(np.uint64)


class WallGeometry(object):
    """The wall-geometry rows of one label image, sorted by (pair_lo, pair_hi).

        pair_lo, pair_hi  int64 (P,), lo < hi: the label ids as stored in the image
        fwd, rev          uint64 (P, 3) faces per axis with lo (fwd) or hi (rev) on the low-coordinate side
        sum1              uint64 (P, 3) sum of the doubled face centres, array axes
        sum2              uint64 (P, 6) sum of their products xx, xy, xz, yy, yz, zz
        voxelsize         three floats
        ms                milliseconds of the pass kernel on the device; None for host tables
    """

    def __init__(self, pair_lo, pair_hi, fwd, rev, sum1, sum2, voxelsize=(1.0, 1.0, 1.0), ms=None):
        self.pair_lo = np.asarray(pair_lo).astype(np.int64).reshape(-1)
        self.pair_hi = np.asarray(pair_hi).astype(np.int64).reshape(-1)
        P = self.pair_lo.size
        if self.pair_hi.size != P:
            raise ValueError("pair_lo and pair_hi must have the same length")
        if P and not (self.pair_lo < self.pair_hi).all():
            raise ValueError("every row needs pair_lo < pair_hi")
        if P and (self.pair_lo.min() < 0 or self.pair_hi.max() > 0xFFFFFFFF):
            raise ValueError("labels must fit in uint32")
        self.fwd = np.asarray(fwd).astype(np.uint64).reshape(-1, 3)
        self.rev = np.asarray(rev).astype(np.uint64).reshape(-1, 3)
        self.sum1 = np.asarray(sum1).astype(np.uint64).reshape(-1, 3)
        self.sum2 = np.asarray(sum2).astype(np.uint64).reshape(-1, 6)
        for name in ("fwd", "rev", "sum1", "sum2"):
            if getattr(self, name).shape[0] != P:
                raise ValueError("%s must have one row per pair" % name)
        self.voxelsize = voxelsize3(voxelsize)
        self.ms = ms

    def __len__(self):
        return int(self.pair_lo.size)

    # -- counts
    def faces(self):
        """uint64 (P, 3): faces per axis, fwd + rev (the `faces` of the sweep's pair list)."""
        return self.fwd + self.rev

    def n(self):
        """float64 (P,): faces of the wall."""
        return self.faces().sum(axis=1).astype(np.float64)

    def _face_surface(self):
        vx, vy, vz = self.voxelsize
        return np.array([vy * vz, vz * vx, vx * vy], dtype=np.float64)

    # -- first order
    def centroid(self, real=True):
        """float64 (P, 3): the mean face centre, sum1 / (2 n), in voxel units or times the voxel size."""
        c = self.sum1.astype(np.float64) / (2.0 * self.n())[:, None]
        return c * np.asarray(self.voxelsize, dtype=np.float64) if real else c

    def vector_area(self, real=True):
        """float64 (P, 3): the sum of the faces' oriented areas, (fwd - rev) times the face areas (vy vz, vz vx, vx vy); it
        points from lo to hi.  Zero for a closed wall (a cell wholly enclosed by its neighbour)."""
        v = self.fwd.astype(np.int64) - self.rev.astype(np.int64)
        return v * self._face_surface() if real else v.astype(np.float64)

    def projected_area(self, real=True):
        """float64 (P,): the norm of the vector area: the area of the wall projected along its mean normal.  A flat wall tilted
        against the axes has this area, whereas its voxel faces add up to as much as sqrt(3) times it."""
        return np.linalg.norm(self.vector_area(real), axis=1)

    def voxel_area(self, real=True):
        """float64 (P,): the area of the wall's voxel faces, F0 vy vz + F1 vz vx + F2 vx vy (what `wall_areas` gives)."""
        f = self.faces()
        if not real:
            return (f[:, 0] + f[:, 1] + f[:, 2]).astype(np.float64)
        s = self._face_surface()
        return f[:, 0] * s[0] + f[:, 1] * s[1] + f[:, 2] * s[2]

    def normal(self):
        """float64 (P, 3): the unit vector along the vector area in real units, from lo to hi; NaN where the vector area is zero."""
        v = self.vector_area(True)
        norm = np.linalg.norm(v, axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(norm[:, None] > 0, v / norm[:, None], np.nan)

    # -- second order
    def covariance(self, real=True):
        """float64 (P, 3, 3): the covariance of the face centres, sum2 / (4 n) - mean mean^T, in voxel units or scaled by the voxel
        size.  The sums are first moved to an integer origin next to the wall's mean and the n^2-scaled difference
        n S2 - S1 S1^T is taken in exact integers (in float64 only where it would not fit 63 bits)."""
        P = len(self)
        cov = np.zeros((P, 3, 3), dtype=np.float64)
        if not P:
            return cov
        n = self.faces().sum(axis=1)                                      # uint64
        o = self.sum1 // n[:, None]                                       # an origin within one unit of the doubled mean
        s1 = (self.sum1 - n[:, None] * o).astype(np.int64)                # 0 <= s1 < n
        nf = n.astype(np.float64)
        ni = n.astype(np.int64)
        for k, (d, e) in enumerate(PAIR_ORDER):
            # modulo 2^64; the true value is small, so the int64 view is exact
            s2 = (self.sum2[:, k] - o[:, d] * self.sum1[:, e] - o[:, e] * self.sum1[:, d] + n * o[:, d] * o[:, e]).view(np.int64)
            fits = (nf * np.abs(s2.astype(np.float64)) < 2.0 ** 62) & (nf * nf < 2.0 ** 62)
            exact = (ni * np.where(fits, s2, 0) - s1[:, d] * s1[:, e]).astype(np.float64) / (nf * nf)
            loose = s2.astype(np.float64) / nf - (s1[:, d].astype(np.float64) / nf) * (s1[:, e].astype(np.float64) / nf)
            c = np.where(fits, exact, loose) / 4.0
            cov[:, d, e] = c
            cov[:, e, d] = c
        if real:
            vs = np.asarray(self.voxelsize, dtype=np.float64)
            cov = cov * (vs[:, None] * vs[None, :])
        return cov

    def plane_fit(self, real=True):
        """The least-squares plane through the face centres of every wall, by one batched `eigh` of the covariances:
        (normal float64 (P, 3): the unit direction of least variance, signed to agree with the vector area; thickness float64
        (P,): the rms distance of the faces from the plane, sqrt(lambda_min); extents float64 (P, 2): the rms extents along the
        two in-plane principal directions, smaller first)."""
        cov = self.covariance(real)
        if not cov.shape[0]:
            return np.zeros((0, 3)), np.zeros(0), np.zeros((0, 2))
        val, vec = np.linalg.eigh(cov)                                     # ascending
        normal = vec[:, :, 0].copy()
        flip = np.einsum("ij,ij->i", normal, self.vector_area(real)) < 0
        normal[flip] *= -1.0
        root = np.sqrt(np.maximum(val, 0.0))
        return normal, root[:, 0], root[:, 1:]

    # -- lookups
    def wall_rows(self, lo, hi):
        """Rows of the walls (lo[i], hi[i]) (in either order), -1 where the table has no such wall."""
        a, b = np.asarray(lo, dtype=np.int64).reshape(-1), np.asarray(hi, dtype=np.int64).reshape(-1)
        want = _keys(np.minimum(a, b), np.maximum(a, b))
        have = _keys(self.pair_lo, self.pair_hi)
        if not have.size:
            return np.full(want.shape, -1, dtype=np.int64)
        at = np.minimum(np.searchsorted(have, want), have.size - 1)
        return np.where(have[at] == want, at, -1)

    def as_dict(self, column, exclude=()):
        """{(lo, hi): value} of the walls none of whose labels is in `exclude`.  column: the name of a method without arguments
        ('centroid', 'normal', 'projected_area', 'voxel_area', 'vector_area', 'n', 'faces', 'covariance') or of an array
        ('fwd', 'rev', 'sum1', 'sum2')."""
        values = getattr(self, column)
        if callable(values):
            values = values()
        chosen = np.asarray(list(exclude), dtype=np.int64).reshape(-1)
        keep = ~(np.isin(self.pair_lo, chosen) | np.isin(self.pair_hi, chosen)) if chosen.size else np.ones(len(self), dtype=bool)
        values = np.asarray(values)[keep]
        keys = zip(self.pair_lo[keep].tolist(), self.pair_hi[keep].tolist())
        return dict(zip(keys, values.tolist() if values.ndim == 1 else list(values)))

    # -- slabs
    @staticmethod
    def merge(parts, voxelsize=None):
        """The rows of the slabs of one volume (each a WallGeometry, positions in the volume's frame) as one: every field is added
        over equal pairs."""
        parts = list(parts)
        if not parts:
            raise ValueError("nothing to merge")
        keys = np.concatenate([_keys(p.pair_lo, p.pair_hi) for p in parts])
        uniq, inv = np.unique(keys, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        out = []
        for name, width in (("fwd", 3), ("rev", 3), ("sum1", 3), ("sum2", 6)):
            t = np.zeros((uniq.size, width), dtype=np.uint64)
            np.add.at(t, inv, np.concatenate([getattr(p, name) for p in parts]).reshape(-1, width))
            out.append(t)
        return WallGeometry((uniq >> np.uint64(32)).astype(np.int64), (uniq & np.uint64(0xFFFFFFFF)).astype(np.int64),
                            out[0], out[1], out[2], out[3], parts[0].voxelsize if voxelsize is None else voxelsize)


def resident_wall_geometry(resident, voxelsize=(1.0, 1.0, 1.0)):
    """The wall-geometry pass over the volume resident in `resident` (a ResidentVolume), with the pairs of its current
    extraction -- swept first when the context holds none that fits (the pass needs the pair list)."""
    ctx = resident.ctx
    x, _ = resident.over_extraction(lambda x: ctx.wallgeo_extract())
    fwd, rev, sum1, sum2 = ctx.wallgeo_get()
    return WallGeometry(x.lo, x.hi, fwd, rev, sum1, sum2, voxelsize, ms=ctx.wallgeo_timing())


def wall_geometry(image, voxelsize=None, device=0):
    """The wall-geometry rows of a label image (a 2-D or 3-D integer array): a `WallGeometry`.  voxelsize: None = the image's
    own `voxelsize` attribute when it has one, else ones."""
    from .extraction import ResidentVolume
    if voxelsize is None:
        voxelsize = getattr(image, "voxelsize", None)
    if voxelsize is None:
        voxelsize = (1.0, 1.0, 1.0)
    rv = ResidentVolume(np.asarray(image), device=device)
    try:
        return rv.wall_geometry(voxelsize)
    finally:
        rv.close()
