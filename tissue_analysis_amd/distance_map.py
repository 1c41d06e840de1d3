"""Exact Euclidean distance maps of a label image: per voxel the distance to the nearest voxel of another label (the cell's own
wall) or of one chosen label (the background), and per label the smallest and the largest of them and where the largest sits
(include/tissue_scan_distance.h, csrc/kernels_distance.hip).

The largest distance of a cell's voxels to its own wall is the radius of its largest inscribed sphere, and the voxel where it is
reached (the pole) is a centre that stays inside a curved or fragmented cell.  The smallest distance of a cell's voxels to the
background is its depth below the tissue surface.  The table holds SQUARED distances (float64, exact for power-of-two voxel sizes);
the square roots are taken here.  No label is special in the table: the methods take an `exclude`."""
from __future__ import annotations

import numpy as np

from . import _capi
from ._tables import voxelsize3

OWN_WALL, FROM_LABEL = _capi.DIST_OWN_WALL, _capi.DIST_FROM_LABEL


class DistanceMap(object):
    """The distance table of one label image.

        labels      int64 (R,)      the label id of every row, ascending
        min2, max2  float64 (R,)    the smallest and the largest squared distance over the label's voxels; +inf for a label
                                    without voxels, and where no voxel has a site
        pole_voxel  int64 (R, 3)    the voxel where max2 is reached, array axes (the first in C order among several);
                                    (-1, -1, -1) for a label without voxels.  The constructor takes it as `pole`
        voxelsize   three floats    the spacing the distances were taken with
        mode        OWN_WALL or FROM_LABEL; site_label: the label of FROM_LABEL; edge: the image margin counted as a site
        ms          (milliseconds of the three passes, milliseconds of the table passes) on the device; None for host tables
    """

    def __init__(self, labels, min2, max2, pole, voxelsize=(1.0, 1.0, 1.0), mode=OWN_WALL, ms=None, site_label=None, edge=False,
                 image=None, profile=None):
        self.labels = np.asarray(labels).astype(np.int64).reshape(-1)
        R = self.labels.size
        self.min2 = np.asarray(min2, dtype=np.float64).reshape(-1)
        self.max2 = np.asarray(max2, dtype=np.float64).reshape(-1)
        p = np.asarray(pole).astype(np.int64)
        if p.size == 0:
            p = p.reshape(0, 3)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("pole must have shape (rows, 3)")
        self.pole_voxel = p
        if self.min2.shape != (R,) or self.max2.shape != (R,) or p.shape[0] != R:
            raise ValueError("the columns of a distance table have one entry per row")
        if R > 1 and not (np.diff(self.labels) > 0).all():
            raise ValueError("the labels of a distance table ascend")
        vs = voxelsize3(voxelsize)
        if mode not in (OWN_WALL, FROM_LABEL):
            raise ValueError("mode must be OWN_WALL (0) or FROM_LABEL (1), not %r" % (mode,))
        self.voxelsize = vs
        self.mode = mode
        self.site_label = site_label
        self.edge = bool(edge)
        self.ms = ms
        self._image = image                # callable: the float64 image of SQUARED distances, shaped like the label image
        self._profile = profile            # callable (edges, signal): the ShellProfile of the image over shells of distance

    def __len__(self):
        return int(self.labels.size)

    @property
    def present(self):
        """bool (R,): the label has voxels."""
        return self.pole_voxel[:, 0] >= 0

    def rows_of(self, labels):
        """int64 row of every label id, -1 for an id without a row."""
        want = np.asarray(labels, dtype=np.int64).reshape(-1)
        if self.labels.size == 0:
            return np.full(want.shape, -1, dtype=np.int64)
        pos = np.minimum(np.searchsorted(self.labels, want), self.labels.size - 1)
        return np.where(self.labels[pos] == want, pos, -1).astype(np.int64)

    def of_labels(self, labels, column="max2"):
        """float64 sqrt of `column` ('min2' or 'max2') for every label id in `labels`; +inf for an id without voxels."""
        if column not in ("min2", "max2"):
            raise ValueError("column must be 'min2' or 'max2', not %r" % (column,))
        rows = self.rows_of(labels)
        out = np.full(rows.shape, np.inf)
        out[rows >= 0] = np.sqrt(getattr(self, column)[rows[rows >= 0]])
        return out

    def _selection(self, labels, exclude):
        out = set(int(l) for l in exclude)
        if labels is None:
            ids = self.labels[self.present]
        else:
            ids = np.asarray(labels, dtype=np.int64).reshape(-1)
            rows = self.rows_of(ids)
            known = rows >= 0
            known[known] = self.present[rows[known]]
            ids = ids[known]
        return [int(l) for l in ids.tolist() if int(l) not in out]

    def max_distance(self, labels=None, exclude=()):
        """{label: the largest distance of its voxels} of the labels that have voxels, without those in `exclude`."""
        ids = self._selection(labels, exclude)
        return dict(zip(ids, self.of_labels(ids, "max2").tolist()))

    def min_distance(self, labels=None, exclude=()):
        """{label: the smallest distance of its voxels}, likewise."""
        ids = self._selection(labels, exclude)
        return dict(zip(ids, self.of_labels(ids, "min2").tolist()))

    def radius(self, labels=None, exclude=()):
        """{label: radius of the largest sphere centred on a voxel of the label that holds no site}: sqrt(max2).  With OWN_WALL that
        is the cell's inscribed radius."""
        return self.max_distance(labels, exclude)

    def pole(self, real=True, labels=None, exclude=()):
        """{label: xyz of the voxel where the largest distance is reached}, in real units (times the voxel size) or in voxels."""
        ids = self._selection(labels, exclude)
        pos = self.pole_voxel[self.rows_of(ids)].astype(np.float64).reshape(-1, 3)
        if real:
            pos = pos * np.asarray(self.voxelsize, dtype=np.float64)
        return dict(zip(ids, pos))

    def image(self):
        """float64 image of the distances (sqrt of the squared ones), with the shape and the axes of the label image.  Downloaded
        from the device: only for a table that came from one, and only while the context still holds it."""
        if self._image is None:
            raise ValueError("this distance table was built on the host: it has no image")
        return np.sqrt(self._image())

    def profile(self, edges, signal=None):
        """The `ShellProfile` of this map over the shells between `edges` (distances in real units, strictly ascending from >= 0,
        64 shells at most; the last may be inf): per label and shell the voxels and, with `signal` (uint8 / uint16, the image's
        shape), its sum, sum of squares and extremes.  One pass over labels, distances and signal on the device: only for a map
        that came from one, and only while the volume it was made from is still swept as it was (the distance pass runs again
        when a later map has taken its image's place)."""
        if self._profile is None:
            raise ValueError("this distance table was built on the host: it has no image to profile")
        return self._profile(edges, signal)


def resident_distance_map(resident, mode=OWN_WALL, site_label=None, voxelsize=(1.0, 1.0, 1.0), edge=False):
    """The distance pass over the volume resident in `resident` (a ResidentVolume), with the rows of its current extraction --
    swept first when the context holds none."""
    ctx = resident.ctx
    vs = voxelsize3(voxelsize)
    if mode not in (OWN_WALL, FROM_LABEL):
        raise ValueError("mode must be OWN_WALL (0) or FROM_LABEL (1), not %r" % (mode,))
    if mode == FROM_LABEL and site_label is None:
        raise ValueError("FROM_LABEL needs a site_label")
    site = 0 if site_label is None else int(site_label)
    if not 0 <= site <= 0xFFFFFFFF:
        raise ValueError("site_label must fit in uint32")
    flags = _capi.DIST_EDGE_IS_SITE if edge else 0
    x, _ = resident.over_extraction(lambda x: ctx.distance_extract(mode, site, vs, flags))
    min2, max2, pole = ctx.distance_get()
    labels = x.ids if x.sparse else np.arange(x.nrows, dtype=np.int64)
    run = [_next_run(resident)]

    def held():
        # the context keeps ONE image: the pass runs again when a later distance map has taken its place
        if resident.ctx is None or resident.last is not x:
            raise RuntimeError("the volume was swept again since this distance map was made: its image is gone")
        if resident._distance_run != run[0]:
            resident.ctx.distance_extract(mode, site, vs, flags)
            run[0] = _next_run(resident)

    def image():
        held()
        return resident.distance_image()

    def profile(edges, signal=None):
        from .shell_profile import ShellProfile
        held()
        e = np.asarray(edges, dtype=np.float64).reshape(-1)
        if signal is not None:
            resident.ctx.set_signal(np.asarray(signal))
        resident.ctx.profile_extract(np.square(e), signal is not None)
        n, s, q, mn, mx = resident.ctx.profile_get()
        return ShellProfile(labels, e, n, s, q, mn, mx, vs, present=pole[:, 0] >= 0, ms=resident.ctx.profile_timing())

    return DistanceMap(labels, min2, max2, pole, vs, mode, ms=ctx.distance_timing(), site_label=site_label if mode == FROM_LABEL else None,
                       edge=edge, image=image, profile=profile)


def _next_run(resident):
    resident._distance_run = getattr(resident, "_distance_run", 0) + 1
    return resident._distance_run


def distance_map(image, mode=OWN_WALL, site_label=None, edge=False, device=0):
    """(DistanceMap, float64 image of the distances) of a label image (a 2-D or 3-D integer array), with the image's own
    `voxelsize` attribute when it has one, else ones."""
    from .extraction import ResidentVolume
    voxelsize = getattr(image, "voxelsize", None)
    if voxelsize is None:
        voxelsize = (1.0, 1.0, 1.0)
    a = np.asarray(image)
    rv = ResidentVolume(a, device=device)
    try:
        dm = rv.distance_map(mode, site_label, voxelsize, edge)
        img = dm.image().reshape(a.shape)
        dm._image = dm._profile = None
        return dm, img
    finally:
        rv.close()
