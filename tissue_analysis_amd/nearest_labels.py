"""Exact nearest-label maps of a label image: for every voxel the label of the nearest voxel that is not empty (the smallest label
among several that are equally near) and the distance to it, and the image with its empty voxels given to the label they lie
nearest to (include/tissue_scan_nearest.h, csrc/kernels_nearest.hip).

This closes the holes that `remove_small_fragments`, `remove_labels_from_image` and `remove_stack_margin_labels_from_image` write
into an image, and with a limit on the distance it grows labels into their surroundings (skimage's expand_labels).  It is
scipy.ndimage.distance_transform_edt(..., return_indices=True) followed by a gather, with a stated rule for ties."""
from __future__ import annotations

import numpy as np

from . import _capi
from ._tables import voxelsize3

NONE = _capi.NEAREST_NONE


class NearestLabels(object):
    """The nearest-label map of one label image, in the ids of the image.

        labels        int64 (R,)    the label id of every row, ascending
        gained_voxels int64 (R,)    the empty voxels every label would gain (the constructor takes it as `gained`)
        filled        int           empty voxels within `max_distance` of a site: what `apply()` fills
        remaining     int           empty voxels that stay empty
        empty         the label of the empty voxels; not_from: the label whose voxels are neither sites nor filled, or None
        max_distance  the limit of the fill in the units of `voxelsize` (inclusive), None = no limit
        voxelsize     three floats  the spacing the distances were taken with
        ms            (milliseconds of the three passes, milliseconds of the counting pass) on the device; None for host tables
    """

    def __init__(self, labels, gained, filled, remaining, empty=0, not_from=None, max_distance=None, voxelsize=(1.0, 1.0, 1.0), ms=None,
                 source=None, images=None, apply=None):
        self.labels = np.asarray(labels).astype(np.int64).reshape(-1)
        self.gained_voxels = np.asarray(gained).astype(np.int64).reshape(-1)
        if self.gained_voxels.shape != self.labels.shape:
            raise ValueError("gained has one entry per row")
        if self.labels.size > 1 and not (np.diff(self.labels) > 0).all():
            raise ValueError("the labels of a nearest-label table ascend")
        vs = voxelsize3(voxelsize)
        self.filled, self.remaining = int(filled), int(remaining)
        if int(self.gained_voxels.sum()) != self.filled:
            raise ValueError("the gained voxels of the labels sum to the filled voxels")
        self.empty = int(empty)
        self.not_from = None if not_from is None else int(not_from)
        self.max_distance = None if max_distance is None else float(max_distance)
        self.voxelsize = vs
        self.ms = ms
        self._source = source              # callable: the label image the map was made from
        self._images = images              # callable: (uint32 image of N, float64 image of D2), shaped like the label image
        self._apply = apply                # callable: writes the map into the image it was made from

    def __len__(self):
        return int(self.labels.size)

    @property
    def max_d2(self):
        """The limit as the device compares it: max_distance squared, +inf without a limit."""
        return max_d2_of(self.max_distance)

    def gained(self):
        """{label: voxels} of the labels that gain at least one voxel."""
        rows = np.flatnonzero(self.gained_voxels)
        return dict(zip(self.labels[rows].tolist(), self.gained_voxels[rows].tolist()))

    def _need(self, what):
        if what is None:
            raise ValueError("this nearest-label table was built on the host: it has no images")
        return what()

    def nearest(self):
        """uint32 image of N: for every voxel the smallest label among its nearest sites (a site's own label); NONE where the
        image has no site.  Downloaded from the device: only for a table that came from one, and only while the context holds it."""
        return self._need(self._images)[0]

    def distance(self):
        """float64 image of the distance of every voxel to its nearest site (0 at a site, inf without one)."""
        return np.sqrt(self._need(self._images)[1])

    def filled_mask(self):
        """bool image: the voxel is empty and within the limit of a site."""
        d2 = self._need(self._images)[1]
        return (self._need(self._source) == self.empty) & np.isfinite(d2) & (d2 <= self.max_d2)

    def image(self):
        """The label image that `apply()` would leave, with the layout and the dtype of the label image."""
        src = self._need(self._source)
        out = src.copy(order="K")
        mask = self.filled_mask()
        out[mask] = self.nearest()[mask].astype(src.dtype)
        return out

    def apply(self):
        """Write the map into the image it was made from (on the device, and the host copy of the resident volume); returns
        what the sweep of the new image returns."""
        if self._apply is None:
            raise ValueError("this nearest-label table was built on the host: there is nothing to apply it to")
        return self._apply()


def max_d2_of(max_distance):
    if max_distance is None:
        return float("inf")
    d = float(max_distance)
    if not d >= 0.0:
        raise ValueError("max_distance must be >= 0, not %r" % (max_distance,))
    return d * d


def resident_nearest_labels(resident, empty=0, not_from=None, voxelsize=(1.0, 1.0, 1.0), max_distance=None):
    """The nearest-label pass over the volume resident in `resident` (a ResidentVolume), with the rows of its current extraction --
    swept first when the context holds none."""
    ctx = resident.ctx
    vs = voxelsize3(voxelsize)
    for name, v in (("empty", empty), ("not_from", not_from)):
        if v is not None and not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("%s must fit in uint32" % name)
    args = (int(empty), None if not_from is None else int(not_from), vs, max_d2_of(max_distance))
    x, _ = resident.over_extraction(lambda x: ctx.nearest_extract(*args))
    gained, filled, remaining = ctx.nearest_get()
    labels = x.ids if x.sparse else np.arange(x.nrows, dtype=np.int64)

    def held():
        if resident.ctx is None or resident.last is not x:
            raise RuntimeError("the volume was swept again since this nearest-label map was made: it is gone")
        try:
            resident.ctx.nearest_debug()
        except _capi.TissueScanError:                      # (an edit through another door: the same pass again would not be the same map)
            raise RuntimeError("the volume changed since this nearest-label map was made: it is gone")
        if resident._nearest_args != args:                 # the context keeps ONE map: the pass runs again when a later one took its place
            resident.ctx.nearest_extract(*args)
            resident._nearest_args = args

    def images():
        held()
        return resident.nearest_images()

    def apply():
        held()
        return resident.apply_nearest()

    resident._nearest_args = args
    return NearestLabels(labels, gained, filled, remaining, empty, not_from, max_distance, vs, ms=ctx.nearest_timing(),
                         source=lambda: resident.host, images=images, apply=apply)
