"""Drop-in for the per-label feature extractors of ``vplants.tissue_analysis.spatial_image_analysis``
(reference file cited as SIA:<line>), with every voxel scan done by ONE fused HIP sweep on an
MI355X instead of per-label scipy.ndimage loops.

Kept verbatim from the reference: module constants ``NPLIST, LIST, DICT`` (SIA:204), the factory
``SpatialImageAnalysis(image, *args, **kwd)`` (SIA:1663), the class names, method names, argument
names/defaults and return-shape rules (dict under DICT, bare value for one label, ``(i, j)`` keys
with i < j for areas) and the cache attributes other code pokes (``_bbox``, ``_neighbors``,
``_center_of_mass``, ``_labels``, ``_voxelsize``, ``_background``, ``_ignoredlabels``).

Documented divergences (DESIGN.md "Reference quirks"):
* label lists come back in ascending order (the reference returns Python-2 ``set`` order);
* ``volume`` uses the true label ids (the reference casts them with ``np.int16``, SIA:1231);
* 2D images are handled by this same class as (X, Y, 1) volumes (the reference's
  ``SpatialImageAnalysis2D`` does not exist, SIA:1677);
* the image is uploaded and swept at construction; mutating ``self.image`` afterwards needs
  ``refresh()``;
* ``return_type=NPLIST`` is the ARRAY mode: where the reference hands back "the values as they are" (SIA:309-334) the
  values here are numpy arrays over the requested labels, with no per-label Python objects -- ``volume`` [n],
  ``center_of_mass`` [n, 3], ``boundingbox`` [n, 6] (starts, then stops), ``neighbors_number`` [n], ``surface_area`` [n],
  ``inertia_axis`` ([n, 3, 3], [n, 3]), ``wall_areas()`` (pairs [m, 2], areas [m]); ``neighbors()`` is a read-only mapping
  over the adjacency's CSR arrays (`.indptr`, `.indices`) whose lists are made when a label is looked up.  (The reference returns dicts from
  ``center_of_mass`` / ``neighbors_number`` / ``wall_areas`` whatever the return type; DICT and LIST do exactly that.)
There is no CPU fallback: constructing an analysis without the built HIP library or without a GPU
raises.
"""
from __future__ import annotations

import copy
import warnings
from os.path import split

import numpy as np

from . import _capi
from .extraction import Extraction, extract_volume
from .geometry import _find_wall_median_voxel, find_wall_median_voxel, geometric_median   # module-level in SIA too (SIA:1499-1635)
from .signal_stats import STATISTICS, WALL_STATISTICS
from .spatial_image import SpatialImage

NPLIST, LIST, DICT = range(3)  # SIA:204

_INT = (int, np.integer)


# ----------------------------------------------------------------------------- module helpers
def dilation(slices):
    """Bounding box grown by one voxel, clamped at zero (SIA:35-37)."""
    return [slice(max(0, s.start - 1), s.stop + 1) for s in slices]


def dilation_by(slices, amount=2):
    """SIA:40-42."""
    return [slice(max(0, s.start - amount), s.stop + amount) for s in slices]


def real_indices(slices, resolutions):
    """Voxel bounding box -> real-world (start, stop) pairs (SIA:63-71)."""
    return [(s.start * r, s.stop * r) for s, r in zip(slices, resolutions)]


def wall(mask_img, label_id, device=0):
    """Labels of the voxels of `mask_img` in the 6-connected one-voxel shell around cell `label_id`, in C index order -- what
    `mask_img[binary_dilation(mask_img == label_id) - (mask_img == label_id)]` gives in the reference (SIA:45-52; nothing
    outside the array counts, scipy's border value 0).  ONE 6-stencil pass of the HIP first-layer kernel over the array (the
    labels are shifted by one on the way in so that a shell voxel labelled 0 stays distinguishable from "not in the shell")."""
    a = np.asarray(mask_img)
    if a.ndim not in (2, 3) or a.dtype.kind not in "ui":
        raise ValueError("wall() takes a 2D / 3D integer label image")
    if a.size == 0:
        return a.ravel()
    top = int(a.max())
    if int(a.min()) < 0 or top > 0xFFFFFFFD or not 0 <= int(label_id) <= 0xFFFFFFFD:
        raise ValueError("labels must lie in [0, 2^32 - 3]")
    vol = np.ascontiguousarray(a if a.ndim == 3 else a[:, :, None]).astype(np.uint16 if top < 0xFFFF else np.uint32) + 1
    with _capi.Context(device) as ctx:
        ctx.set_volume(vol)
        shell = ctx.first_layer(int(label_id) + 1, False, vol)         # the shifted labels of the shell, 0 elsewhere
    return (shell[shell != 0] - 1).astype(a.dtype)


def contact_surface(mask_img, label_id, device=0):
    """The set of labels in contact with cell `label_id` in `mask_img` (SIA:55-60)."""
    return set(np.unique(wall(mask_img, label_id, device)).tolist())


def coordinates_centering3D(coordinates, mean=[]):
    """Coordinates (3 x N, or N x 3) centred on their mean -- or on `mean` -- as a 3 x N array (SIA:123-135)."""
    try:
        x, y, z = coordinates
    except (ValueError, TypeError):
        x, y, z = np.asarray(coordinates).T
    if len(mean) == 0:
        mean = np.mean(np.array([x, y, z]), 1)
    return np.array([x - mean[0], y - mean[1], z - mean[2]])


def compute_covariance_matrix(coordinates):
    """(1 / max(shape)) * P . P^T of a point set given as 3 x N (or N x 3 with N > 3) (SIA:137-150)."""
    coordinates = np.asarray(coordinates)
    if coordinates.shape[0] > 3:
        coordinates = coordinates.T
    return 1. / max(coordinates.shape) * np.dot(coordinates, coordinates.T)


def eigen_values_vectors(cov_matrix):
    """Eigenvalues in decreasing order and the eigenvectors BY ROWS of a covariance matrix of size <= 3 (SIA:152-167)."""
    cov_matrix = np.asarray(cov_matrix)
    assert max(cov_matrix.shape) <= 3
    eig_val, eig_vec = np.linalg.eig(cov_matrix)
    order = eig_val.argsort()[::-1]
    return eig_val[order], np.array(eig_vec[:, order]).T


def distance(ptsA, ptsB):
    """Euclidean distance between two 2D or 3D points; None (with a warning) when their dimensions differ (SIA:169-188)."""
    if len(ptsA) != len(ptsB):
        warnings.warn("It seems that the points are not in the same space!")
        return None
    if len(ptsA) in (2, 3):
        return float(np.sqrt(sum((float(a) - float(b)) ** 2 for a, b in zip(ptsA, ptsB))))
    return None


def return_list_of_vectors(tensor, by_row=True):
    """SIA:191-201."""
    if isinstance(tensor, dict):
        return dict((k, return_list_of_vectors(t, by_row)) for k, t in tensor.items())
    if isinstance(tensor, list) and len(tensor) and np.shape(tensor[0]) == (3, 3):
        return [return_list_of_vectors(t, by_row) for t in tensor]
    if by_row:
        return [tensor[v] for v in range(len(tensor))]
    return [tensor[:, v] for v in range(len(tensor))]


def _removable_background(background, dtype):
    """What `m != background` of SIA:90-92 removes: an integer the image's type can hold; anything else (None, a label
    out of range, an object such as the bound method SIA:895 passes) compares unequal everywhere and removes nothing."""
    if isinstance(background, (bool, np.bool_)) or not isinstance(background, _INT + (np.integer,)):
        return None
    info = np.iinfo(dtype)
    return int(background) if info.min <= int(background) <= info.max and int(background) >= 0 else None


def _hollow(resident, image, background, remove_background):
    arr = np.asarray(image)
    bg = _removable_background(background, arr.dtype) if remove_background else None
    out = resident.hollow(0 if bg is None else bg, bg is not None, 8 * arr.dtype.itemsize)
    if arr.ndim == 2:
        out = out[:, :, 0]
    out = out.astype(arr.dtype, copy=False)
    voxelsize = getattr(image, "voxelsize", None)
    return SpatialImage(out, voxelsize=voxelsize) if voxelsize is not None else out


def hollow_out_cells(image, background, remove_background=True, verbose=True, device=0):
    """SIA:74-95: the image with only the cell walls left -- `image * (laplace(image) != 0)`, then without the background.
    The Laplacian is scipy's on an integer image: six face neighbours minus 6 v in the image's own integer type, the edge
    voxel repeated outside; one stencil pass on the GPU (`ta_volume_hollow`).  A non-negative integer image is needed;
    the sums wrap modulo 2^bits of its type -- what scipy does for unsigned types, and for signed ones as long as
    v[-1] - 2 v + v[+1] stays in range (labels below 2^29 in an int32 image)."""
    from .extraction import ResidentVolume
    if verbose:
        print("Hollowing out cells... ", end="")
    resident = ResidentVolume(np.asarray(image), device=device)
    try:
        m = _hollow(resident, image, background, remove_background)
    finally:
        resident.close()
    if verbose:
        print("Done !!")
    return m


class AbstractSpatialImageAnalysis(object):
    """Same surface as SIA:206-1176 for the hot-path methods; results come from one `Extraction`."""

    def __init__(self, image, ignoredlabels=[], return_type=DICT, background=None,
                 device=0, extraction=None):
        # SIA:223-270
        if isinstance(image, SpatialImage):
            self.image = image
        else:
            self.image = SpatialImage(image)
        if isinstance(ignoredlabels, _INT):
            ignoredlabels = [ignoredlabels]
        self._ignoredlabels = set(int(i) for i in ignoredlabels)
        if background is not None and not isinstance(background, _INT):
            raise ValueError("The label you provided as background is not an integer !")
        try:
            self._voxelsize = image.voxelsize
        except AttributeError:
            self._voxelsize = np.ones(len(self.image.shape))
        if len(self._voxelsize) == 2:
            self._voxelsize = tuple(self._voxelsize) + (1.0,)
        self._background = background
        self._labels = None
        self._bbox = None
        self._kernels = None
        self._neighbors = None
        self._cell_layer1 = None
        self._center_of_mass = {}
        self._walls = None
        self._wall_medians = None
        self._signal_cache = None
        self._mesh_cache = {}
        self._junctions = None
        self._wall_geometry = None
        self._components = None
        self._topology = None
        self._extents = {}
        self._distance_cache = {}
        try:
            self.filepath, self.filename = split(image.info["Filename"])
        except Exception:
            self.filepath, self.filename = None, None
        try:
            self.info = dict((k, v) for k, v in image.info.items() if k != "Filename")
        except Exception:
            pass
        self.return_type = return_type
        self._device = device
        self._rv = None
        self._voxel_layer1 = None
        self._voxel_layer18 = None
        self._x = extraction if extraction is not None else self._sweep()
        if background is not None:
            if not self._x.has(int(background)):
                print(" WARNING!!! The background you provided has not been detected in the image !")
            self._ignoredlabels.update([int(background)])
        else:
            warnings.warn("No value defining the background, some functionalities won't work !")

    # -- the only place voxels are touched: ONE upload per analysis object, one fused sweep on the GPU; the wall
    # voxels, the relabelling passes, the property images and the first voxel layer reuse the resident copy
    def _resident(self):
        from .extraction import ResidentVolume
        if getattr(self, "_rv", None) is None:
            self._rv = ResidentVolume(np.asarray(self.image), device=self._device)
        return self._rv

    def _resident_rows(self):
        """The resident volume in the state its label tables (one entry per ROW of the sweep) need: compacted with the ids of
        the extraction when those are sparse -- a lookup table over ids up to 2^32 is not something to build."""
        rv = self._resident()
        if self._x.sparse and not rv.ctx.is_compact():
            rv.ctx.compact_labels(self._x.ids)
        elif not self._x.sparse and rv.ctx.is_compact():
            raise RuntimeError("the resident volume is compacted but the extraction of this analysis has dense rows")
        return rv

    def _sweep(self):
        return self._resident().extract(_capi.F_ALL)

    def refresh(self):
        """Re-upload and re-run the sweep after ``self.image`` was modified in place."""
        self._resident().upload(np.asarray(self.image))
        self._x = self._sweep()
        self._forget()

    def _forget(self):
        """Drop everything derived from the labels of the image."""
        self._labels = None
        self._bbox = None
        self._neighbors = None
        self._cell_layer1 = None
        self._center_of_mass = {}
        self._walls = None
        self._wall_medians = None
        self._signal_cache = None
        self._sigmom_cache = None
        self._pair_cache = None
        self._mesh_cache = {}
        self._junctions = None
        self._wall_geometry = None
        self._components = None
        self._topology = None
        self._extents = {}
        self._distance_cache = {}
        self._voxel_layer1 = None
        self._voxel_layer18 = None

    @property
    def extraction(self):
        return self._x

    def is3D(self):
        return False

    def background(self):
        return self._background

    def ignoredlabels(self):
        return self._ignoredlabels

    def add2ignoredlabels(self, list2add, verbose=False):  # SIA:279-289
        if isinstance(list2add, _INT):
            list2add = [list2add]
        self._ignoredlabels.update(int(i) for i in list2add)
        self._labels = self.__labels()

    def consideronlylabels(self, list2consider, verbose=False):  # SIA:291-306
        if isinstance(list2consider, _INT):
            list2consider = [list2consider]
        toignore = set(int(v) for v in self._x.present()) - set(int(i) for i in list2consider)
        self._ignoredlabels.update(toignore)
        self._labels = self.__labels()

    def convert_return(self, values, labels=None, overide_return_type=None):  # SIA:309-334
        rt = self.return_type if overide_return_type is None else overide_return_type
        if labels is not None and isinstance(labels, _INT):
            return values
        if rt == NPLIST:
            return values
        if rt == LIST:
            return values if isinstance(values, list) else values.tolist()
        return dict(zip(labels, values))

    # -- labels (SIA:337-414)
    def labels(self):
        if self._labels is None:
            self._labels = self.__labels()
        return self._labels

    def __labels(self):
        return self._label_array().tolist()

    def _label_array(self):
        """The labels of the image that are not ignored, ascending (int64)."""
        present = self._x.present()
        if not self._ignoredlabels:
            return present
        ignored = np.fromiter(self._ignoredlabels, dtype=np.int64, count=len(self._ignoredlabels))
        return present[~np.isin(present, ignored)]

    def _request_array(self, labels):
        """`label_request` as an int64 array (what the array paths index the accumulators with)."""
        if labels is None:
            return np.asarray(self.labels(), dtype=np.int64)
        return np.asarray(self.label_request(labels), dtype=np.int64)

    def nb_labels(self):
        return len(self.labels())

    def label_request(self, labels):
        if isinstance(labels, _INT):
            if int(labels) not in self.labels():
                print("The following id was not found within the image labels: {}".format(labels))
            return [int(labels)]
        if isinstance(labels, list):
            known = set(self.labels())
            asked = set(int(l) for l in labels)
            missing = sorted(asked - known)
            if missing:
                print("The following ids were not found within the image labels: {}".format(missing))
            return sorted(asked & known)
        if labels is None:
            return self.labels()
        if isinstance(labels, str):
            key = labels.lower()
            if key == "all":
                return self.labels()
            if key == "l1":
                return self.cell_first_layer()
            if key == "l2":
                return self.cell_second_layer()
            return labels
        raise ValueError("This is not usable as `labels`: {}".format(labels))

    # -- barycentre (SIA:417-480): sum1 / count from the sweep
    def center_of_mass(self, labels=None, real=True, verbose=False):
        labels = self.label_request(labels)
        idx = np.asarray(labels, dtype=np.int64)
        if idx.size:                                 # (an id the image does not hold -- label_request printed it -- gets row 0's)
            known = self._x.rows_of(idx, missing=-1) >= 0
            com = self._x.barycenters(np.where(known, idx, self._x.labels_of(0)))
        else:
            com = np.zeros((0, 3))
        if len(self._center_of_mass) < len(labels):                  # the reference's cache, voxel units (SIA:471)
            self._center_of_mass.update(zip(labels, com))
        if real:
            com = com * np.asarray(self._voxelsize, dtype=np.float64)
        if len(labels) == 1:
            return com[0]
        if self.return_type == NPLIST:
            return com
        return dict(zip(labels, com))

    # -- bounding boxes (SIA:483-535): min/max from the sweep, list indexed by label - 1
    def _bbox_list(self):
        if self._bbox is None:
            present = self._x.present()
            top = int(present.max()) if present.size else 0
            self._bbox = self._x.bbox_slices_upto(top)
        return self._bbox

    def _bbox_slices(self, labels):
        """label -> (slice, slice, slice) or None, whatever `return_type` is: what the methods that crop the image need
        (under NPLIST `boundingbox(list)` answers with an [n, 6] array, which indexes nothing)."""
        boxes = self._bbox_list()
        return dict((c, boxes[c - 1] if 1 <= c <= len(boxes) else None) for c in labels)

    def boundingbox(self, labels=None, real=False):
        if labels is not None and not isinstance(labels, list) and labels == 0:
            zero = self._x.bbox_slices(0)
            if zero is None:
                raise IndexError("list index out of range")   # nd.find_objects(image == 0)[0]
            return zero
        if labels is None:
            labels = copy.copy(self.labels())
            if self.background() is not None:
                labels.append(self.background())
        if isinstance(labels, list) and self.return_type == NPLIST:
            idx = np.asarray(labels, dtype=np.int64)
            if idx.size and (idx.min() < 1 or idx.max() > self._x.max_label):
                raise IndexError("list index out of range")
            box = self._x.bbox[self._x.rows_of(idx)]
            return box * np.tile(np.asarray(self._voxelsize, dtype=np.float64), 2) if real else box
        boxes = self._bbox_list()
        if isinstance(labels, list):
            found = [boxes[i - 1] for i in labels]
            if real:
                return self.convert_return([real_indices(b, self._voxelsize) for b in found], labels)
            return self.convert_return(found, labels)
        try:
            if labels < 1:
                raise IndexError
            if real:
                return real_indices(boxes[labels - 1], self._voxelsize)
            return boxes[labels - 1]
        except Exception:
            return None

    # -- neighbours (SIA:538-693): rows of the face-pair adjacency from the sweep
    def neighbors(self, labels=None, min_contact_area=None, real_area=True, verbose=True):
        if labels is None:
            return self._all_neighbors(min_contact_area, real_area)
        if not isinstance(labels, list):
            return self._neighbors_with_mask(labels, min_contact_area, real_area)
        return self._neighbors_from_list_with_mask(labels, min_contact_area, real_area)

    def _neighbors_with_mask(self, label, min_contact_area=None, real_area=True):
        neigh = self._x.neighbors_of(int(label))
        if min_contact_area is not None:
            neigh = self._neighbors_filtering_by_contact_area(label, neigh, min_contact_area, real_area)
        return neigh

    def _neighbors_from_list_with_mask(self, labels, min_contact_area=None, real_area=True):
        edges = {}
        for label in labels:
            edges[label] = self._neighbors_with_mask(label, min_contact_area, real_area)
        return edges

    def _all_neighbors(self, min_contact_area=None, real_area=True):
        if self._neighbors is None:
            keys = copy.copy(self.labels())                              # the keys of boundingbox() (SIA:639)
            if self.background() is not None:
                keys.append(self.background())
            if self.return_type in (NPLIST, LIST):
                keys = list(range(1, len(keys) + 1))                     # SIA:642-645, as written: re-keyed by position
            # (NPLIST: a mapping view over the adjacency's CSR arrays -- the lists are made when a label is looked up)
            self._neighbors = self._x.neighbor_rows(keys) if self.return_type == NPLIST else self._x.neighbor_lists(keys)
        if min_contact_area is None:
            return self._neighbors
        return self._filter_with_area(self._neighbors, min_contact_area, real_area)

    def _filter_with_area(self, neighborhood_dictionary, min_contact_area, real_area):
        return dict((l, self._neighbors_filtering_by_contact_area(l, neighborhood_dictionary[l], min_contact_area, real_area))
                    for l in neighborhood_dictionary)

    def _neighbors_filtering_by_contact_area(self, label, neighbors, min_contact_area, real_area):
        areas = self.cell_wall_area(label, list(neighbors), real_area)
        nei = copy.copy(list(neighbors))
        for (i, j), area in areas.items():
            if area < min_contact_area:
                nei.remove(i if j == label else j)
        return nei

    def neighbor_kernels(self):
        """The six one-sided 3x3x3 structuring elements of SIA:695-716 (kept for API parity; the
        sweep counts the faces they select directly)."""
        if self._kernels is None:
            ks = []
            for axis in range(3):
                for missing in (0, 2):
                    k = np.zeros((3, 3, 3), dtype=bool)
                    sel = [1, 1, 1]
                    sel[axis] = slice(None)
                    k[tuple(sel)] = True
                    sel[axis] = missing
                    k[tuple(sel)] = False
                    ks.append(k)
            self._kernels = tuple(ks)
        return self._kernels

    def neighbors_number(self, labels=None, min_contact_area=None, real_area=True, verbose=True):
        if self.return_type == NPLIST and min_contact_area is None and (labels is None or isinstance(labels, list)):
            # one degree per label AS ASKED FOR, in the caller's order (an id the image does not hold has no neighbour);
            # labels=None: the keys of _all_neighbors are positions 1..n (SIA:642-645), the k-th value belongs to the k-th label
            if labels is None:
                keys = copy.copy(self.labels())
                if self.background() is not None:
                    keys.append(self.background())
                idx = np.asarray(keys, dtype=np.int64)
            else:
                idx = np.asarray(labels, dtype=np.int64)
            return self._x.degrees_of(idx)
        nei = self.neighbors(labels, min_contact_area, real_area, verbose)
        if isinstance(nei, dict):
            return dict((k, len(v)) for k, v in nei.items())
        return len(nei)

    def get_voxel_face_surface(self):  # SIA:751-756
        a = self._voxelsize
        return np.array([a[1] * a[2], a[2] * a[0], a[0] * a[1]])

    # -- wall areas (SIA:908-993): per-axis shared-face counts x face area
    def cell_wall_area(self, label_id, neighbors, real=True):
        unique_neighbor = not isinstance(neighbors, list)
        if unique_neighbor:
            neighbors = [neighbors]
        faces = self._x.faces_between(int(label_id), [int(n) for n in neighbors]).astype(np.float64)
        if real:
            surf = self.get_voxel_face_surface()
            area = faces[:, 0] * float(surf[0]) + faces[:, 1] * float(surf[1]) + faces[:, 2] * float(surf[2])
        else:
            area = faces[:, 0] + faces[:, 1] + faces[:, 2]
        wall = {}
        for n, a in zip(neighbors, area):
            key = (min(label_id, n), max(label_id, n))
            wall[key] = wall.get(key, 0.0) + float(a)
        if unique_neighbor:
            return next(iter(wall.values()))
        return wall

    def wall_areas(self, neighbors=None, real=True):
        if neighbors is None:
            # every wall of every label: one pass over the sweep's pair list instead of one cell_wall_area call per label
            # (same dictionary: the walls (l, n), n > l, of the labels l that neighbors() has as keys)
            x = self._x
            nei = self.neighbors()
            keys = np.fromiter(nei.keys(), dtype=np.int64, count=len(nei))
            if x.sparse:
                sel = np.flatnonzero(np.isin(x.lo, keys))
            else:
                is_key = np.zeros(max(x.max_label + 2, int(keys.max()) + 1 if keys.size else 0), dtype=bool)
                is_key[keys] = True
                sel = np.flatnonzero(is_key[x.lo])
            area = x.pair_areas(self.get_voxel_face_surface() if real else None)[sel]
            if self.return_type == NPLIST:
                return np.stack([x.lo[sel], x.hi[sel]], axis=1), area
            return dict(zip(zip(x.lo[sel].tolist(), x.hi[sel].tolist()), area.tolist()))
        areas = {}
        for label_id, lneighbors in neighbors.items():
            neigh = [n for n in lneighbors if n > label_id]
            if len(neigh) > 0:
                for key, val in self.cell_wall_area(label_id, neigh, real=real).items():
                    areas[key] = areas.get(key, 0.0) + val
        return areas

    # -- a second image on another grid (include/tissue_scan_resample.h; one gather pass on the GPU)
    def _index_matrix(self, image, transform, voxelsize):
        """None when `image` is taken as lying on this grid (no transform and no voxel size named): today's path.  Else the 3 x 4
        index matrix from this grid into `image`'s: `transform` maps physical coordinates of this image to those of `image`
        (None = identity), whose voxel size is `voxelsize`, or its own (a SpatialImage), or this image's."""
        if transform is None and voxelsize is None:
            return None
        from .resample import index_matrix
        if voxelsize is None:
            voxelsize = getattr(image, "voxelsize", self._voxelsize)
        return index_matrix(transform, self._voxelsize, voxelsize)

    def resample_onto_grid(self, image, transform=None, order=0, fill=0, voxelsize=None):
        """`image` (any shape; uint8 / uint16 / uint32) resampled onto this analysis' grid on the GPU: a SpatialImage with this
        image's shape and voxel size.  `transform`: the homogeneous matrix (4 x 4, 3 x 3 for 2-D images) from physical
        coordinates of this image to those of `image`, None = identity, so that only the voxel sizes differ; order 0 nearest
        neighbour (labels), 1 trilinear (signals); `fill` where `image` has no voxel."""
        from .resample import index_matrix
        vs = getattr(image, "voxelsize", self._voxelsize) if voxelsize is None else voxelsize
        out = self._resident().resample(np.asarray(image), index_matrix(transform, self._voxelsize, vs), order, fill).image()
        return SpatialImage(out, voxelsize=tuple(self._voxelsize))

    # -- intensity statistics of a signal image over the labels (include/tissue_scan_signal.h; one pass on the GPU)
    def _signal_stats(self, signal, matrix=None):
        """SignalStats of `signal` over this image: uploaded and reduced once per array OBJECT (a signal modified in place
        needs a new array, or refresh()) and index matrix, on the resident label volume."""
        cache = getattr(self, "_signal_cache", None)
        key = None if matrix is None else matrix.tobytes()
        if cache is not None and cache[0] is signal and cache[2] == key:
            return cache[1]
        stats = self._resident_rows().signal(np.asarray(signal), walls=True, matrix=matrix)
        self._signal_cache = (signal, stats, key)
        return stats

    def cell_signal(self, signal, labels=None, statistic='mean', transform=None, voxelsize=None):
        """Per-label `statistic` of the intensity image `signal` (uint8 / uint16, the image's shape): 'mean', 'std'
        (population), 'min', 'max' (float64) or 'sum' (integer); returned like volume().  With `transform` (physical coordinates
        of this image -> those of `signal`) and / or `voxelsize` (of `signal`; a SpatialImage brings its own) the signal may lie
        on any grid: it is resampled onto this one on the GPU, trilinearly -- so for wall_signal, signal_quantiles,
        signal_median and signal_histogram."""
        if statistic not in STATISTICS:
            raise ValueError("statistic must be one of %s, not %r" % ("|".join(STATISTICS), statistic))
        labels = self.label_request(labels)
        values = self._signal_stats(signal, self._index_matrix(signal, transform, voxelsize)).of_labels(labels, statistic)
        return self.convert_return(values, labels)

    def wall_signal(self, signal, neighbors=None, statistic='mean', transform=None, voxelsize=None):
        """{(l1, l2): value} for the walls wall_areas(neighbors) returns: 'mean' = the signal averaged over both sides of every
        face of the wall (face-weighted, like the wall area), 'sides' = (mean on l1's side, mean on l2's side), l1 < l2."""
        if statistic not in WALL_STATISTICS:
            raise ValueError("statistic must be one of %s, not %r" % ("|".join(WALL_STATISTICS), statistic))
        walls = self.wall_areas(neighbors, real=False)
        if isinstance(walls, tuple):
            keys = [tuple(k) for k in np.asarray(walls[0]).tolist()]
        else:
            keys = list(walls.keys())
        stats = self._signal_stats(signal, self._index_matrix(signal, transform, voxelsize))
        lo = np.array([k[0] for k in keys], dtype=np.int64)
        hi = np.array([k[1] for k in keys], dtype=np.int64)
        rows = stats.wall_rows(lo, hi)
        if statistic == 'mean':
            col = stats.wall_mean
            return dict((k, float(col[r]) if r >= 0 else float('nan')) for k, r in zip(keys, rows.tolist()))
        a, b = stats.wall_side_means
        return dict((k, (float(a[r]), float(b[r])) if r >= 0 else (float('nan'), float('nan'))) for k, r in zip(keys, rows.tolist()))

    # -- where in the cell the signal sits (include/tissue_scan_sigmoments.h; one pass on the GPU)
    def _signal_moments(self, signal):
        """SignalMoments of `signal` over this image: uploaded and reduced once per array OBJECT, like `_signal_stats`."""
        cache = getattr(self, "_sigmom_cache", None)
        if cache is not None and cache[0] is signal:
            return cache[1]
        moments = self._resident_rows().signal_moments(np.asarray(signal), self._voxelsize)
        self._sigmom_cache = (signal, moments)
        return moments

    def _signal_moment_column(self, signal, labels, column, real):
        labels = self.label_request(labels)
        values = self._signal_moments(signal).of_labels(labels, column, real)
        if len(labels) == 1:
            return values[0]
        return self.convert_return(values if self.return_type == NPLIST else list(values), labels)

    def signal_center_of_mass(self, signal, labels=None, real=True):
        """Per label the centroid of the intensity image `signal` (uint8 / uint16, the image's shape) over the label's voxels,
        what scipy.ndimage.center_of_mass(signal, image, labels) gives (times the voxel size with `real`); NaN for a label
        without signal.  Returned like center_of_mass()."""
        return self._signal_moment_column(signal, labels, "centroid", real)

    def signal_polarity(self, signal, labels=None, real=True, normalised=False):
        """Per label the vector from the cell's barycentre to its signal centroid; normalised: divided by the cell's radius of
        gyration (dimensionless, 0 for a uniform signal).  Returned like center_of_mass()."""
        labels = self.label_request(labels)
        m = self._signal_moments(signal)
        rows = m.rows_of(np.asarray(labels, dtype=np.int64).reshape(-1), missing=-1)
        values = m.polarity(real, normalised)[np.where(rows >= 0, rows, 0)]
        values[rows < 0] = np.nan
        if len(labels) == 1:
            return values[0]
        return self.convert_return(values if self.return_type == NPLIST else list(values), labels)

    def signal_inertia_axis(self, signal, labels=None, real=True):
        """Per label the axes along which the signal is spread: (eigenvectors as rows, eigenvalues) of the signal-weighted
        covariance of the voxel positions, by decreasing eigenvalue; the counterpart of inertia_axis(), returned like it."""
        labels = self.label_request(labels)
        m = self._signal_moments(signal)
        rows = m.rows_of(np.asarray(labels, dtype=np.int64).reshape(-1), missing=-1)
        vecs, vals = m.inertia_axis(real)
        at = np.where(rows >= 0, rows, 0)
        vecs, vals = vecs[at], vals[at]
        vecs[rows < 0] = np.nan
        vals[rows < 0] = np.nan
        if len(labels) == 1:
            return return_list_of_vectors(vecs[0]), vals[0]
        if self.return_type == NPLIST:
            return vecs, vals
        axes = [list(v) for v in vecs]
        return self.convert_return(axes, labels), self.convert_return(list(vals), labels)

    # -- two channels per cell (include/tissue_scan_cosignal.h; one pass over labels + both channels on the GPU)
    def _channel_pair(self, a, b, thresholds=(0, 0)):
        """ChannelPairStats of the channels `a`, `b` over this image: uploaded and reduced once per pair of array OBJECTS and
        thresholds, like `_signal_stats`."""
        thresholds = (int(thresholds[0]), int(thresholds[1]))
        cache = getattr(self, "_pair_cache", None)
        if cache is not None and cache[0] is a and cache[1] is b and cache[2] == thresholds:
            return cache[3]
        bb = np.asarray(b)
        pair = self._resident_rows().signal_pair(bb if a is b else np.asarray(a), bb, thresholds)
        self._pair_cache = (a, b, thresholds, pair)
        return pair

    def signal_ratio(self, a, b, labels=None):
        """Per label the ratio sum(a) / sum(b) of two intensity images (uint8 / uint16 each, the image's shape) over the label's
        voxels -- the read-out of a ratiometric reporter; NaN where sum(b) == 0.  Returned like volume().  Both channels lie on
        this image's grid: one on another grid goes through resample_onto_grid(order=1) first (there is no `transform=` here:
        the resample pass owns one result buffer)."""
        labels = self.label_request(labels)
        return self.convert_return(self._channel_pair(a, b).of_labels(labels, "ratio"), labels)

    def signal_correlation(self, a, b, labels=None):
        """Per label Pearson's correlation coefficient of the two intensity images over the label's voxels; NaN for a label of
        fewer than two voxels or with a constant channel.  Returned like volume()."""
        labels = self.label_request(labels)
        return self.convert_return(self._channel_pair(a, b).of_labels(labels, "pearson"), labels)

    def signal_colocalisation(self, a, b, thresholds, labels=None):
        """Per label Manders' coefficients (M1, M2) for thresholds = (t_a, t_b): M1 the fraction of sum(a) that lies in voxels with
        b > t_b, M2 the fraction of sum(b) in voxels with a > t_a.  One pair per label, returned like volume() (NPLIST: an array
        [labels, 2])."""
        labels = self.label_request(labels)
        pair = self._channel_pair(a, b, thresholds)
        values = np.stack([pair.of_labels(labels, "manders_m1"), pair.of_labels(labels, "manders_m2")], axis=1)
        return self.convert_return(values if self.return_type == NPLIST else [tuple(v) for v in values.tolist()], labels)

    # -- exact histograms, medians and quantiles of a signal image (include/tissue_scan_sighist.h; radix select on the GPU)
    def signal_quantiles(self, signal, q, labels=None, method='linear', transform=None, voxelsize=None):
        """Per label the quantiles `q` (a sequence in [0, 1]) of the intensity image `signal` (uint8 / uint16, the image's shape),
        by numpy.quantile's rule for `method` ('linear', 'lower', 'higher' or 'midpoint') over the exact order statistics of the
        label's voxels.  One array of len(q) per label, returned like volume() (NPLIST: an array [labels, len(q)])."""
        labels = self.label_request(labels)
        sq = self._resident_rows().signal_quantiles(np.asarray(signal), q, method, matrix=self._index_matrix(signal, transform, voxelsize))
        return self.convert_return(sq.of_labels(labels), labels)

    def signal_median(self, signal, labels=None, transform=None, voxelsize=None):
        """Per label the median of the intensity image `signal` over the label's voxels (float64, what numpy.median of them
        gives, NaN for a label without voxels); returned like volume()."""
        labels = self.label_request(labels)
        sq = self._resident_rows().signal_quantiles(np.asarray(signal), [0.5], 'midpoint', matrix=self._index_matrix(signal, transform, voxelsize))
        return self.convert_return(sq.of_labels(labels)[:, 0], labels)

    def signal_histogram(self, signal, labels=None, bin_width=None, transform=None, voxelsize=None):
        """Per label the histogram of the intensity image `signal`: uint64 counts of the bins [b * bin_width, (b + 1) * bin_width),
        `bin_width` a power of two that leaves at most 256 bins (default 1 for uint8, 256 for uint16).  One array per label,
        returned like volume() (NPLIST: an array [labels, bins])."""
        labels = self.label_request(labels)
        h = self._resident_rows().signal_histogram(np.asarray(signal), bin_width, matrix=self._index_matrix(signal, transform, voxelsize))
        return self.convert_return(h.of_labels(labels), labels)

    # -- cell surface meshes (include/tissue_scan_mesh.h; count, scan and emit on the GPU)
    def cell_meshes(self, labels=None, sub_factor=1):
        """The exact voxel-face surface meshes of `labels` (default: labels(), so no background and no ignored label) on
        image[::sub_factor, ::sub_factor, ::sub_factor], in real units (voxel size times sub_factor): a `CellMeshes`,
        `meshes[label]` = (points, triangles).  Unlike the reference (VTK marching cubes and smoothing on an image subsampled
        by interpolation), no smoothing and a strided subsampling.  Cached per argument set until the image changes."""
        wanted = tuple(self.labels()) if labels is None else tuple(self.label_request(labels))
        key = (wanted, int(sub_factor))
        cache = getattr(self, "_mesh_cache", None)
        if cache is None:
            cache = self._mesh_cache = {}
        if key not in cache:
            vs = tuple(float(v) for v in self._voxelsize)
            cache[key] = self._resident_rows().meshes(list(wanted), int(sub_factor), vs)
        return cache[key]

    # -- overlap with a second label image of the same grid (include/tissue_scan_overlap.h; one pass on the GPU)
    def overlap(self, other_image, transform=None, voxelsize=None, fill=0):
        """The overlap table of this image with `other_image` (the next frame, or another segmentation of the same image): a
        `LabelOverlap` of rows (a, b, n) in the ids of the two images.  Nothing is excluded here:
        `overlap(next).lineage(exclude=(0, analysis.background()))` leaves the background out.  The two share a grid, or
        `transform` (physical coordinates of this image -> those of `other_image`, None = identity) and / or `voxelsize` (of
        `other_image`; a SpatialImage brings its own) place the other image, of any shape: it is resampled onto this grid on
        the GPU by nearest neighbour, voxels where it has none reading as the label `fill`."""
        return self._resident().overlap(np.asarray(other_image), self._index_matrix(other_image, transform, voxelsize), fill)

    # -- cell junctions (include/tissue_scan_junctions.h; two walks over the resident volume on the GPU)
    def cell_junctions(self):
        """The lines where three cells meet and the points where four cells meet: a `CellJunctions` in the ids of the image and
        with this analysis' voxel size.  Nothing is excluded here (the background and the ignored labels have rows): the
        methods of the result take an `exclude`.  Cached until `refresh()` or an edit of the image."""
        if getattr(self, "_junctions", None) is None:
            self._junctions = self._resident().junctions(tuple(float(v) for v in self._voxelsize))
        return self._junctions

    def cell_vertices(self, real=True):
        """{(a, b, c, d): xyz} of every point where four labels meet (none excluded)."""
        return self.cell_junctions().cell_vertices(real=real)

    # -- connected components of the labels (include/tissue_scan_components.h; a union-find over the resident volume on the GPU)
    def label_components(self):
        """One row per face-connected blob of equal label: a `LabelComponents` in the ids of the image and with this analysis'
        voxel size.  Nothing is excluded here (the background and the ignored labels have rows).  Cached until `refresh()` or
        an edit of the image."""
        if getattr(self, "_components", None) is None:
            self._components = self._resident().components(tuple(float(v) for v in self._voxelsize))
        return self._components

    def disconnected_labels(self):
        """{label: k} of the labels whose voxels form k > 1 separate blobs, without the ignored labels."""
        return self.label_components().fragmented(exclude=self._ignoredlabels)

    # -- Euler numbers: tunnels and cavities (include/tissue_scan_topology.h; one pass over the resident volume on the GPU)
    def cell_topology(self):
        """The twelve exact block counts of every label and what follows from them: a `CellTopology` (Euler numbers for 6- and
        26-connectivity, intrinsic volumes) in the ids of the image and with this analysis' voxel size.  Nothing is excluded
        here.  Cached until `refresh()` or an edit of the image."""
        if getattr(self, "_topology", None) is None:
            self._topology = self._resident_rows().topology(tuple(float(v) for v in self._voxelsize))
        return self._topology

    def euler_number(self, labels=None, connectivity=6):
        """Per label the Euler number of its voxels, joined across faces (connectivity 6) or across faces, edges and corners
        (26): blobs - tunnels + cavities.  A ball gives 1, a cell with a tunnel through it 0, one that encloses a cavity 2.
        Returned like volume()."""
        labels = self.label_request(labels)
        return self.convert_return(self.cell_topology().of_labels(labels, "euler_number", connectivity), labels)

    def mean_breadth(self, labels=None, real=True):
        """Per label the mean breadth of its voxel solid (half the intrinsic volume V1; a box of a x b x c voxels gives
        (a s0 + b s1 + c s2) / 2), in real units or in voxels; returned like volume()."""
        labels = self.label_request(labels)
        vs = None if real else (1.0, 1.0, 1.0)
        return self.convert_return(self.cell_topology().of_labels(labels, "mean_breadth", voxelsize=vs), labels)

    def topological_defects(self, exclude=()):
        """{label: {'blobs': b0, 'euler': chi6, 'tunnels_minus_cavities': b0 - chi6}} of the labels that are not unions of balls:
        those whose face-connected Euler number differs from the number of their face-connected blobs (`label_components()`),
        without those in `exclude`.  For 6-connectivity only: the components are face-connected."""
        from .cell_topology import topological_defects
        return topological_defects(self.cell_topology(), self.label_components(), exclude)

    # -- oriented extents: length, width, depth (include/tissue_scan_extents.h; one pass over the resident volume on the GPU)
    def cell_extents(self, axes=None, real=True):
        """How far every label reaches along three directions of its own: a `CellExtents` (lengths, oriented box, fill) in the
        ids of the image, with this analysis' voxel size (ones with real=False).  axes: None = every cell's principal axes, those
        of its PHYSICAL covariance from the sweep's exact moments, by decreasing eigenvalue; or one direction (completed to a
        frame), one [3, 3] frame for every cell, or {label: [3, 3]} (the other labels take the image axes), in array axes.
        Nothing is excluded here.  With axes=None cached per `real` until `refresh()` or an edit of the image; not cached with
        axes of the caller's."""
        vs = tuple(float(v) for v in self._voxelsize) if real else (1.0, 1.0, 1.0)
        if axes is not None:
            return self._resident_rows().cell_extents(axes, vs)
        cache = getattr(self, "_extents", None)
        if cache is None:
            cache = self._extents = {}
        if bool(real) not in cache:
            cache[bool(real)] = self._resident_rows().cell_extents(None, vs)
        return cache[bool(real)]

    def cell_lengths(self, labels=None, real=True):
        """Per label its extents along its principal axes, ordered major, middle, minor axis: how long, wide and thick the cell
        is (the exact extent of the union of its voxel boxes; NaN for a label without voxels).  Returned like center_of_mass()."""
        labels = self.label_request(labels)
        values = self.cell_extents(real=real).of_labels(labels, "lengths")
        if len(labels) == 1:
            return values[0]
        return self.convert_return(values if self.return_type == NPLIST else list(values), labels)

    def cell_extent_along(self, direction, labels=None, real=True):
        """Per label its extent along `direction` (array axes; say, the organ axis); returned like volume()."""
        labels = self.label_request(labels)
        return self.convert_return(self.cell_extents(direction, real).of_labels(labels, "lengths")[:, 0], labels)

    def box_fill(self, labels=None):
        """Per label the share of its oriented box (along its principal axes) that the cell fills: 1 for a cuboid, 0.52 for a
        ball; returned like volume()."""
        labels = self.label_request(labels)
        return self.convert_return(self.cell_extents().of_labels(labels, "fill"), labels)

    # -- exact Euclidean distance maps (include/tissue_scan_distance.h; three passes over the resident volume on the GPU)
    def _distance_map(self, mode, label, edge, real):
        cache = getattr(self, "_distance_cache", None)
        if cache is None:
            cache = self._distance_cache = {}
        key = (int(mode), None if label is None else int(label), bool(edge), bool(real))
        if key not in cache:
            vs = tuple(float(v) for v in self._voxelsize) if real else (1.0, 1.0, 1.0)
            cache[key] = self._resident_rows().distance_map(mode, label, vs, bool(edge))
        return cache[key]

    def wall_distance(self, edge_is_wall=False, real=True):
        """The distance of every voxel to the nearest voxel of another label -- to its own cell's wall: a `DistanceMap` in the ids of
        the image, with this analysis' voxel size (ones with real=False).  With `edge_is_wall` the image margin bounds the cells it
        cuts.  Nothing is excluded here; `.image()` downloads the distances.  Cached per argument set until `refresh()` or an edit
        of the image."""
        return self._distance_map(_capi.DIST_OWN_WALL, None, edge_is_wall, real)

    def distance_from(self, label=None, edge_is_wall=False, real=True):
        """The distance of every voxel to the nearest voxel of `label` (default: the background): a `DistanceMap`, as above."""
        if label is None:
            label = self.background()
        if label is None:
            raise ValueError("distance_from needs a label (this analysis has no background)")
        return self._distance_map(_capi.DIST_FROM_LABEL, int(label), edge_is_wall, real)

    def inscribed_radius(self, labels=None, real=True):
        """Per label the radius of its largest inscribed sphere centred on a voxel: the largest distance of its voxels to a voxel
        of another label (+inf for an image of one label); returned like volume().  `wall_distance().pole()` is where it sits."""
        labels = self.label_request(labels)
        return self.convert_return(self.wall_distance(real=real).of_labels(labels, "max2"), labels)

    def cell_depth(self, labels=None, real=True):
        """Per label the smallest distance of its voxels to the background: a continuous depth below the tissue surface, where
        cell_first_layer() gives a layer index; returned like volume()."""
        labels = self.label_request(labels)
        return self.convert_return(self.distance_from(real=real).of_labels(labels, "min2"), labels)

    # -- nearest-label maps (include/tissue_scan_nearest.h; three passes over the resident volume on the GPU)
    def nearest_labels(self, empty=0, max_distance=None, not_from=None, real=True):
        """For every voxel the nearest voxel that is neither `empty` nor `not_from` (None: nothing excluded), the smallest label
        among several that are equally near: a `NearestLabels` in the ids of the image, with this analysis' voxel size (ones with
        real=False, and then `max_distance` is in voxels).  `.gained()` tells what every label would gain from the empty voxels
        within `max_distance` (None: all of them), `.image()` is the image `fill_erased_voxels()` would leave.  Not cached."""
        vs = tuple(float(v) for v in self._voxelsize) if real else (1.0, 1.0, 1.0)
        return self._resident_rows().nearest_labels(int(empty), not_from, vs, max_distance)

    def fill_erased_voxels(self, empty=0, max_distance=None, not_from=None, real=True):
        """Modify the image so that every voxel of `empty` (what `remove_small_fragments`, `remove_labels_from_image` and
        `remove_stack_margin_labels_from_image` erase to) takes the label of the nearest voxel that is neither `empty` nor
        `not_from`, the smallest label among several that are equally near; with `max_distance` only the voxels that far from one
        at most (inclusive; real units, or voxels with real=False).  Returns {label: voxels gained}."""
        rv = self._resident_rows()
        nl = self.nearest_labels(empty, max_distance, not_from, real)
        gained = nl.gained()
        if nl.filled:                                      # (no new label value: nothing to check against the image dtype)
            self._edit_image(rv, np.zeros(0, dtype=np.int64), 0, lambda rv, table: nl.apply())
        return gained

    def expand_labels(self, distance, into=None, real=True):
        """Modify the image so that the labels grow by `distance` into the voxels of `into` (default: the background), every
        voxel going to the label it lies nearest to: skimage.segmentation.expand_labels with a stated rule for ties (the
        smallest label).  Returns {label: voxels gained}."""
        if into is None:
            into = self.background()
        if into is None:
            raise ValueError("expand_labels needs a label to grow into (this analysis has no background)")
        return self.fill_erased_voxels(empty=int(into), max_distance=distance, real=real)

    # -- distance-shell profiles (include/tissue_scan_profile.h; one pass over labels, distances and signal on the GPU)
    def _shell_profile(self, edges, signal, from_label, edge_is_wall, real=True):
        dm = self.wall_distance(edge_is_wall, real) if from_label is None else self.distance_from(from_label, edge_is_wall, real)
        return dm.profile(edges, signal)

    def shell_volumes(self, edges, labels=None, real=True, from_label=None, edge_is_wall=False):
        """Per label the volumes of its shells of distance: entry k is the volume of the label's voxels whose distance to the
        cell's own wall (`from_label`: to the nearest voxel of that label) lies in [edges[k], edges[k + 1]); `edges` ascend
        strictly from >= 0 (64 shells at most, the last edge may be inf), in real units and the volumes too, or both in voxels
        with real=False.  One (K,) array per label, returned like volume()."""
        labels = self.label_request(labels)
        prof = self._shell_profile(edges, None, from_label, edge_is_wall, real)
        unit = float(np.prod(prof.voxelsize))
        values = self._shell_rows(prof, prof.n.astype(np.float64) * unit, labels, 0.0)
        return self.convert_return(values, labels)

    def signal_profile(self, signal, edges, labels=None, statistic='mean', from_label=None, edge_is_wall=False):
        """Per label the `statistic` ('mean', 'std', 'min', 'max', 'sum', or 'fraction': the shell's share of the label's counted
        signal) of the intensity image `signal` (uint8 / uint16, the image's shape) in every shell of distance, the shells as in
        shell_volumes() with distances in real units.  One (K,) array per label, returned like cell_signal()."""
        methods = dict(mean="mean", std="std", min="minimum", max="maximum", sum="total", fraction="fraction")
        if statistic not in methods:
            raise ValueError("statistic must be one of %s, not %r" % ("|".join(methods), statistic))
        labels = self.label_request(labels)
        prof = self._shell_profile(edges, signal, from_label, edge_is_wall)
        by_label = getattr(prof, methods[statistic])(labels=labels)
        empty = np.zeros(prof.shells, dtype=np.uint64) if statistic == "sum" else np.full(prof.shells, np.nan)
        values = [by_label.get(int(l), empty) for l in labels]
        return self.convert_return(values, labels)

    @staticmethod
    def _shell_rows(prof, column, labels, missing):
        rows = prof.rows_of(labels)
        return [column[r] if r >= 0 else np.full(prof.shells, missing) for r in rows.tolist()]

    def _current_components(self):
        """`label_components()`, run again when the context no longer holds the tables it was read from."""
        cc = self.label_components()
        try:
            held = self._resident().ctx.components_size() == len(cc)
        except _capi.TissueScanError:
            held = False
        if not held:
            self._components = None
            cc = self.label_components()
        return cc

    def _relabel_components(self, new_label):
        """Rows of the component table the context holds -> new labels, on the resident volume and in the image."""
        rv = self._resident()
        img = np.asarray(self.image)
        top = int(np.iinfo(rv.host.dtype).max)
        if np.issubdtype(img.dtype, np.integer):           # (new ids: they must survive the write-back too)
            top = min(top, int(np.iinfo(img.dtype).max))
        self._edit_image(rv, np.asarray(new_label, dtype=np.int64), top, lambda rv, table: rv.relabel_components(table))

    def split_disconnected_labels(self):
        """Modify the image so that every label is one face-connected blob: the largest blob of a label keeps the label, every
        other one gets a new id above the largest label, in the order of the component table.  Returns {new id: old label}.
        Raises ValueError, with the image untouched, when a new id does not fit the image dtype."""
        cc = self._current_components()
        new = cc.split_map()
        changed = new != cc.label
        if changed.any():
            self._relabel_components(new)
        return dict(zip(new[changed].tolist(), cc.label[changed].tolist()))

    def remove_small_fragments(self, min_voxels, erase_value=0):
        """Modify the image so that the blobs of a label that are not its largest and have fewer than `min_voxels` voxels read
        `erase_value` (which joins the ignored labels, as in `remove_labels_from_image`).  Returns the number of blobs erased."""
        cc = self._current_components()
        new = cc.erase_map(min_voxels, erase_value)
        changed = new != cc.label
        if changed.any():
            self._relabel_components(new)
            self._ignoredlabels.update([int(erase_value)])
        return int(changed.sum())

    # -- wall geometry (include/tissue_scan_wallgeo.h; one pass over the resident volume on the GPU)
    def wall_geometry(self):
        """Signed face counts, centroid sums and second moments of every wall: a `WallGeometry` in the ids of the image and with
        this analysis' voxel size.  Nothing is excluded here (background walls have rows).  Cached until `refresh()` or an edit
        of the image."""
        if getattr(self, "_wall_geometry", None) is None:
            self._wall_geometry = self._resident_rows().wall_geometry(tuple(float(v) for v in self._voxelsize))
        return self._wall_geometry

    def _wall_geometry_column(self, neighbors, values):
        """`values` (one entry per row of wall_geometry()) for the walls wall_areas(neighbors) returns, in its forms."""
        walls = self.wall_areas(neighbors, real=False)
        geo = self.wall_geometry()
        if isinstance(walls, tuple):
            pairs = np.asarray(walls[0]).reshape(-1, 2)
            rows = geo.wall_rows(pairs[:, 0], pairs[:, 1])
            out = np.where((rows >= 0).reshape((-1,) + (1,) * (values.ndim - 1)), values[np.maximum(rows, 0)], np.nan)
            return walls[0], out
        keys = list(walls.keys())
        rows = geo.wall_rows([k[0] for k in keys], [k[1] for k in keys])
        nan = np.full(values.shape[1:], np.nan) if values.ndim > 1 else float('nan')
        return dict((k, (values[r] if values.ndim > 1 else float(values[r])) if r >= 0 else nan) for k, r in zip(keys, rows.tolist()))

    def wall_normals(self, neighbors=None):
        """{(l1, l2): unit normal} for the walls wall_areas(neighbors) returns: along the wall's vector area in real units, from
        l1 to l2 (l1 < l2); NaN for a closed wall."""
        return self._wall_geometry_column(neighbors, self.wall_geometry().normal())

    def wall_projected_areas(self, neighbors=None, real=True):
        """{(l1, l2): area} for the walls wall_areas(neighbors) returns: the norm of the wall's vector area, never more than
        its voxel-face area of wall_areas()."""
        return self._wall_geometry_column(neighbors, self.wall_geometry().projected_area(real))

    def surface_area(self, labels=None, real=True):
        """Per-label total surface area = the sum of the label's wall areas with all its face neighbours
        (SURVEY.md §8 "Semantics": sum_m wall_area(l, m); the reference has no dedicated method, `cell_wall_area`
        SIA:908-959 gives it one wall at a time).  real: F0 vy vz + F1 vz vx + F2 vx vy; else the number of faces."""
        single = isinstance(labels, _INT)
        req = [int(labels)] if single else self.label_request(labels)
        faces = self._x.surface_faces(req).astype(np.float64)
        if real:
            surf = self.get_voxel_face_surface()
            area = faces[:, 0] * float(surf[0]) + faces[:, 1] * float(surf[1]) + faces[:, 2] * float(surf[2])
        else:
            area = faces[:, 0] + faces[:, 1] + faces[:, 2]
        return float(area[0]) if single else self.convert_return(area, req)

    # -- layers and margins (SIA:996-1022): host post-processing of the sweep results
    def cell_first_layer(self, filter_by_area=True, minimal_external_area=10, real_area=True):
        if self._cell_layer1 is None:
            self._cell_layer1 = [int(n) for n in self.neighbors(self.background())]
        cell_layer1 = self._cell_layer1
        if filter_by_area:
            areas = self.cell_wall_area(self.background(), list(self._cell_layer1), real_area)
            cell_layer1 = [l for l in self._cell_layer1
                           if (self.background(), l) in areas
                           and areas[(self.background(), l)] > minimal_external_area]
        return sorted(set(cell_layer1) - self._ignoredlabels)

    def cell_second_layer(self, filter_by_area=True, minimal_L1_area=10, real_area=True):
        l1 = self.cell_first_layer()
        nei = self.neighbors(l1, minimal_L1_area, real_area, True)
        l2 = set()
        for n in nei.values():
            l2.update(int(v) for v in n)
        self._cell_layer2 = sorted(l2 - set(self._cell_layer1) - self._ignoredlabels)
        return self._cell_layer2


    # -- first voxel layer (SIA:1024-1046): `image * (dilate6(image == bg) - (image == bg)) + (image == bg)` as one
    # 6-stencil pass over the resident volume on the GPU
    def voxel_first_layer(self, keep_background=True):
        """First layer of voxels in contact with the background: they keep their label, the rest of the tissue
        becomes 0, the background 1 (keep_background) or 0.  Cached like in the reference (the first call's
        `keep_background` wins, SIA:1044-1046)."""
        if self._voxel_layer1 is None:
            layer = self._resident().first_layer(self.background(), keep_background)
            img = np.asarray(self.image)
            if img.ndim == 2:
                layer = layer[:, :, 0]
            self._voxel_layer1 = SpatialImage(layer.astype(img.dtype, copy=False),
                                              voxelsize=getattr(self.image, "voxelsize", None))
        return self._voxel_layer1

    # -- coordinates of every voxel next to another label (SIA:883-905)
    def cells_walls_coords(self):
        """x, y, z (lists) of the voxels `hollow_out_cells` keeps.  As written in the reference: the background handed to
        it is the bound method `self.background` (SIA:895), which no voxel equals, so background voxels next to a cell
        are returned too; label 0 never is (`image * mask` is 0 there).  2-D images: every voxel that is not 0 (the same
        comparison with the method leaves the background in, SIA:897-898)."""
        if self.is3D():
            image = np.asarray(_hollow(self._resident(), self.image, self.background, True))
            x, y, z = np.where(image != 0)
            return list(x), list(y), list(z)
        x, y = np.where(np.asarray(self.image) != 0)
        return list(x), list(y)

    # -- the first layer of voxels of a cell (SIA:1399-1448): `mask - binary_erosion(mask, 18-structure)` inside a crop.
    # A voxel of the cell is eroded away unless all its 18 neighbours are the cell's AND inside the crop, so the layer is
    # the cell's voxels that have another label among their 18 neighbours -- one stencil pass over the resident volume
    # for every label at once (`ta_volume_layer18`) -- plus the cell's voxels on the faces of the crop.
    def _layer18(self):
        if getattr(self, "_voxel_layer18", None) is None:
            self._voxel_layer18 = self._resident().layer18()
        return self._voxel_layer18

    def cells_voxel_layer(self, labels, region_boundingbox=False, single_frame=False):
        if isinstance(labels, _INT):
            labels = [labels]
        if single_frame:
            region_boundingbox = True
        bbox = bboxes = None
        if not isinstance(region_boundingbox, bool):
            if sum(isinstance(s, slice) for s in region_boundingbox) == 3:
                bbox = tuple(region_boundingbox)
            else:
                print("TypeError: Wong type for 'region_boundingbox', should either be bool or la tuple of slices")
                return None
        elif region_boundingbox:
            bbox = self.region_boundingbox(labels)
        else:
            bboxes = self._bbox_slices(labels)
        image, differs = np.asarray(self.image), self._layer18()
        vox_layer = np.zeros_like(image[bbox], dtype=int) if single_frame else {}
        clabel = None
        for clabel in labels:
            crop = bbox if bbox is not None else bboxes[clabel]
            mask = image[crop] == clabel
            edge = np.zeros(mask.shape, dtype=bool)
            for axis in range(mask.ndim):
                if mask.shape[axis]:
                    first, last = [slice(None)] * mask.ndim, [slice(None)] * mask.ndim
                    first[axis], last[axis] = 0, -1
                    edge[tuple(first)] = True
                    edge[tuple(last)] = True
            layer = np.array(mask & ((differs[crop] != 0) | edge), dtype=int)
            if single_frame:
                vox_layer += layer
            else:
                vox_layer[clabel] = layer
        if len(labels) == 1:
            return vox_layer[clabel]
        return vox_layer

    # -- wall voxels (SIA:759-880, 1049-1111): one GPU pass finds the wall voxels of EVERY pair (18-neighbourhood
    # contact, scipy's generate_binary_structure(3, 2)); the methods below are lookups in that table.
    def wall_table(self):
        if self._walls is None:
            self._walls = self._resident().wall_table()
        return self._walls

    def wall_medians_of(self, keys):
        """The median voxel (TGI:210-242: Weiszfeld position by the reference's rules, truncated, nearest wall voxel) of the
        walls `keys` = lo << 32 | hi (uint64 array).  Returns (found bool[len(keys)], medians int64[found.sum(), 3]).
        With nothing but the resident volume at hand the DEVICE computes the medians of all walls from the records it has
        grouped by pair, and E x 3 integers come back (round 4; rounds 2-3 moved ~20 bytes per wall voxel to the host for
        this); with a wall table already on the host -- or an image that is not C-ordered -- the same arithmetic runs on
        the host over the walls asked for (`geometry.median_voxels`)."""
        from .geometry import gather_segments, median_voxels
        keys = np.asarray(keys, dtype=np.uint64)
        if self._walls is None and getattr(self, "_wall_medians", None) is None:
            self._wall_medians = self._resident().wall_medians() or False
        dev = getattr(self, "_wall_medians", None)
        if dev:
            have, _sizes, med, moving = dev
            at = np.searchsorted(have, keys)
            found = at < have.size
            found[found] = have[at[found]] == keys[found]
            if moving[at[found]].any():        # (raised for a wall that was ASKED for, like the reference: SIA:1630-1633)
                k = int(keys[found][moving[at[found]]][0])
                raise ValueError("Weiszfeld iteration: the wall (%d, %d) is still moving after the last pass" % (k >> 32, k & 0xFFFFFFFF))
            return found, med[at[found]]
        table = self.wall_table()
        at = np.searchsorted(table.pairs, keys)
        found = at < table.pairs.size
        found[found] = table.pairs[at[found]] == keys[found]
        rows, sizes = gather_segments(table.start[at[found]], table.stop[at[found]])
        return found, median_voxels(table.coords[rows].astype(np.int64), sizes).reshape(-1, 3)

    def wall_voxels_between_two_cells(self, label_1, label_2, bbox=None, verbose=False):  # SIA:759-806
        """3xN array of the voxel coordinates of the contact wall between two labels (np.where order)."""
        return self.wall_table().between(label_1, label_2)

    def wall_voxels_per_cell(self, label_1, bbox=None, neighbors=None, neighbors2ignore=[], verbose=False):  # SIA:809-880
        if neighbors is None:
            neighbors = self.neighbors(label_1)
        if isinstance(neighbors, _INT):
            neighbors = [neighbors]
        if isinstance(neighbors, dict) and len(neighbors) != 1:
            neighbors = copy.copy(neighbors[label_1])
        if neighbors2ignore != []:
            for nei in neighbors2ignore:
                try:
                    neighbors.remove(nei)
                except ValueError:
                    pass
        coord = {}
        neighbors_not_found = []
        for label_2 in neighbors:
            xyz = self.wall_table().between(label_1, label_2)
            if xyz.shape[1]:
                coord[min(label_1, label_2), max(label_1, label_2)] = xyz
            else:
                neighbors_not_found.append(label_2)
        if neighbors_not_found:
            print("Some walls have not been found comparing to the `neighbors` list of {}: {}".format(
                label_1, neighbors_not_found))
        return coord

    def wall_voxels_per_cells_pairs(self, labels=None, neighborhood=None, only_epidermis=False,
                                    ignore_background=False, min_contact_area=None, real_area=True,
                                    verbose=True):  # SIA:1049-1111
        # only_epidermis (SIA:1062-1065, 1073-1076): the reference takes the first voxel layer, but then only uses it
        # for the DEFAULT label list (np.unique of that image: 0 = emptied interior, 1 = background, and the labels
        # that touch the background); the walls themselves are still found on the full image (SIA:826, 1108)
        image = self.voxel_first_layer(True) if only_epidermis else None
        compute_neighborhood = neighborhood is None
        if isinstance(labels, list) and isinstance(neighborhood, dict):
            labels = [label for label in labels if label in neighborhood]
        if labels is None and not only_epidermis:
            labels = self.labels()
        elif labels is None and only_epidermis:
            labels = [int(v) for v in np.unique(np.asarray(image))]
        elif isinstance(labels, list):
            labels.sort()
            if not isinstance(neighborhood, dict):
                compute_neighborhood = True
        elif isinstance(labels, _INT):
            labels = [labels]
        else:
            raise ValueError("Couldn't find any labels.")
        dict_wall_voxels = {}
        for label in labels:
            if compute_neighborhood:
                neighbors = self.neighbors(label, min_contact_area, real_area)
            elif isinstance(neighborhood, dict):
                neighbors = copy.copy(neighborhood[label])
            else:
                neighbors = neighborhood
            if ignore_background:
                neighbors2ignore = [n for n in neighbors if n not in labels]
            else:
                neighbors2ignore = [n for n in neighbors if n not in labels + [self.background()]]
            neighbors = [n for n in neighbors if (min(label, n), max(label, n)) not in dict_wall_voxels]
            if neighbors != []:
                dict_wall_voxels.update(self.wall_voxels_per_cell(label, None, neighbors, neighbors2ignore, verbose=False))
        return dict_wall_voxels

    # -- image mutation (SIA:1114-1176): one lookup-table sweep on the GPU instead of per-label crops.
    # The reference leaves its caches (_labels, _bbox, _neighbors ...) stale after these calls; here the
    # relabelled volume is swept again in the same upload, so every later answer describes the new image.
    def _edit_image(self, rv, values, top, relabel):
        """One relabel of the resident volume `rv` (`relabel(rv, table)` -> the Extraction of the new volume) whose new label
        values are `values`, none above `top`; the image is written back when it does not share rv's memory; every cache goes."""
        img = np.asarray(self.image)
        for v in (values.min(), values.max()) if values.size else ():
            if not (0 <= int(v) <= top):
                raise ValueError("value %r does not fit the image dtype %s" % (int(v), img.dtype))
        x = relabel(rv, values)                   # resident volume and rv.host are relabelled; no new upload
        target = img if img.ndim == 3 else img[:, :, None]
        if not np.shares_memory(target, rv.host):          # the image had another dtype / layout: write it back
            np.copyto(target, rv.host.astype(img.dtype), casting="unsafe")
        self._x = x
        self._forget()

    def _relabel_image(self, mapping):
        rv = self._resident_rows()
        top = np.iinfo(rv.host.dtype).max
        lut = self._x.labels_of(np.arange(self._x.nrows)).astype(np.int64)        # one entry per ROW: the row's own id
        for old, new in mapping.items():
            if not (0 <= int(new) <= top):
                raise ValueError("value %r does not fit the image dtype %s" % (new, rv.host.dtype))
            row = self._x.row_of(old)
            if row >= 0:
                lut[row] = int(new)
        self._edit_image(rv, lut, top, lambda rv, table: rv.relabel(table.astype(np.uint32)))

    def fuse_labels_in_image(self, labels, verbose=True):  # SIA:1114-1136
        """Modify the image so the given labels are fused (to the min value)."""
        assert isinstance(labels, list) and len(labels) >= 2
        assert self.background() not in labels
        min_lab = min(labels)
        labels.remove(min_lab)                      # the caller's list loses its minimum, as in the reference
        if verbose:
            print("Fusing the following {} labels: {} to value '{}'.".format(len(labels), labels, min_lab))
        self._relabel_image(dict((l, min_lab) for l in labels))
        return None

    def remove_labels_from_image(self, labels, erase_value=0, verbose=True):  # SIA:1138-1165
        if isinstance(labels, _INT):
            labels = [labels]
        try:
            labels.remove(self.background())
        except ValueError:
            pass
        if verbose:
            print("Removing", len(labels), "cell-labels.")
        self._relabel_image(dict((l, erase_value) for l in labels))
        self._ignoredlabels.update([erase_value])
        for label in labels:
            self._ignoredlabels.discard(label)

    def remove_stack_margin_labels_from_image(self, erase_value=0, voxel_distance_from_margin=5,
                                              verbose=True):  # SIA:1168-1176
        self.remove_labels_from_image(self.labels_at_stack_margins(voxel_distance_from_margin), erase_value, verbose)

    def property_image(self, property_dict, dtype=np.uint16):
        """Image of a per-label property (PropertySpatialImage.create_property_image, PSI:207-221):
        labels without a value, and the background, map to the background id; values are cast with
        ``astype(dtype)`` per label, which is what the reference does per voxel."""
        bg = self.background()
        if bg is None:
            raise ValueError("property_image needs the background label")
        dtype = np.dtype(dtype)
        lut = np.full(self._x.nrows, bg, dtype=np.float64)                        # one entry per ROW of the sweep
        for l, v in property_dict.items():
            row = self._x.row_of(l)
            if row >= 0 and int(l) != bg:
                lut[row] = v
        with np.errstate(invalid="ignore"):
            lut = lut.astype(dtype)
        out = self._resident_rows().map(lut, np.array(bg).astype(dtype))
        if np.asarray(self.image).ndim == 2:
            out = out[:, :, 0]
        return SpatialImage(out, voxelsize=getattr(self.image, "voxelsize", None))


class SpatialImageAnalysis3D(AbstractSpatialImageAnalysis):
    """SIA:1179-1448 (volume, inertia, margins) on top of the same sweep."""

    def __init__(self, image, ignoredlabels=[], return_type=DICT, background=None,
                 device=0, extraction=None):
        AbstractSpatialImageAnalysis.__init__(self, image, ignoredlabels, return_type, background,
                                              device=device, extraction=extraction)
        self._voxel_layer1 = None
        self._voxel_layer18 = None

    def is3D(self):
        return True

    def volume(self, labels=None, real=True):  # SIA:1197-1243
        labels = self.label_request(labels)
        volume = self._x.volumes(labels)
        if real is True:
            volume = np.multiply(volume, self._voxelsize[0] * self._voxelsize[1] * self._voxelsize[2])
        return self.convert_return(volume, labels)

    def inertia_axis(self, labels=None, real=True, verbose=False):  # SIA:1246-1292
        labels = self.label_request(labels)
        vecs, vals = self._x.inertia(labels)
        if real:
            vals = vals * np.linalg.norm(vecs * np.asarray(self._voxelsize, dtype=np.float64), axis=2)
        if len(labels) == 1:
            return return_list_of_vectors(vecs[0]), vals[0]
        if self.return_type == NPLIST:
            return vecs, vals                                           # [n, 3, 3] (rows = axes), [n, 3]
        rows = list(vecs.reshape(-1, 3))                                # return_list_of_vectors for all labels at once
        axes = [rows[k:k + 3] for k in range(0, len(rows), 3)]
        return self.convert_return(axes, labels), self.convert_return(list(vals), labels)

    def reduced_inertia_axis(self, labels=None, real=True, verbose=False):  # SIA:1295-1341
        return self.inertia_axis(labels, real, verbose)

    def labels_at_stack_margins(self, voxel_distance_from_margin=5):  # SIA:1344-1358
        """A label has a voxel within d of a stack face iff its bounding box reaches that far, so
        the six slab scans of the reference reduce to a test on the sweep's bounding boxes."""
        d = int(voxel_distance_from_margin)
        x = self._x
        present = x.present()
        if present.size == 0:
            return []
        if d > 0:    # (image[-0:] is the whole image in the reference's slicing: distance 0 names every label)
            box = x.bbox[x.rows_of(present)]
            shape = np.asarray(x.shape, dtype=np.int64)
            present = present[(box[:, :3] < d).any(axis=1) | (box[:, 3:] > shape - d).any(axis=1)]
        if self._background is not None:
            present = present[present != self._background]
        return present.tolist()

    def region_boundingbox(self, labels):  # SIA:1361-1396
        if isinstance(labels, list) and len(labels) == 1:
            return self.boundingbox(labels[0])
        if isinstance(labels, _INT):
            return self.boundingbox(labels)
        boxes = self._bbox_slices(labels)
        missing = [c for c in labels if c not in boxes or boxes[c] is None]
        if missing:
            warnings.warn("You have asked for unknown cells labels: " + " ".join(str(k) for k in missing))
        known = [c for c in labels if c not in missing]
        starts = [min(boxes[c][d].start for c in known) for d in range(3)]
        stops = [max(boxes[c][d].stop for c in known) for d in range(3)]
        return tuple(slice(a, b) for a, b in zip(starts, stops))


def SpatialImageAnalysis(image, *args, **kwd):
    """Factory of SIA:1663-1680.  File names need openalea's imread, which is out of scope."""
    if isinstance(image, str):
        raise NotImplementedError("reading images from file names needs openalea.image (not part of this path)")
    assert len(image.shape) in [2, 3]
    return SpatialImageAnalysis3D(image, *args, **kwd)
