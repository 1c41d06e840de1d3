"""Per-cell triangle surface meshes, extracted on the GPU (include/tissue_scan_mesh.h, csrc/kernels_mesh.hip).

How this differs from the reference (`PropertySpatialImage.compute_cell_meshes`, `spatial_image_analysis_to_cell_triangular_meshes`):
the reference hands the image to VTK (marching cubes, then smoothing) after subsampling it; here the mesh of a cell is its EXACT
voxel-face surface -- the faces where the label changes, two triangles each, no smoothing -- and subsampling is strided
(`image[::s, ::s, ::s]`, voxel size times s), not interpolated.  The mesh is closed and exact: the volume it encloses is the
cell's voxel count, its faces toward each neighbour are that wall's faces, its centroid is the cell's centre of mass.

Corner K of the meshed image (K in 0 .. ceil(n / s) on each axis) sits at (K - 1/2) * voxelsize * s, in array-axis order, so a
voxel's centre is where `center_of_mass` puts it.  Each cell has a vertex set of its own: a corner two cells share is a vertex
of both (the `coef` shrink of `composed` moves each copy on its own).
"""
from __future__ import annotations

from collections.abc import Mapping

import numpy as np

from . import _capi

OUTSIDE = -1          # the neighbour of a face on the stack border


class CellMeshes(Mapping):
    """The surface meshes of a set of cells, concatenated (the layout of the reference's `composed_triangular_mesh`).

        labels             int64 [C], ascending
        points             float64 [V, 3]: per-cell vertex blocks, vertex_offsets[i] .. vertex_offsets[i + 1] for labels[i]
        triangles          uint32 [T, 3]: GLOBAL vertex indices; triangle_offsets[i] .. triangle_offsets[i + 1] for labels[i];
                           triangles 2k and 2k + 1 of a cell are one voxel face, their normal points out of the cell
        triangle_cell      int64 [T]: the cell of every triangle
        triangle_neighbor  int64 [T]: the label on the other side of its face, OUTSIDE (-1) at the stack border
        vertex_offsets, triangle_offsets   uint64 [C + 1]

    As a Mapping, `meshes[label]` is (points [n, 3], triangles [k, 3] indexing those points), like the reference's
    `cell_meshes` dict."""

    def __init__(self, labels, points, triangles, triangle_cell, triangle_neighbor, vertex_offsets, triangle_offsets,
                 sub_factor=1, ms=None):
        self.labels = np.asarray(labels, dtype=np.int64)
        self.points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        self.triangles = np.asarray(triangles, dtype=np.uint32).reshape(-1, 3)
        self.triangle_cell = np.asarray(triangle_cell, dtype=np.int64)
        self.triangle_neighbor = np.asarray(triangle_neighbor, dtype=np.int64)
        self.vertex_offsets = np.asarray(vertex_offsets, dtype=np.uint64)
        self.triangle_offsets = np.asarray(triangle_offsets, dtype=np.uint64)
        self.sub_factor = int(sub_factor)
        self.ms = ms

    # ------------------------------------------------------------------ Mapping
    def _index(self, label):
        i = int(np.searchsorted(self.labels, int(label)))
        if i >= self.labels.size or self.labels[i] != int(label):
            raise KeyError(label)
        return i

    def __getitem__(self, label):
        i = self._index(label)
        v0, v1 = int(self.vertex_offsets[i]), int(self.vertex_offsets[i + 1])
        t0, t1 = int(self.triangle_offsets[i]), int(self.triangle_offsets[i + 1])
        return self.points[v0:v1], (self.triangles[t0:t1].astype(np.int64) - v0).astype(np.uint32)

    def __iter__(self):
        return iter(self.labels.tolist())

    def __len__(self):
        return int(self.labels.size)

    def __contains__(self, label):
        try:
            self._index(label)
        except (KeyError, TypeError, ValueError):
            return False
        return True

    # ------------------------------------------------------------------ queries
    def wall(self, l1, l2):
        """(points of l1, the triangles of l1 that face l2, indexing those points).  l2 = OUTSIDE (-1): the stack border."""
        i = self._index(l1)
        v0 = int(self.vertex_offsets[i])
        t0, t1 = int(self.triangle_offsets[i]), int(self.triangle_offsets[i + 1])
        keep = self.triangle_neighbor[t0:t1] == int(l2)
        return self.points[v0:int(self.vertex_offsets[i + 1])], (self.triangles[t0:t1][keep].astype(np.int64) - v0).astype(np.uint32)

    def composed(self, coef=1.0):
        """(points, triangles, triangle_cell): every cell's points shrunk by `coef` about the mean of that cell's mesh points,
        as the reference does before it composes the cell meshes (coef = 1: the points as they are)."""
        pts = self.points
        if coef != 1:
            pts = pts.copy()
            for i in range(self.labels.size):
                v0, v1 = int(self.vertex_offsets[i]), int(self.vertex_offsets[i + 1])
                centre = pts[v0:v1].mean(axis=0)
                pts[v0:v1] = centre + coef * (pts[v0:v1] - centre)
        return pts, self.triangles, self.triangle_cell

    def to_ply(self, path, labels=None):
        """Binary little-endian PLY: vertices (double x, y, z = array axes 0, 1, 2), faces with int `label` and `neighbor`
        properties.  `labels`: the cells to write (all by default)."""
        if labels is None:
            pts, tri, cell, nb = self.points, self.triangles, self.triangle_cell, self.triangle_neighbor
        else:
            parts = [self._index(l) for l in sorted(set(int(l) for l in labels))]
            vs, ts, cs, ns, base = [], [], [], [], 0
            for i in parts:
                v0, v1 = int(self.vertex_offsets[i]), int(self.vertex_offsets[i + 1])
                t0, t1 = int(self.triangle_offsets[i]), int(self.triangle_offsets[i + 1])
                vs.append(self.points[v0:v1])
                ts.append(self.triangles[t0:t1].astype(np.int64) - v0 + base)
                cs.append(self.triangle_cell[t0:t1])
                ns.append(self.triangle_neighbor[t0:t1])
                base += v1 - v0
            pts = np.concatenate(vs) if vs else np.zeros((0, 3))
            tri = np.concatenate(ts) if ts else np.zeros((0, 3), dtype=np.int64)
            cell = np.concatenate(cs) if cs else np.zeros(0, dtype=np.int64)
            nb = np.concatenate(ns) if ns else np.zeros(0, dtype=np.int64)
        header = ("ply\nformat binary_little_endian 1.0\ncomment cell surface meshes (exact voxel faces)\n"
                  "element vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                  "element face %d\nproperty list uchar uint vertex_indices\nproperty int label\nproperty int neighbor\n"
                  "end_header\n" % (len(pts), len(tri)))
        face = np.zeros(len(tri), dtype=np.dtype([("n", "u1"), ("v", "<u4", (3,)), ("label", "<i4"), ("neighbor", "<i4")]))
        face["n"] = 3
        face["v"] = tri
        face["label"] = cell
        face["neighbor"] = nb
        with open(path, "wb") as f:
            f.write(header.encode("ascii"))
            f.write(np.ascontiguousarray(pts, dtype="<f8").tobytes())
            f.write(face.tobytes())


def resident_meshes(resident, labels=None, sub_factor=1, voxelsize=(1.0, 1.0, 1.0)):
    """The meshes of `labels` (ids; None = every label, background included) of the volume resident in `resident` (a
    ResidentVolume), on its current extraction -- swept first when the context holds none."""
    ctx = resident.ctx
    s = int(sub_factor)
    if s < 1:
        raise ValueError("sub_factor must be >= 1, not %r" % (sub_factor,))

    def wanted(x):
        if labels is None:
            return None
        rows = x.rows_of(np.asarray(list(labels), dtype=np.int64).reshape(-1), missing=-1)
        w = np.zeros(x.nrows, dtype=np.uint8)
        w[rows[rows >= 0]] = 1
        return w

    x, out = resident.over_extraction(lambda x: ctx.mesh(s, wanted(x)))
    cells, voff, toff, corners, tri, tcell, tnb, ms = out
    ids = (lambda r: r.astype(np.int64)) if x.ids is None else (lambda r: x.ids[r.astype(np.int64)])
    nb = np.full(tnb.shape, OUTSIDE, dtype=np.int64)
    inside = tnb != _capi.MESH_OUTSIDE
    nb[inside] = ids(tnb[inside])
    shape = resident.host.shape
    g = tuple(-(-int(n) // s) + 1 for n in shape)
    K = np.stack(np.unravel_index(corners.astype(np.int64), g), axis=1).astype(np.int64)
    scale = np.asarray(voxelsize, dtype=np.float64) * s
    return CellMeshes(ids(cells), (K - 0.5) * scale, tri, ids(tcell), nb, voff, toff, sub_factor=s, ms=ms)


# ---------------------------------------------------------------------- the reference's module functions
def spatial_image_analysis_to_cell_triangular_meshes(sia, labels=None, sub_factor=1):
    """{label: (points, triangles)} of the cells `labels` of `sia` (its labels() by default) -- a CellMeshes.  Exact voxel-face
    surfaces of image[::sub_factor, ...]; the reference subsamples by 6 and smooths through VTK."""
    return sia.cell_meshes(labels, sub_factor)


def _property(sia, property_name, labels):
    if isinstance(property_name, dict):
        return dict((int(l), property_name[l]) for l in labels if l in property_name)
    if property_name == 'volume':
        values = sia.volume(labels)
    elif property_name == 'neighborhood_size':
        values = sia.neighbors_number(labels)
    else:
        return dict((l, l) for l in labels)       # (the reference's fall-through: the label itself)
    if isinstance(values, dict):
        return values
    return dict(zip(labels, np.asarray(values).tolist()))


def spatial_image_analysis_to_triangular_mesh(sia, property_name=None, labels=None, sub_factor=1):
    """(mesh, matching): `mesh` has `points` [V, 3], `triangles` [T, 3] and `triangle_data` {triangle: value of the property
    of its cell}; `matching` is {triangle: cell}.  property_name: 'volume', 'neighborhood_size', a {label: value} dict, or
    anything else for the label itself (as the reference falls through)."""
    meshes = sia.cell_meshes(labels, sub_factor)
    cells = meshes.labels.tolist()
    prop = _property(sia, property_name, cells)
    matching = dict(enumerate(meshes.triangle_cell.tolist()))
    data = dict((t, prop.get(c)) for t, c in matching.items())
    return TriangularMesh(meshes.points, meshes.triangles, data), matching


class TriangularMesh(object):
    """points [V, 3], triangles [T, 3] and triangle_data {triangle: value}: what `composed_triangular_mesh` returns."""

    def __init__(self, points, triangles, triangle_data=None):
        self.points = points
        self.triangles = triangles
        self.triangle_data = {} if triangle_data is None else triangle_data
