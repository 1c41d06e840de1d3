"""The topology of every cell: Euler numbers for 6- and for 26-connectivity, and the intrinsic volumes of the voxel solid (mean
breadth, half its surface), from the twelve exact block counts of the Euler-number pass (include/tissue_scan_topology.h,
csrc/kernels_topology.hip).  The integers stay in the memory-axis order of the pass; the axis permutation of an image that is not
C-ordered, the voxel size and every float (float64) are the host's work, here."""
from __future__ import annotations

import numpy as np

from ._tables import _ByLabel, to_array_axes, voxelsize3

COLUMNS = ("euler_number", "mean_breadth", "half_surface")


class CellTopology(_ByLabel):
    """Block counts whose rows line up with an `Extraction`: rows 0..max_label, or one per id of `.ids` when the ids are sparse.
    Twelve int64 columns as the pass gives them; the per-axis ones in MEMORY-axis order k = 0, 1, 2 (`perm[k]` is the array axis
    of k):

        n0         voxels (the extraction's count)
        n1 [R, 3]  same-label face pairs along axis k
        n2 [R, 3]  2 x 2 squares of the label normal to axis k
        n3         2 x 2 x 2 cubes of the label
        v          lattice vertices the label touches
        e  [R, 3]  lattice edges along axis k the label touches

    and what follows from them, in exact integers until a voxel size comes in:

        faces()               F_k = 2 n0 - n1[k], lattice faces normal to ARRAY axis k the label touches, the image border included
        euler_number(6)       n0 - sum n1 + sum n2 - n3: the voxels joined across faces only
        euler_number(26)      v - sum e + sum F - n0: the closed voxel solid
        intrinsic_volumes()   (chi26, V1, V2, volume); mean_breadth() = V1 / 2
    """

    def __init__(self, extraction, n0, n1, n2, n3, v, e, perm=(0, 1, 2), voxelsize=(1.0, 1.0, 1.0), ms=None):
        self.extraction = extraction
        self.ids = None if extraction is None else extraction.ids
        one = lambda a: np.asarray(a).astype(np.int64).reshape(-1)
        three = lambda a: np.asarray(a).astype(np.int64).reshape(-1, 3)
        self.n0, self.n3, self.v = one(n0), one(n3), one(v)
        self.n1, self.n2, self.e = three(n1), three(n2), three(e)
        R = self.n0.size
        if any(a.shape[0] != R for a in (self.n1, self.n2, self.n3, self.v, self.e)):
            raise ValueError("the twelve columns must have one row per label")
        self.perm = tuple(int(p) for p in perm)
        if sorted(self.perm) != [0, 1, 2]:
            raise ValueError("perm must be a permutation of (0, 1, 2), not %r" % (perm,))
        self.voxelsize = voxelsize3(voxelsize)
        self.ms = ms

    def __len__(self):
        return int(self.n0.size)

    # ------------------------------------------------------------------ exact integers
    def _faces_memory(self):
        return 2 * self.n0[:, None] - self.n1

    def faces(self):
        """int64 [R, 3]: the lattice faces normal to each ARRAY axis that every label touches, each counted once: 2 n0 - n1."""
        return to_array_axes(self._faces_memory(), self.perm)

    def face_pairs(self):
        """int64 [R, 3]: n1 in ARRAY-axis order."""
        return to_array_axes(self.n1, self.perm)

    def euler_number(self, connectivity=6):
        """int64 [R]: the Euler number of every row's voxels, joined across faces (6) or across faces, edges and corners (26)."""
        if connectivity == 6:
            return self.n0 - self.n1.sum(axis=1) + self.n2.sum(axis=1) - self.n3
        if connectivity == 26:
            return self.v - self.e.sum(axis=1) + self._faces_memory().sum(axis=1) - self.n0
        raise ValueError("connectivity must be 6 or 26, not %r" % (connectivity,))

    # ------------------------------------------------------------------ floats
    def intrinsic_volumes(self, voxelsize=None):
        """(chi26 int64 [R], V1, V2, volume float64 [R]) of the closed voxel solid of every row, with `voxelsize` per ARRAY axis
        (default: this object's).  V1 is twice the mean breadth -- a box of a x b x c voxels gives a s0 + b s1 + c s2 --, V2 half
        the surface, the faces on the image border included."""
        vs = self.voxelsize if voxelsize is None else voxelsize3(voxelsize)
        s = [vs[self.perm[k]] for k in range(3)]                  # per memory axis
        area = [s[1] * s[2], s[0] * s[2], s[0] * s[1]]
        F = self._faces_memory()
        v1 = np.zeros(len(self), dtype=np.float64)
        v2 = np.zeros(len(self), dtype=np.float64)
        for a in range(3):
            others = F.sum(axis=1) - F[:, a]
            v1 += s[a] * (self.e[:, a] - others + self.n0).astype(np.float64)
            v2 += area[a] * (F[:, a] - self.n0).astype(np.float64)
        return self.euler_number(26), v1, v2, self.n0.astype(np.float64) * (s[0] * s[1] * s[2])

    def mean_breadth(self, voxelsize=None):
        """float64 [R]: V1 / 2 of `intrinsic_volumes`."""
        return 0.5 * self.intrinsic_volumes(voxelsize)[1]

    # ------------------------------------------------------------------ lookups by label id
    def of_labels(self, labels, column="euler_number", connectivity=6, voxelsize=None):
        """`column` of every label id in `labels`: 'euler_number' (int64, for `connectivity`), 'mean_breadth' or 'half_surface'
        (float64, with `voxelsize`).  An id without a row has no voxels: 0, as for a row without voxels."""
        if column not in COLUMNS:
            raise ValueError("column must be one of %s, not %r" % ("|".join(COLUMNS), column))
        if column == "euler_number":
            col = self.euler_number(connectivity)
        else:
            col = self.intrinsic_volumes(voxelsize)[1 if column == "mean_breadth" else 2]
            if column == "mean_breadth":
                col = 0.5 * col
        return self._pick(col, labels, 0)


def topological_defects(topology, components, exclude=()):
    """{label: {'blobs': b0, 'euler': chi6, 'tunnels_minus_cavities': b0 - chi6}} of the labels whose face-connected Euler number
    is not their number of face-connected blobs -- the labels that are not unions of balls --, without those in `exclude`.
    topology: a CellTopology; components: a LabelComponents of the same image (`per_label()` is {label: blobs})."""
    out = set(int(l) for l in exclude)
    blobs = components.per_label()
    labels = sorted(l for l in blobs if l not in out)
    chi = topology.of_labels(labels, "euler_number", 6)
    found = {}
    for l, x in zip(labels, chi.tolist()):
        if x != blobs[l]:
            found[l] = {'blobs': int(blobs[l]), 'euler': int(x), 'tunnels_minus_cavities': int(blobs[l]) - int(x)}
    return found


def resident_topology(resident, voxelsize=(1.0, 1.0, 1.0)):
    """The Euler-number pass over the volume resident in `resident` (a ResidentVolume), with the rows of its current extraction --
    swept first when the context holds none that fits."""
    ctx = resident.ctx
    x, _ = resident.over_extraction(lambda x: ctx.topology_extract())
    n0, n1, n2, n3, v, e = ctx.topology_rows()
    return CellTopology(x, n0, n1, n2, n3, v, e, ctx.memory_axes(), voxelsize, ms=ctx.topology_timing())
