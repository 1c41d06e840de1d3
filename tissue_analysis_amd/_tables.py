"""What the per-label and per-wall tables of the feature modules have in common on the host: what a voxel size is, how label ids
find their rows, and how per-axis columns get from memory-axis to array-axis order."""
from __future__ import annotations

import numpy as np


def voxelsize3(v):
    """Three floats from a voxel size of two (a 2-D image: 1.0 is appended) or three entries."""
    vs = tuple(float(x) for x in v)
    if len(vs) == 2:
        vs = vs + (1.0,)
    if len(vs) != 3:
        raise ValueError("voxelsize must have two or three entries")
    return vs


def to_array_axes(mem, perm):
    """Columns of a [R, 3] array from memory-axis to array-axis order: perm[k] is the array axis of memory axis k."""
    out = np.empty_like(mem)
    for k in range(3):
        out[:, perm[k]] = mem[:, k]
    return out


class _ByLabel(object):
    """Rows that line up with an `Extraction` (`self.extraction`): rows 0..max_label, or one per id of `.ids` when the ids are
    sparse.  Without an extraction (rows merged from slabs) the rows are the label ids, len(self) of them."""

    def rows_of(self, labels, missing=None):
        if self.extraction is None:
            idx = np.asarray(labels, dtype=np.int64)
            return idx if missing is None else np.where((idx >= 0) & (idx < len(self)), idx, missing)
        return self.extraction.rows_of(labels, missing)

    def _pick(self, table, labels, fill):
        """table[row] of every label id in `labels`, `fill` for an id without a row."""
        rows = self.rows_of(np.asarray(labels, dtype=np.int64).reshape(-1), missing=-1)
        known = rows >= 0
        out = table[np.where(known, rows, 0)].copy()
        out[~known] = fill
        return out
