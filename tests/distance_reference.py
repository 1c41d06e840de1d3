"""References for the distance maps (include/tissue_scan_distance.h), host only.

Two of them, which share nothing with the kernels and nothing with each other:

  brute_d2   every pair of voxels.  For power-of-two spacings in exact integer arithmetic (the spacings are scaled to integers, the
             result divided by a power of two: no rounding anywhere); for other spacings in float64, ((a0 + a1) + a2).  For volumes
             of about 2 000 voxels at most: the pair matrix is N x N.
  scipy_d2   per label crop (mode 0) or for the site class (mode 1) scipy.ndimage.distance_transform_edt(mask, sampling,
             return_indices=True), and D2 recomputed from the returned indices as sum (spacing * delta)^2: squaring the returned
             distance would lose the last bit, since it is a rounded square root.

EDGE_IS_SITE is the same transform of the image padded by one voxel that is a site for every voxel.  table() is plain NumPy
reductions over an image of D2."""
import math

import numpy as np
from scipy import ndimage

OWN_WALL, FROM_LABEL = 0, 1


def is_dyadic(spacing):
    return all(math.frexp(float(s))[0] == 0.5 for s in spacing)


def _padded(V, edge):
    """(labels, pad mask), one voxel larger on every side when `edge`."""
    V = np.asarray(V)
    if not edge:
        return V, np.zeros(V.shape, dtype=bool)
    lab = np.pad(V, 1, mode="constant", constant_values=0)
    pad = np.ones(lab.shape, dtype=bool)
    pad[1:-1, 1:-1, 1:-1] = False
    return lab, pad


def brute_d2(V, spacing=(1.0, 1.0, 1.0), mode=OWN_WALL, site=None, edge=False):
    V = np.asarray(V)
    lab, pad = _padded(V, edge)
    coords = np.stack(np.meshgrid(*[np.arange(n) for n in lab.shape], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    assert len(coords) <= 4096, "the pair matrix is N x N"
    lab_f, pad_f = lab.reshape(-1).astype(np.int64), pad.reshape(-1)
    if mode == OWN_WALL:
        sites = (lab_f[None, :] != lab_f[:, None]) | pad_f[None, :]
    else:
        sites = np.broadcast_to(((lab_f == int(site)) & ~pad_f) | pad_f, (len(lab_f), len(lab_f)))
    delta = coords[:, None, :] - coords[None, :, :]
    if is_dyadic(spacing):
        ratios = [float(s).as_integer_ratio() for s in spacing]
        den = max(d for _, d in ratios)
        w = np.array([n * (den // d) for n, d in ratios], dtype=np.int64)
        pair = ((delta * w) ** 2).sum(axis=-1)
        assert int(pair.max()) < 2 ** 53
        big = np.iinfo(np.int64).max
        best = np.where(sites, pair, big).min(axis=1)
        out = np.where(best == big, np.inf, best.astype(np.float64) / float(den * den))
    else:
        t = (delta.astype(np.float64) * np.asarray(spacing, dtype=np.float64)) ** 2
        pair = (t[..., 0] + t[..., 1]) + t[..., 2]
        out = np.where(sites, pair, np.inf).min(axis=1)
    out = out.reshape(lab.shape)
    return out[1:-1, 1:-1, 1:-1].copy() if edge else out


def _edt_d2(inside, spacing):
    """D2 of every voxel of the boolean image to the nearest voxel where it is False, from the indices scipy returns; +inf when there
    is no such voxel."""
    if inside.all():
        return np.full(inside.shape, np.inf)
    idx = ndimage.distance_transform_edt(inside, sampling=spacing, return_distances=False, return_indices=True)
    own = np.indices(inside.shape)
    t = [(float(spacing[a]) * (own[a] - idx[a]).astype(np.float64)) ** 2 for a in range(3)]
    return (t[0] + t[1]) + t[2]


def scipy_d2(V, spacing=(1.0, 1.0, 1.0), mode=OWN_WALL, site=None, edge=False):
    V = np.asarray(V)
    lab, pad = _padded(V, edge)
    if mode == OWN_WALL:
        # per label, on its bounding box grown by one voxel: the nearest voxel of another label lies inside it (clamping a site
        # into that box brings it no further away along any axis, and the layer around the bounding box holds no voxel of the label)
        out = np.zeros(lab.shape, dtype=np.float64)
        ids, rank = np.unique(lab, return_inverse=True)
        rank = np.where(pad, 0, np.asarray(rank).reshape(lab.shape) + 1)
        for k, box in enumerate(ndimage.find_objects(rank), start=1):
            if box is None:
                continue
            box = tuple(slice(max(s.start - 1, 0), min(s.stop + 1, n)) for s, n in zip(box, lab.shape))
            inside = rank[box] == k
            out[box][inside] = _edt_d2(inside, spacing)[inside]
    else:
        out = _edt_d2(~(((lab == int(site)) & ~pad) | pad), spacing)
    return out[1:-1, 1:-1, 1:-1].copy() if edge else out


def table(V, d2, rows):
    """(min2 f64[rows], max2 f64[rows], pole i32[rows, 3]) of the labels 0 .. rows - 1: absent ones read inf, inf, (-1, -1, -1)."""
    V = np.asarray(V)
    min2, max2 = np.full(rows, np.inf), np.full(rows, np.inf)
    pole = np.full((rows, 3), -1, dtype=np.int32)
    for l in np.unique(V):
        where = np.argwhere(V == l)                      # C order of the array axes, whatever the memory layout
        vals = d2[tuple(where.T)]
        min2[l], max2[l] = vals.min(), vals.max()
        pole[l] = where[int(np.argmax(vals == vals.max()))]
    return min2, max2, pole


def table_by_id(V, d2):
    """The same keyed by the ids present, ascending: (ids, min2, max2, pole)."""
    ids = np.unique(V)
    rank = np.searchsorted(ids, V)
    return (ids,) + table(rank, d2, len(ids))
