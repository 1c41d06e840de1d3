"""References for the nearest-label maps (include/tissue_scan_nearest.h), host only.

Three of them, which share nothing with the kernels and no arithmetic with each other:

  brute_sites   every voxel against every site, a few planes at a time: its cost grows with the sites, not with the square of the
                voxels, so it reaches the volumes that cross the launch caps.  Power-of-two spacings only, in exact integers; beside
                N and D2 it returns `ways`, the number of distinct labels at exactly the minimal distance.
  brute         every pair of voxels. For power-of-two spacings in exact integer arithmetic (the spacings are scaled to integers, the
                result divided by a power of two: no rounding anywhere); for other spacings in float64, ((a0 + a1) + a2).  N is the
                smallest label among the sites at exactly the minimal distance.  At most 4096 voxels: the pair matrix is N x N.
  by_label_edt  at any size.  For every site label l in ascending order D2_l from scipy.ndimage.distance_transform_edt(V != l,
                sampling, return_indices=True), recomputed from the returned indices as sum (spacing * delta)^2 (squaring the returned
                distance would lose the last bit); then N = ids[argmin over l] -- argmin returns the first minimum, which is the
                smallest label -- and D2 = min over l.

All begin their answer with (N uint32, D2 float64) with the shape of V; N is NONE and D2 +inf where there is no site.  filled() and
result() apply the definitions of "filled" on top of them."""
import math

import numpy as np
from scipy import ndimage

NONE = 0xFFFFFFFF


def is_dyadic(spacing):
    return all(math.frexp(float(s))[0] == 0.5 for s in spacing)


def site_mask(V, empty, not_from=None):
    V = np.asarray(V)
    sites = V != empty
    if not_from is not None:
        sites &= V != not_from
    return sites


def brute(V, empty=0, spacing=(1.0, 1.0, 1.0), not_from=None, ties=False):
    """(N, D2), and with `ties` a bool image too: the voxel has sites of two labels or more at exactly its minimal distance."""
    V = np.asarray(V)
    assert V.size <= 4096, "the pair matrix is N x N"
    coords = np.stack(np.meshgrid(*[np.arange(n) for n in V.shape], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    sites = site_mask(V, empty, not_from).reshape(-1)
    if not sites.any():
        out = np.full(V.shape, NONE, dtype=np.uint32), np.full(V.shape, np.inf)
        return out + (np.zeros(V.shape, dtype=bool),) if ties else out
    labels = V.reshape(-1)[sites].astype(np.int64)
    delta = coords[:, None, :] - coords[sites][None, :, :]
    if is_dyadic(spacing):
        ratios = [float(s).as_integer_ratio() for s in spacing]
        den = max(d for _, d in ratios)
        w = np.array([n * (den // d) for n, d in ratios], dtype=np.int64)
        pair = ((delta * w) ** 2).sum(axis=-1)
        assert int(pair.max()) < 2 ** 53
        best = pair.min(axis=1)
        d2 = best.astype(np.float64) / float(den * den)
    else:
        t = (delta.astype(np.float64) * np.asarray(spacing, dtype=np.float64)) ** 2
        pair = (t[..., 0] + t[..., 1]) + t[..., 2]
        best = pair.min(axis=1)
        d2 = best
    at_best = pair == best[:, None]
    nearest = np.where(at_best, labels[None, :], np.int64(NONE)).min(axis=1)
    out = nearest.astype(np.uint32).reshape(V.shape), d2.reshape(V.shape)
    if ties:
        out += ((np.where(at_best, labels[None, :], -1).max(axis=1) != nearest).reshape(V.shape),)
    return out


def brute_sites(V, empty=0, spacing=(1.0, 1.0, 1.0), not_from=None, budget=1 << 22):
    """(N, D2, ways) at any size with few sites: every voxel against every site, whole planes of axis 0 at a time so that no array
    has more than about `budget` elements.  Power-of-two spacings only, in the exact integers of brute().  ways (int32) is the number
    of distinct labels among the sites at exactly the minimal distance, 0 where there is no site."""
    V = np.asarray(V)
    assert V.ndim == 3 and is_dyadic(spacing), "exact integers need power-of-two spacings"
    ratios = [float(s).as_integer_ratio() for s in spacing]
    den = max(d for _, d in ratios)
    w = [n * (den // d) for n, d in ratios]
    assert sum((w[a] * V.shape[a]) ** 2 for a in range(3)) < 2 ** 53
    where = np.argwhere(site_mask(V, empty, not_from))
    if where.shape[0] == 0:
        return np.full(V.shape, NONE, dtype=np.uint32), np.full(V.shape, np.inf), np.zeros(V.shape, dtype=np.int32)
    labels = V[tuple(where.T)].astype(np.int64)
    order = np.argsort(labels, kind="stable")
    where, labels = where[order], labels[order]          # ascending labels: the first site at the minimum has the smallest label
    groups = np.flatnonzero(np.r_[True, labels[1:] != labels[:-1]])
    along = [(w[a] * (np.arange(V.shape[a], dtype=np.int64)[None, :] - where[:, a, None])) ** 2 for a in range(3)]      # [site][position]
    N = np.empty(V.shape, dtype=np.uint32)
    D2 = np.empty(V.shape, dtype=np.float64)
    ways = np.empty(V.shape, dtype=np.int32)
    planes = max(1, budget // (labels.size * V.shape[1] * V.shape[2]))
    for q in range(0, V.shape[0], planes):
        d = along[0][:, q:q + planes, None, None] + along[1][:, None, :, None] + along[2][:, None, None, :]
        best = d.min(axis=0)
        at_best = d == best[None]
        N[q:q + planes] = labels[at_best.argmax(axis=0)]
        D2[q:q + planes] = best.astype(np.float64) / float(den * den)
        ways[q:q + planes] = at_best.sum(axis=0) if groups.size == labels.size else np.logical_or.reduceat(at_best, groups, axis=0).sum(axis=0)
    return N, D2, ways


def label_d2(V, label, spacing):
    """D2 of every voxel to the nearest voxel of `label`, from the indices scipy returns."""
    V = np.asarray(V)
    idx = ndimage.distance_transform_edt(V != label, sampling=spacing, return_distances=False, return_indices=True)
    own = np.indices(V.shape)
    t = [(float(spacing[a]) * (own[a] - idx[a]).astype(np.float64)) ** 2 for a in range(3)]
    return (t[0] + t[1]) + t[2]


def by_label_edt(V, empty=0, spacing=(1.0, 1.0, 1.0), not_from=None, per_label=False):
    V = np.asarray(V)
    ids = np.unique(V[site_mask(V, empty, not_from)])
    if ids.size == 0:
        out = np.full(V.shape, NONE, dtype=np.uint32), np.full(V.shape, np.inf)
        return out + ((ids, np.zeros((0,) + V.shape)),) if per_label else out
    stack = np.stack([label_d2(V, l, spacing) for l in ids])
    first = np.argmin(stack, axis=0)
    out = ids[first].astype(np.uint32), stack.min(axis=0)
    return out + ((ids, stack),) if per_label else out


def filled(V, d2, empty=0, max_d2=np.inf):
    """bool image of the voxels that are filled."""
    return (np.asarray(V) == empty) & np.isfinite(d2) & (d2 <= max_d2)


def result(V, nearest, d2, empty=0, max_d2=np.inf, rows=None):
    """(image after the fill, gained int64[rows] by label, filled voxels, empty voxels left)."""
    V = np.asarray(V)
    f = filled(V, d2, empty, max_d2)
    image = np.where(f, nearest, V).astype(V.dtype)
    if rows is None:
        rows = int(V.max()) + 1
    gained = np.bincount(nearest[f].astype(np.int64), minlength=rows).astype(np.int64)
    return image, gained, int(f.sum()), int((V == empty).sum() - f.sum())
