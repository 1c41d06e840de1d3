"""NumPy restatement of the wall-geometry rows (include/tissue_scan_wallgeo.h), independent of the product code.

A face is a pair of voxels p, q = p + e_d of different labels; its pair is (lo, hi) = (min, max) of the two labels, its position
c = p + q (doubled voxel-centre coordinates, array axes, axis 0 global).  Rows, sorted by lo << 32 | hi: fwd[d] faces of axis d
with V[p] == lo, rev[d] with V[p] == hi, sum1 = sum of c, sum2 = sum of c_x c_y for xx, xy, xz, yy, yz, zz.  All uint64; the
accumulation is np.add.at on uint64 (a float bincount is inexact above 2^53)."""
import numpy as np

PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def _as3d(V):
    V = np.asarray(V)
    return V[:, :, None] if V.ndim == 2 else V


def _empty():
    z = lambda w: np.zeros((0, w), dtype=np.uint64)
    return dict(lo=np.zeros(0, dtype=np.int64), hi=np.zeros(0, dtype=np.int64), fwd=z(3), rev=z(3), sum1=z(3), sum2=z(6))


def rows(V, first_owned=0, a0_origin=0):
    """dict(lo, hi int64 [P]; fwd, rev, sum1 uint64 [P, 3]; sum2 uint64 [P, 6]) of the label image V (2-D or 3-D, any layout).

    first_owned = 1: plane 0 of V is the low halo of a slab whose first owned plane has the global coordinate a0_origin along
    axis 0.  A face belongs to the slab of its higher voxel: the halo plane gives only its faces with plane 1, and no face
    inside it."""
    V = _as3d(V)
    keys, axes, revs, cs = [], [], [], []
    for d in range(3):
        if V.shape[d] < 2:
            continue
        low = [slice(None)] * 3
        high = [slice(None)] * 3
        low[d], high[d] = slice(0, V.shape[d] - 1), slice(1, V.shape[d])
        a, b = V[tuple(low)], V[tuple(high)]                        # a = V[p], b = V[p + e_d]
        face = a != b
        if first_owned and d != 0:
            face[0] = False                                         # faces inside the halo plane belong to the slab below
        p = np.stack(np.nonzero(face), axis=-1).astype(np.int64)    # p, in the buffer's coordinates
        if not p.shape[0]:
            continue
        va, vb = a[face].astype(np.uint64), b[face].astype(np.uint64)
        c = 2 * p
        c[:, d] += 1
        c[:, 0] += 2 * (int(a0_origin) - int(first_owned))
        keys.append((np.minimum(va, vb) << np.uint64(32)) | np.maximum(va, vb))
        axes.append(np.full(p.shape[0], d, dtype=np.int64))
        revs.append(va > vb)
        cs.append(c.astype(np.uint64))
    if not keys:
        return _empty()
    keys, axes, revs, cs = np.concatenate(keys), np.concatenate(axes), np.concatenate(revs), np.concatenate(cs)
    uniq, inv = np.unique(keys, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    P = uniq.size
    fwd, rev = np.zeros((P, 3), dtype=np.uint64), np.zeros((P, 3), dtype=np.uint64)
    np.add.at(fwd, (inv[~revs], axes[~revs]), np.uint64(1))
    np.add.at(rev, (inv[revs], axes[revs]), np.uint64(1))
    sum1, sum2 = np.zeros((P, 3), dtype=np.uint64), np.zeros((P, 6), dtype=np.uint64)
    np.add.at(sum1, inv, cs)
    np.add.at(sum2, inv, np.stack([cs[:, x] * cs[:, y] for x, y in PAIRS], axis=1))
    return dict(lo=(uniq >> np.uint64(32)).astype(np.int64), hi=(uniq & np.uint64(0xFFFFFFFF)).astype(np.int64),
                fwd=fwd, rev=rev, sum1=sum1, sum2=sum2)


def merge(parts):
    """Rows of the slabs of one volume as one: every field added over equal pairs."""
    keys = np.concatenate([(p["lo"].astype(np.uint64) << np.uint64(32)) | p["hi"].astype(np.uint64) for p in parts])
    if not keys.size:
        return _empty()
    uniq, inv = np.unique(keys, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    out = dict(lo=(uniq >> np.uint64(32)).astype(np.int64), hi=(uniq & np.uint64(0xFFFFFFFF)).astype(np.int64))
    for name, width in (("fwd", 3), ("rev", 3), ("sum1", 3), ("sum2", 6)):
        t = np.zeros((uniq.size, width), dtype=np.uint64)
        np.add.at(t, inv, np.concatenate([p[name] for p in parts]).reshape(-1, width))
        out[name] = t
    return out
