"""NumPy restatement of the cell-mesh contract of include/tissue_scan_mesh.h, written from the definition (not from the kernels).

    W = V[::s, ::s, ::s]; a boundary face of cell c is a face of a voxel p with W[p] = c whose neighbour q = p +- e_a is outside W
    (neighbour OUTSIDE = -1) or holds another label.  Two triangles per face, normal from p to q; per cell, the vertices are the
    distinct corners of its faces.  Order: cells ascending; vertices by C-order index of the corner; faces by C-order index of p,
    then direction -0, +0, -1, +1, -2, +2.
"""
import numpy as np

OUTSIDE = -1


def mesh(V, labels=None, sub_factor=1, voxelsize=(1.0, 1.0, 1.0)):
    """dict of labels, points (float64 [V, 3]), corners (int64 [V, 3]), triangles (uint32 [T, 3], global), triangle_cell,
    triangle_neighbor (int64 [T]), vertex_offsets, triangle_offsets (uint64 [C + 1]).  labels=None: every label, background
    included."""
    V = np.asarray(V)
    if V.ndim == 2:
        V = V[:, :, None]
    s = int(sub_factor)
    W = V[::s, ::s, ::s].astype(np.int64)
    m = np.array(W.shape, dtype=np.int64)
    present = np.unique(W)
    cells = present if labels is None else np.intersect1d(present, np.asarray(list(labels), dtype=np.int64))
    P = np.pad(W, 1, constant_values=OUTSIDE)

    # faces: (cell, voxel index, direction, neighbour)
    vox = np.arange(W.size, dtype=np.int64).reshape(W.shape)
    wanted = np.isin(W, cells)
    fc, fv, fd, fn = [], [], [], []
    for d in range(6):
        a, step = d // 2, (1 if d % 2 else -1)
        sl = [slice(1, 1 + int(m[k])) for k in range(3)]
        sl[a] = slice(1 + step, 1 + step + int(m[a]))
        nb = P[tuple(sl)]
        hit = wanted & (nb != W)
        fc.append(W[hit]); fv.append(vox[hit]); fd.append(np.full(int(hit.sum()), d, dtype=np.int64)); fn.append(nb[hit])
    fc, fv, fd, fn = (np.concatenate(x) for x in (fc, fv, fd, fn))
    order = np.lexsort((fd, fv, fc))
    fc, fv, fd, fn = fc[order], fv[order], fd[order], fn[order]

    # vertices: (cell, corner) where the cell holds some but not all of the eight voxels around the corner
    g = m + 1
    around = np.stack([P[i:i + int(g[0]), j:j + int(g[1]), k:k + int(g[2])].reshape(-1)
                       for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    uniform = (around == around[0]).all(axis=0)
    vc, vk = [], []
    for d in range(8):
        first = np.ones(around.shape[1], dtype=bool)
        for e in range(d):
            first &= around[e] != around[d]
        hit = first & ~uniform & np.isin(around[d], cells)
        vc.append(around[d][hit]); vk.append(np.flatnonzero(hit).astype(np.int64))
    vc, vk = np.concatenate(vc), np.concatenate(vk)
    order = np.lexsort((vk, vc))
    vc, vk = vc[order], vk[order]

    # triangles
    rank = np.searchsorted(cells, fc)
    vkey = np.searchsorted(cells, vc) * int(g.prod()) + vk
    p = np.stack(np.unravel_index(fv, W.shape), axis=1)
    a = fd // 2
    plus = fd % 2
    K0 = p.copy()
    K0[np.arange(len(a)), a] += plus
    eb = np.eye(3, dtype=np.int64)[(a + 1) % 3]
    ed = np.eye(3, dtype=np.int64)[(a + 2) % 3]
    quad = [K0, K0 + eb, K0 + eb + ed, K0 + ed]

    def index(K):
        key = rank * int(g.prod()) + np.ravel_multi_index(tuple(K.T), tuple(g))
        at = np.searchsorted(vkey, key)
        assert (vkey[at] == key).all()
        return at

    v0, v1, v2, v3 = (index(K) for K in quad)
    tri = np.empty((2 * len(fc), 3), dtype=np.int64)
    pos = plus == 1
    tri[0::2] = np.where(pos[:, None], np.stack([v0, v1, v2], 1), np.stack([v0, v2, v1], 1))
    tri[1::2] = np.where(pos[:, None], np.stack([v0, v2, v3], 1), np.stack([v0, v3, v2], 1))
    corners = np.stack(np.unravel_index(vk, tuple(g)), axis=1).astype(np.int64)
    scale = np.asarray(voxelsize, dtype=np.float64) * s
    return dict(labels=cells.astype(np.int64),
                corners=corners,
                points=(corners - 0.5) * scale,
                triangles=tri.astype(np.uint32),
                triangle_cell=np.repeat(fc, 2),
                triangle_neighbor=np.repeat(fn, 2),
                vertex_offsets=np.append(np.searchsorted(vc, cells), len(vc)).astype(np.uint64),
                triangle_offsets=np.append(2 * np.searchsorted(fc, cells), 2 * len(fc)).astype(np.uint64),
                face_direction=fd)


def six_volume(corners, triangles):
    """Six times the signed volume a closed triangle set encloses, exactly (int64 determinants of corner coordinates)."""
    a, b, c = (corners[triangles[:, i].astype(np.int64)] for i in range(3))
    return int(np.einsum("ij,ij->i", a, np.cross(b, c)).sum())
