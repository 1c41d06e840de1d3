"""NumPy restatement of include/tissue_scan_overlap.h and of what tissue_analysis_amd.label_overlap derives from the table: the
overlap table of two label volumes (np.unique on a << 32 | b with counts), its margins, the Jaccard index, best matches with
the tie rule, lineage, and the merge of slab tables.  Written independently of the package (plain loops where the package is
vectorised), so that the two can be compared."""
import numpy as np


def table(A, B, first_owned=0):
    """(a int64[P], b int64[P], n uint64[P]) sorted by (a, b): n voxels with label a in A and b in B.  first_owned = 1: plane 0
    along axis 0 is a slab's low halo and adds nothing."""
    A, B = np.asarray(A), np.asarray(B)
    assert A.shape == B.shape
    A, B = A[first_owned:], B[first_owned:]
    keys = (A.astype(np.uint64).reshape(-1) << np.uint64(32)) | B.astype(np.uint64).reshape(-1)
    u, c = np.unique(keys, return_counts=True)
    return (u >> np.uint64(32)).astype(np.int64), (u & np.uint64(0xFFFFFFFF)).astype(np.int64), c.astype(np.uint64)


def merge(tables):
    """The tables of the slabs of a volume, summed over equal (a, b)."""
    tot = {}
    for a, b, n in tables:
        for x, y, c in zip(a.tolist(), b.tolist(), n.tolist()):
            tot[(x, y)] = tot.get((x, y), 0) + c
    keys = sorted(tot)
    return (np.array([k[0] for k in keys], dtype=np.int64), np.array([k[1] for k in keys], dtype=np.int64),
            np.array([tot[k] for k in keys], dtype=np.uint64))


def margins(a, b, n):
    """({label of A: voxels}, {label of B: voxels})."""
    sa, sb = {}, {}
    for x, y, c in zip(a.tolist(), b.tolist(), n.tolist()):
        sa[x] = sa.get(x, 0) + c
        sb[y] = sb.get(y, 0) + c
    return sa, sb


def jaccard(a, b, n):
    sa, sb = margins(a, b, n)
    return np.array([float(c) / float(sa[x] + sb[y] - c) for x, y, c in zip(a.tolist(), b.tolist(), n.tolist())], dtype=np.float64)


def best_match(a, b, n, side="b", exclude=()):
    """{label of `side`: (partner, n)}: the partner with the largest n, ties to the smallest partner id, partners in `exclude`
    never chosen (a label whose partners are all excluded is absent)."""
    exclude = set(int(e) for e in exclude)
    best = {}
    for x, y, c in zip(a.tolist(), b.tolist(), n.tolist()):
        own, other = (x, y) if side == "a" else (y, x)
        if other in exclude:
            continue
        cur = best.get(own)
        if cur is None or c > cur[1] or (c == cur[1] and other < cur[0]):
            best[own] = (other, c)
    return best


def lineage(a, b, n, min_fraction=0.5, exclude=(0,)):
    """{mother: [daughters ascending]}."""
    exclude = set(int(e) for e in exclude)
    _, sb = margins(a, b, n)
    out = {}
    for d, (m, c) in best_match(a, b, n, "b", exclude).items():
        if d in exclude:
            continue
        if float(c) >= float(min_fraction) * float(sb[d]):
            out.setdefault(m, []).append(d)
    return dict((m, sorted(ds)) for m, ds in out.items())


def division_fixture(dims=(96, 96, 96), n_cells=200, seed=5, rng_seed=1, offset=1000):
    """Frame A = a Voronoi tissue; frame B = the same with about half of the cells cut by a random plane through their
    barycentre, one side renamed label + offset.  Returns (A uint16, B uint32, {label of B: its mother in A})."""
    from tissue_analysis_amd import synth
    A = synth.voronoi_labels(dims, n_cells, seed, dtype=np.uint16)
    rng = np.random.default_rng(rng_seed)
    ids = np.unique(A)
    ids = ids[ids > 1]
    split = ids[rng.random(ids.size) < 0.5]
    x = np.indices(dims)
    cnt = np.bincount(A.ravel())
    bc = [np.bincount(A.ravel(), weights=x[d].ravel()) / np.maximum(cnt, 1) for d in range(3)]
    nrm = rng.normal(size=(cnt.size, 3))
    side = sum((x[d] - bc[d][A]) * nrm[:, d][A] for d in range(3)) > 0
    is_split = np.zeros(cnt.size, bool)
    is_split[split] = True
    B = A.astype(np.uint32)
    m = is_split[A] & side
    B[m] = A[m].astype(np.uint32) + offset
    truth = dict((int(l), int(l)) for l in ids)
    for l in split:
        if (B == int(l) + offset).any():
            truth[int(l) + offset] = int(l)
    return A, B, truth


def shifted(V, s, fill=1):
    """V moved by s voxels along each axis, `fill` where nothing arrives."""
    out = np.full_like(V, fill)
    src = tuple(slice(max(0, -d), V.shape[i] - max(0, d)) for i, d in enumerate(s))
    dst = tuple(slice(max(0, d), V.shape[i] - max(0, -d)) for i, d in enumerate(s))
    out[dst] = V[src]
    return out
