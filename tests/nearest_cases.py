"""Label volumes that put the tie rule and the chunk carry of the nearest-label pass (csrc/kernels_nearest.hip) to work, and a
restatement of its passes with a switch per tie rule.  Host only, seeded, without the library.

  lattice_shell    sites on all integer points of a sphere (an ellipsoid under power-of-two spacings) around a centre voxel: the
                   centre has every site equally near, hundreds of voxels have three or more, and the column through the centre
                   holds parabolas that all meet at one integer position: each pops its predecessor at that one boundary.
                   Every site has its own label; assignments() moves the smallest label over every site in turn.
  row_carry_rows   rows of 200 voxels built by hand around the 64-voxel chunks of the row pass.
  cap_sites        a handful of sites in a volume of any shape, placed around the first row and the first voxel of the second trip
                   of the kernels behind NEAR_ROW_MAX_GROUPS and NEAR_VOXEL_MAX_GROUPS (tests/launch_limits.py).
  model            the row pass and the two column passes, sequential and in plain Python, with one switch per tie rule.  It exists
                   to show WITHOUT a GPU that the cases above tell a kernel that drops a rule from one that keeps it
                   (test_nearest_cpu.py).  The GPU tests never compare with it: their reference is nearest_reference.brute_sites.
"""
import collections
import itertools
import math

import numpy as np

NONE = 0xFFFFFFFF
INF = float("inf")
UNIT, HALF, MIXED = (1.0, 1.0, 1.0), (0.5, 1.0, 2.0), (2.0, 0.25, 1.0)
PERMS = list(itertools.permutations(range(3)))


def in_layout(V, perm):
    """A copy of the array with memory axes perm (slowest first): a fill that writes into it leaves V alone."""
    return np.array(V.transpose(perm), order="C").transpose(np.argsort(perm))


# ---- lattice shells -----------------------------------------------------------------------------------------------------------------
Shell = collections.namedtuple("Shell", "shape centre sites")

# name: (spacing, the spacing as integers, sum (weight * p)^2 over the sites, empty voxels outside the shell, sites)
SHELLS = collections.OrderedDict([
    ("r9", (UNIT, (1, 1, 1), 9, 2, 30)),
    ("r26", (UNIT, (1, 1, 1), 26, 2, 72)),
    ("r41", (UNIT, (1, 1, 1), 41, 1, 96)),
    ("half20", (HALF, (1, 2, 4), 20, 2, 16)),
    ("half36", (HALF, (1, 2, 4), 36, 2, 20)),
    ("mixed80", (MIXED, (8, 1, 4), 80, 2, 16)),
    ("mixed144", (MIXED, (8, 1, 4), 144, 2, 20)),
])


def lattice_shell(weights, c, pad):
    """Shell(shape, centre voxel, int64 [sites, 3] in the C order of the array axes): all integer points p with
    sum (weights[a] * p[a])^2 == c around the centre, and `pad` voxels beyond the outermost site along every axis."""
    reach = [math.isqrt(c // (w * w)) for w in weights]
    points = [p for p in itertools.product(*[range(-r, r + 1) for r in reach]) if sum((w * x) ** 2 for w, x in zip(weights, p)) == c]
    centre = tuple(r + pad for r in reach)
    sites = np.array(sorted(tuple(x + o for x, o in zip(p, centre)) for p in points), dtype=np.int64).reshape(-1, 3)
    return Shell(tuple(2 * (r + pad) + 1 for r in reach), centre, sites)


def shell(name):
    spacing, weights, c, pad, _ = SHELLS[name]
    return lattice_shell(weights, c, pad)


def shell_layouts(name):
    """The memory layouts a shell is run in: all of them for the smallest, C order and one permutation for the others."""
    return PERMS if name == "r9" else [PERMS[0], PERMS[4]]


def shell_d2(name):
    """D2 of the centre: c in the units of the spacing."""
    spacing, weights, c, _, _ = SHELLS[name]
    den = max(float(s).as_integer_ratio()[1] for s in spacing)
    return c / float(den * den)


def assignments(sites, seed=5, randoms=4):
    """(name, uint32 [sites]) label assignments, every one a permutation of 1 .. sites: seeded random ones, and for every site in
    turn the smallest label on it with the others descending, and again ascending, in the order of the sites.  Whatever pass loses
    the label of whatever site, one of them has the smallest label there."""
    rng = np.random.default_rng(seed)
    for k in range(randoms):
        yield "random%d" % k, (rng.permutation(sites) + 1).astype(np.uint32)
    for j in range(sites):
        for name, others in (("down", np.arange(sites, 1, -1)), ("up", np.arange(2, sites + 1))):
            labels = np.insert(others, j, 1).astype(np.uint32)
            yield "%s%d" % (name, j), labels


OFF_CENTRE_SHAPE, OFF_CENTRE_COLUMNS = (11, 11, 140), (64, 127)          # the r9 shell around the end of a chunk of the row pass


def shell_volume(sh, labels, dtype=np.uint16, shape=None, centre=None):
    """The shell's sites with `labels` in an otherwise empty (0) volume; with shape and centre, the shell moved to that centre."""
    V = np.zeros(sh.shape if shape is None else shape, dtype=dtype)
    at = sh.sites if centre is None else sh.sites - np.array(sh.centre) + np.array(centre)
    assert (at >= 0).all() and (at < np.array(V.shape)).all()
    V[tuple(at.T)] = labels
    return V


# ---- rows around the chunks of the row pass -------------------------------------------------------------------------------------------
ROW_LENGTH, ROW_CHUNK = 200, 64
ROW_SPACING = (1.0, 256.0, 1.0)                           # a voxel of another row is farther than any voxel of the own one

# position: label.  The smaller label is the left site in one row and the right site in the next.
CARRY_ROWS = [
    {60: 2, 68: 7}, {60: 7, 68: 2},                       # a tie at 64, the first lane of the second chunk
    {1: 3, 127: 9}, {1: 9, 127: 3},                       # a tie at 64 with the left site carried
    {3: 4, 189: 8}, {3: 8, 189: 4},                       # a tie at 96: the carry goes over the chunk 64 .. 127, which has no site
    {0: 5},
    {199: 6},                                             # in the last chunk, which is 8 voxels
    {63: 11, 64: 10, 128: 12},
    {},
    dict((i, 1 + (7 * i) % 13) for i in range(ROW_LENGTH)),
]


def row_carry_rows():
    """uint16 (1, rows, 200); with ROW_SPACING a row's answer is that of its own sites (the row without a site takes its neighbours')."""
    V = np.zeros((1, len(CARRY_ROWS), ROW_LENGTH), dtype=np.uint16)
    for r, row in enumerate(CARRY_ROWS):
        for i, l in row.items():
            V[0, r, i] = l
    assert V.size <= 4096
    return V


# ---- sites around the second trips of the strided kernels --------------------------------------------------------------------------
CAP_DIMS, CAP_CONTROL_DIMS = (1026, 257, 17), (1019, 257, 16)
CAP_SPACING = (0.5, 1.0, 2.0)
CAP_LATE, CAP_MIDDLE = 1021, 960                          # planes of CAP_DIMS: from here every row is of the row pass's second trip; the
                                                          # first voxel of the streaming kernels' second trip lies in plane 960
# pairs whose bisector passes through rows of the second trip: the plane 1023, and row 45 of every plane; and a pair whose bisector,
# plane 975, lies in the second trip of the streaming kernels only
CAP_PAIRS = [((1022, 100, 5), (1024, 100, 5)), ((1024, 40, 12), (1024, 50, 12)), ((970, 180, 3), (980, 180, 3))]


def cap_sites(dims=CAP_DIMS, dtype=np.uint16, seed=4):
    """16 sites, every one with its own label, in an otherwise empty volume: the pairs above, three more from plane 1021 on, three in
    the planes 960 .. 1019, four in front of them (with this seed none of them comes between a pair: the tests assert the ties).  For
    other dims the same pattern, scaled."""
    rng = np.random.default_rng(seed)
    at = [p for pair in CAP_PAIRS for p in pair]
    for lo, hi, count in ((CAP_LATE, CAP_DIMS[0], 3), (CAP_MIDDLE, 1020, 3), (0, CAP_MIDDLE, 4)):
        for _ in range(count):
            at.append((int(rng.integers(lo, hi)), int(rng.integers(0, CAP_DIMS[1])), int(rng.integers(0, CAP_DIMS[2]))))
    labels = rng.permutation(len(at)) + 1
    V = np.zeros(dims, dtype=dtype)
    for p, l in zip(at, labels):
        V[tuple(x * (n - 1) // (N - 1) for x, n, N in zip(p, dims, CAP_DIMS))] = l
    assert int(np.count_nonzero(V)) == len(at) == 16
    return V


# ---- the passes, restated -------------------------------------------------------------------------------------------------------------
def _column(f, lab, idx, w, chain, boundary, previous):
    """One column (the flat indices idx) in place: the lower envelope of the parabolas f(v) + w^2 (i - v)^2 on a stack of (position,
    f, left boundary, label, boundary label), then the walk back."""
    w2 = w * w
    sv, sf, sz, sl, sb = [], [], [], [], []
    for i, at in enumerate(idx):
        fi = f[at]
        if fi == INF:
            continue
        carried, carried_at, s = NONE, 0.0, -INF
        while sv:
            s = ((fi + w2 * float(i * i)) - (sf[-1] + w2 * float(sv[-1] * sv[-1]))) / (2.0 * w2 * float(i - sv[-1]))
            if s > sz[-1]:
                break
            if s == sz[-1]:                               # the popped entry and what met it at its boundary are lowest at s too
                carried, carried_at = (min(sl[-1], sb[-1]) if chain else sl[-1]), s
            else:
                carried = NONE
            for stack in (sv, sf, sz, sl, sb):
                stack.pop()
        sv.append(i); sf.append(fi); sz.append(s); sl.append(lab[at])
        sb.append(carried if carried != NONE and carried_at == s else NONE)
    if not sv:
        return
    k = len(sv) - 1
    for i in range(len(idx) - 1, -1, -1):
        while sz[k] > i:
            k -= 1
        l = sl[k]
        if sz[k] == i:
            if boundary:
                l = min(l, sb[k])
            if previous:
                l = min(l, sl[k - 1])
        f[idx[i]] = sf[k] + (w * float(i - sv[k])) ** 2
        lab[idx[i]] = l


def model(V, perm=(0, 1, 2), spacing=UNIT, empty=0, not_from=None, chain=True, boundary=True, previous=True):
    """(N uint32, D2 float64) of V held with memory axes perm, by the passes of the kernels.  The switches drop one tie rule each:
    chain     the boundary label of a popped entry goes on to the entry that pops it (off: only the popped entry's own label);
    boundary  the walk back reads the boundary label where a voxel lies exactly on a boundary;
    previous  it reads the label of the entry below there."""
    M = np.ascontiguousarray(np.asarray(V).transpose(perm))
    w = [float(spacing[p]) for p in perm]
    n0, n1, n2 = M.shape
    vol = M.reshape(-1).tolist()
    f, lab = [INF] * len(vol), [NONE] * len(vol)
    for at in range(0, len(vol), n2):                     # rows: the nearest site in front, then the nearest behind
        near, label = [INF] * n2, [NONE] * n2
        for order in (range(n2), range(n2 - 1, -1, -1)):
            pos = None
            for i in order:
                c = vol[at + i]
                if c != empty and c != not_from:
                    pos, site = i, c
                if pos is not None:
                    d = abs(i - pos)
                    if d < near[i] or (d == near[i] and site < label[i]):
                        near[i], label[i] = d, site
        for i in range(n2):
            if near[i] != INF:
                f[at + i], lab[at + i] = (w[2] * float(near[i])) ** 2, label[i]
    for q in range(n0):                                   # columns along memory axis 1 ...
        for c in range(n2):
            _column(f, lab, range(q * n1 * n2 + c, (q + 1) * n1 * n2, n2), w[1], chain, boundary, previous)
    for c in range(n1 * n2):                              # ... and along memory axis 0
        _column(f, lab, range(c, len(vol), n1 * n2), w[0], chain, boundary, previous)
    back = np.argsort(perm)
    return (np.array(lab, dtype=np.uint32).reshape(M.shape).transpose(back), np.array(f, dtype=np.float64).reshape(M.shape).transpose(back))
