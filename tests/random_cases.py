"""A fixed, seeded list of random volumes for tests/test_gpu_random_features.py: NumPy only, importable without a GPU.

case(i) is the frozen description of case i of N_CASES, drawn from numpy.random.default_rng((SEED, i)): the dims, the class of
the label field, of the ids, of the signal, the layout / mode the context is brought into, and the options of every pass.  The
arrays are made from the description by volume(c), signal(c), second(c) -- each from a generator of its own, (SEED, i, k), so
that a change to one drawing leaves the others alone -- and memoised read-only.  pass_order(i) and fetch_order(i) are the two
permutations the runner enqueues and fetches in; chains() deals the cases onto the reused contexts.

The modes are a fixed multiset (MODE_COUNTS: exactly eight slabs) in an order drawn from (SEED, "modes"); everything else is
drawn per case.  Ids above DENSE_ID_LIMIT are drawn only for a compacted context: a dense row table of 2^20 labels x 256 bins
is gigabytes, which is what compaction is for.  tests/test_random_cases_cpu.py is the census of the list; SEED and CHAIN_SEED
were found by counting upwards until a list passed it (about one seed in thirty does).

references(i) computes, once, everything the runner compares a case with (the imports of the reference modules -- scipy, the C
oracle -- happen there, not on import of this file)."""
import collections
import functools

import numpy as np

SEED = 65
CHAIN_SEED = 5
N_CASES = 48
MAX_VOXELS = 160000
UNIQUE_MAX_VOXELS = 4096                # one label per voxel: more would be more rows than a dense context should hold
WALL_VOXEL_CAP = 20000                  # helpers.brute_wall_records takes ~0.1 s at 5 000 voxels, ~0.5 s at 75 000
DENSE_ID_LIMIT = 5000

N2 = (1, 3, 8, 17, 64, 130, 255, 256, 257, 300, 511, 512, 513, 520)
N2_WEIGHTS = (1, 1, 3, 1, 3, 1, 1, 2, 1, 2, 1, 2, 1, 2)       # rows of whole 16-byte strips are 5 of the 14: drawn about as often as the rest
N1 = (1, 2, 3, 4, 5, 7, 9, 16, 21)
N0 = (1, 2, 3, 5, 12, 15, 16, 17, 33)

MODES = ("upload_c", "upload_f", "upload_t", "adopt", "adopt_offset", "slab", "compact")
MODE_COUNTS = dict(upload_c=6, upload_f=6, upload_t=6, adopt=6, adopt_offset=6, slab=8, compact=10)
FIELDS = ("blocky", "speckle", "voronoi", "bodies", "unique")
IDS = ("dense", "zero", "gaps", "u16_top", "u32_sparse")
SIGNALS = ("uniform", "constant", "two", "highbyte", "ramp", "label")
SPACINGS = ((1.0, 1.0, 1.0), (0.5, 0.5, 1.0), (1.0, 0.5, 0.25))
OWN_WALL, FROM_LABEL = 0, 1
PASSES = ("signal", "wallgeo", "overlap", "junctions", "components", "distance", "profile", "sighist", "sigrank")
SLAB_REFUSED = ("distance", "profile", "sigrank")            # passes a slab refuses; so do the mesh and the wall-voxel fetches
FETCHES = ("labels", "adjacency") + PASSES + ("mesh", "walls")
NO_RANK = np.uint64(0xFFFFFFFFFFFFFFFF)

Case = collections.namedtuple("Case", (
    "index name dims field field_arg ids ldtype mode label_off signal_off second_off origin sdtype signal signal_axis bdtype "
    "tile_planes sweep_shape dist_mode site_present edge_is_site spacing prof_bins prof_on_lattice prof_last_inf prof_signal "
    "log2_width rank_kind"))


def _pick(rng, values, weights=None):
    p = None if weights is None else np.asarray(weights, dtype=np.float64) / float(sum(weights))
    return values[int(rng.choice(len(values), p=p))]


@functools.lru_cache(maxsize=None)
def _modes():
    order = [m for m in MODES for _ in range(MODE_COUNTS[m])]
    assert len(order) == N_CASES
    rng = np.random.default_rng((SEED, 0x6D6F6465))
    return tuple(order[k] for k in rng.permutation(N_CASES))


@functools.lru_cache(maxsize=None)
def case(i):
    i = int(i)
    assert 0 <= i < N_CASES
    rng = np.random.default_rng((SEED, i))
    mode = _modes()[i]
    field = _pick(rng, FIELDS, (3, 2, 3, 2, 2))
    cap = UNIQUE_MAX_VOXELS if field == "unique" else MAX_VOXELS
    while True:
        dims = (_pick(rng, N0), _pick(rng, N1), _pick(rng, N2, N2_WEIGHTS))
        if dims[0] * dims[1] * dims[2] <= cap and not (mode == "slab" and dims[0] < 2):       # (a slab: a halo plane and an owned one)
            break
    if field == "blocky":
        field_arg = (int(rng.integers(1, 4, endpoint=True)), int(rng.integers(1, 5, endpoint=True)), int(rng.integers(1, 40, endpoint=True)),
                     _pick(rng, (int(rng.integers(1, 12, endpoint=True)), 64), (3, 1)))
    elif field == "speckle":
        field_arg = int(rng.integers(1, 6, endpoint=True))
    elif field == "voronoi":
        field_arg = _pick(rng, (3, 10, 45, 90))
    elif field == "bodies":
        field_arg = tuple(int(rng.integers(0, 2, endpoint=True)) for _ in range(3))          # cuts along each axis
    else:
        field_arg = None
    ids = _pick(rng, IDS if mode == "compact" else IDS[:3], (1, 1, 1, 2, 2) if mode == "compact" else None)
    ldtype = {"u16_top": "uint16", "u32_sparse": "uint32"}.get(ids) or _pick(rng, ("uint16", "uint32"))
    sdtype = _pick(rng, ("uint8", "uint16"))
    sig = _pick(rng, SIGNALS)
    bdtype = _pick(rng, ("uint16", "uint32"))
    offsets = (1, int(rng.integers(0, 1, endpoint=True)), int(rng.integers(0, 1, endpoint=True))) if mode == "adopt_offset" else (0, 0, 0)
    origin = _pick(rng, (1, 7, 40)) if mode == "slab" else 0
    tile_planes = _pick(rng, (0, 1, 5, 32))
    sweep_shape = _pick(rng, (-1, 0, 1)) if ldtype == "uint32" else -1
    dist_mode = _pick(rng, (OWN_WALL, FROM_LABEL))
    site_present = bool(rng.integers(0, 3)) if dist_mode == FROM_LABEL else True              # (absent: one case in three of mode 1)
    edge = bool(rng.integers(0, 2))
    spacing = _pick(rng, SPACINGS)
    bins = _pick(rng, (1, 5, 64))
    on_lattice, last_inf, prof_signal = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    log2_width = int(rng.integers(0, 8, endpoint=True)) + (8 if sdtype == "uint16" else 0)
    rank_kind = _pick(rng, (0, 0, 0, 0, 1, 2, 3, 8))                                          # 0: sighist_reference.standard_ranks
    name = "%02d-%s-%dx%dx%d-%s-%s-%s-%s-%s%s-b%s-tp%d-sh%d-d%d%s%s-sp%s-k%d%s%s%s-w%d-r%d" % (
        i, mode, dims[0], dims[1], dims[2], field, ids, ldtype.replace("uint", "u"), sdtype.replace("uint", "s"), sig,
        "+%d%d%d" % offsets if mode == "adopt_offset" else ("@%d" % origin if mode == "slab" else ""), bdtype[4:], tile_planes,
        sweep_shape, dist_mode, "" if site_present else "absent", "E" if edge else "", "".join("%g" % (1 / s) for s in spacing), bins,
        "L" if on_lattice else "", "I" if last_inf else "", "S" if prof_signal else "", log2_width, rank_kind)
    return Case(i, name, dims, field, field_arg, ids, ldtype, mode, offsets[0], offsets[1], offsets[2], origin, sdtype, sig,
                int(rng.integers(0, 3)), bdtype, tile_planes, sweep_shape, dist_mode, site_present, edge, spacing, bins, on_lattice,
                last_inf, prof_signal, log2_width, rank_kind)


def cases():
    return [case(i) for i in range(N_CASES)]


def first_owned(c):
    return 1 if c.mode == "slab" else 0


def compacted(c):
    return c.mode == "compact"


def whole(c):
    return c.mode != "slab"


def runs(c, what):
    """Does the runner run pass / fetch `what` on case c (rather than assert the documented refusal)?"""
    if what in SLAB_REFUSED or what == "mesh":
        return whole(c)
    if what == "walls":
        return whole(c) and voxels(c) <= WALL_VOXEL_CAP
    return True


def voxels(c):
    return c.dims[0] * c.dims[1] * c.dims[2]


def memory_order(c):
    """The array axes from the slowest in memory to the fastest, by the rule of ta_volume_set: decreasing stride, the axes of one
    voxel first (they are layout-neutral) in their own order."""
    a = in_layout(c, np.empty(c.dims, dtype=np.uint8))
    return tuple(sorted(range(3), key=lambda d: -(1 << 62 if a.shape[d] == 1 else a.strides[d])))


def memory_dims(c):
    """The dims of the buffer in memory order, slowest axis first."""
    return tuple(c.dims[d] for d in memory_order(c))


def c_ordered(c):
    """Array axes = memory axes: what ta_wall_medians asks for."""
    return memory_order(c) == (0, 1, 2)


def memory_view(c, a):
    """The array `a` of the case's dims with its axes in memory order (shape memory_dims(c))."""
    return a.transpose(memory_order(c))


def in_layout(c, a):
    """The C-ordered array `a` of the case's dims in the memory layout of its mode (the same array, other strides)."""
    if c.mode == "upload_f":
        return np.asfortranarray(a)
    if c.mode == "upload_t":
        return np.ascontiguousarray(a.transpose(1, 2, 0)).transpose(2, 0, 1)
    return np.ascontiguousarray(a)


def _frozen(a):
    a.setflags(write=False)
    return a


def _blocks(rng, dims, block, nlab):
    coarse = [-(-d // b) for d, b in zip(dims, block)]
    v = rng.integers(0, nlab, size=coarse)
    for ax, b in enumerate(block):
        v = np.repeat(v, b, axis=ax)
    return np.ascontiguousarray(v[:dims[0], :dims[1], :dims[2]]).astype(np.int64)


def _field(c, rng):
    """int64 image of label indices 0 .. k - 1."""
    dims = c.dims
    if c.field == "blocky":
        return _blocks(rng, dims, c.field_arg[:3], c.field_arg[3])
    if c.field == "speckle":
        return rng.integers(0, c.field_arg, size=dims).astype(np.int64)
    if c.field == "voronoi":
        from tissue_analysis_amd import synth
        v = synth.voronoi_labels(dims, c.field_arg, int(rng.integers(0, 1 << 30)), dtype=np.uint16)
        return np.unique(v, return_inverse=True)[1].reshape(dims).astype(np.int64)
    if c.field == "bodies":
        body = np.zeros(dims, dtype=np.int64)
        wall = np.zeros(dims, dtype=bool)
        for ax, ncuts in enumerate(c.field_arg):
            n = dims[ax]
            cuts = np.unique(rng.integers(1, max(n - 1, 2), size=ncuts)) if n >= 3 else np.zeros(0, dtype=np.int64)
            shape = [n if a == ax else 1 for a in range(3)]
            body = body * (len(cuts) + 1) + np.searchsorted(cuts, np.arange(n), side="right").reshape(shape)
            wall |= np.isin(np.arange(n), cuts).reshape(shape)
        return np.where(wall, 0, body + 1)
    return rng.permutation(voxels(c)).reshape(dims).astype(np.int64)


def _ids(c, rng, k):
    if c.ids == "dense":
        ids = np.arange(1, k + 1)
    elif c.ids == "zero":
        ids = np.arange(k)
    else:
        top = {"gaps": int(rng.integers(min(2 * k + 1, DENSE_ID_LIMIT), DENSE_ID_LIMIT, endpoint=True)), "u16_top": 65535,
               "u32_sparse": 1 << 20}[c.ids]
        ids = rng.choice(top, size=k - 1, replace=False) if k > 1 else np.zeros(0, dtype=np.int64)      # below top ...
        ids = np.concatenate([ids, [top]])                                                              # ... and top itself
    return rng.permutation(ids).astype(np.int64)


@functools.lru_cache(maxsize=None)
def volume(c):
    """The label volume of the case, C-ordered, with the dims of the BUFFER (a slab's plane 0 is its halo plane)."""
    rng = np.random.default_rng((SEED, c.index, 1))
    f = _field(c, rng)
    return _frozen(_ids(c, rng, int(f.max()) + 1)[f].astype(c.ldtype))


@functools.lru_cache(maxsize=None)
def signal(c):
    rng = np.random.default_rng((SEED, c.index, 2))
    top = int(np.iinfo(c.sdtype).max)
    if c.signal == "uniform":
        s = rng.integers(0, top, size=c.dims, endpoint=True)
    elif c.signal == "constant":
        s = np.full(c.dims, int(rng.integers(0, top, endpoint=True)))
    elif c.signal == "two":
        s = rng.integers(0, 1, size=c.dims, endpoint=True) * top
    elif c.signal == "highbyte":                       # one high byte: every rank of a row shares one selector of the second pass
        s = rng.integers(0, 255, size=c.dims, endpoint=True) + (0x4200 if c.sdtype == "uint16" else 0)
    elif c.signal == "ramp":
        step = 1 if c.sdtype == "uint8" else 97
        line = np.arange(c.dims[c.signal_axis], dtype=np.int64) * step % (top + 1)
        s = np.broadcast_to(line.reshape([-1 if a == c.signal_axis else 1 for a in range(3)]), c.dims)
    else:
        s = volume(c).astype(np.int64) * 37 % (top + 1)
    return _frozen(np.ascontiguousarray(s).astype(c.sdtype))


@functools.lru_cache(maxsize=None)
def second(c):
    """The second label volume of the overlap pass: blocky, seven labels at most."""
    rng = np.random.default_rng((SEED, c.index, 3))
    block = (int(rng.integers(1, 4, endpoint=True)), int(rng.integers(1, 5, endpoint=True)), int(rng.integers(1, 40, endpoint=True)))
    return _frozen(_blocks(rng, c.dims, block, int(rng.integers(1, 7, endpoint=True))).astype(c.bdtype))


@functools.lru_cache(maxsize=None)
def row_image(c):
    """(the row of every voxel, the number of rows, the rank -> id table or None): ranks in a compacted context, else the labels."""
    V = volume(c)
    if not compacted(c):
        return V, int(V.max()) + 1, None
    ids = np.unique(V)
    return _frozen(np.searchsorted(ids, V).astype(V.dtype)), int(ids.size), ids.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def site_label(c):
    """The id the distance map of mode 1 measures from: one the volume holds, or the smallest one it does not."""
    V = volume(c)
    rng = np.random.default_rng((SEED, c.index, 4))
    if c.site_present:
        return int(V.reshape(-1)[int(rng.integers(0, V.size))])
    present = np.unique(V)
    gaps = np.flatnonzero(present != np.arange(present.size))
    return int(gaps[0]) if gaps.size else int(present.size)


@functools.lru_cache(maxsize=None)
def edges2(c):
    """K + 1 ascending squared edges.  On the lattice: multiples of the smallest squared spacing, which D2 takes wherever the
    nearest site lies along that axis alone; off it: halfway between such multiples."""
    rng = np.random.default_rng((SEED, c.index, 5))
    m = min(c.spacing) ** 2
    steps = np.cumsum(rng.integers(1, 3, size=c.prof_bins + 1, endpoint=True)).astype(np.float64)
    first = float(rng.integers(0, 1, endpoint=True))
    e = m * (steps - steps[0] + first if c.prof_on_lattice else steps - 0.5)       # (the first edge: 0 or m; off the lattice m / 2 or 3 m / 2)
    if c.prof_last_inf:
        e[-1] = np.inf
    return _frozen(e)


@functools.lru_cache(maxsize=None)
def ranks(c):
    """u64 [rows, n]: sighist_reference.standard_ranks, or n drawn ranks a row between 0 and two past the row's voxels, one in
    eight of them 'none'."""
    rows, nrows, _ = row_image(c)
    n = np.bincount(rows[first_owned(c):].reshape(-1).astype(np.int64), minlength=nrows).astype(np.uint64)
    if c.rank_kind == 0:
        import sighist_reference
        return _frozen(sighist_reference.standard_ranks(n))
    rng = np.random.default_rng((SEED, c.index, 6))
    r = (rng.random((nrows, c.rank_kind)) * (n[:, None].astype(np.float64) + 2.0)).astype(np.uint64)
    return _frozen(np.where(rng.integers(0, 8, size=r.shape) == 0, NO_RANK, r))


def _order(i, k, names):
    rng = np.random.default_rng((SEED, int(i), k))
    return [names[j] for j in rng.permutation(len(names))]


def pass_order(i):
    """The passes in the order the runner enqueues them: a permutation with the one rule INTEGRATION.md has among them -- the profile
    reads 'the image the context holds, that is of the last ta_distance_extract' (section 19), and is TA_EINVAL without one: should
    the permutation put it first, the two change places."""
    order = _order(i, 8, PASSES)
    d, p = order.index("distance"), order.index("profile")
    if p < d:
        order[d], order[p] = order[p], order[d]
    return tuple(order)


def fetch_order(i):
    return tuple(_order(i, 9, FETCHES))


@functools.lru_cache(maxsize=None)
def chains():
    """Eight chains of six cases for one reused context each.  Eight compacted cases are dealt one to a chain, the other forty in an
    order drawn from CHAIN_SEED; within a chain the largest volume comes first, then the smallest, then alternating, so that every
    case after the first runs in buffers a bigger one left."""
    rng = np.random.default_rng((SEED, CHAIN_SEED, 0x636861))
    compact = [c.index for c in cases() if compacted(c)]
    compact = [compact[k] for k in rng.permutation(len(compact))]
    rest = [i for i in range(N_CASES) if i not in compact[:8]]
    rest = [rest[k] for k in rng.permutation(len(rest))]
    out = []
    for k in range(8):
        members = sorted([compact[k]] + rest[5 * k:5 * k + 5], key=lambda i: (-voxels(case(i)), i))
        out.append(tuple(members[j] for j in (0, 5, 1, 4, 2, 3)))
    return tuple(out)


def transitions(chain):
    """(compacted -> dense, dense -> compacted) steps of a chain."""
    state = [compacted(case(i)) for i in chain]
    return (sum(a and not b for a, b in zip(state[:-1], state[1:])), sum(b and not a for a, b in zip(state[:-1], state[1:])))


# ---- what a case is compared with ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def references(i):
    """dict: the reference of every array the runner fetches for case i, from tests/*_reference.py and the oracle, with the
    `first_owned` / `rows` / `a0_origin` arguments of the case's mode.  Entries of passes the mode refuses are absent."""
    import components_reference
    import distance_reference
    import junction_reference
    import mesh_reference
    import overlap_reference
    import profile_reference
    import sighist_reference
    import signal_reference
    import wall_geometry_reference
    from helpers import brute_wall_records
    from oracle import onepass_c
    from tissue_analysis_amd import geometry

    c = case(i)
    V, S, B = volume(c), signal(c), second(c)
    rows, nrows, ids = row_image(c)
    fo, origin = first_owned(c), c.origin
    # (a halo plane lies one below the slab's origin, and only its faces with plane 1 count)
    sweep = dict(onepass_c.extract(np.ascontiguousarray(rows), max_label=nrows - 1, origin=(origin - fo, 0, 0), own_first_plane=not fo))
    if ids is not None:                                # the pair list answers in ids
        sweep["pair_lo"], sweep["pair_hi"] = ids[sweep["pair_lo"].astype(np.int64)], ids[sweep["pair_hi"].astype(np.int64)]
    by_row = None if ids is None else rows
    ref = dict(sweep=sweep, nrows=nrows, ids=ids,
               signal_labels=signal_reference.labels(V, S, nrows, rows=by_row, first_owned=fo),
               signal_walls=signal_reference.walls(V, S, first_owned=fo),
               wallgeo=wall_geometry_reference.rows(V, first_owned=fo, a0_origin=origin),
               overlap=overlap_reference.table(V, B, first_owned=fo),
               junctions=junction_reference.tables(V, first_owned=fo, a0_origin=origin),
               components=components_reference.table(V, first_owned=fo, a0_origin=origin),
               sighist=sighist_reference.histogram(V, S, nrows, c.log2_width, by_row, fo))
    if whole(c):
        d2 = distance_reference.scipy_d2(V, c.spacing, c.dist_mode, site_label(c), c.edge_is_site)
        ref["d2"] = d2
        ref["distance"] = distance_reference.table(rows, d2, nrows)
        ref["profile"] = profile_reference.table(rows, d2, S if c.prof_signal else None, edges2(c), nrows)
        ref["sigrank"] = sighist_reference.order_statistics(V, S, nrows, ranks(c), by_row, fo)
        ref["mesh"] = mesh_reference.mesh(V)
    if runs(c, "walls"):
        lo, hi, coords = brute_wall_records(V)
        ref["walls"] = (lo, hi, coords)
        keys, count = np.unique((lo.astype(np.uint64) << np.uint64(32)) | hi.astype(np.uint64), return_counts=True)
        if c_ordered(c):                                # (ta_wall_medians refuses the other layouts)
            med, moving = _medians(geometry, coords.astype(np.int64), count)
            ref["medians"] = (keys, count.astype(np.uint32), med.astype(np.int32), moving)
    return ref


def _medians(geometry, coords, count):
    """(geometry.median_voxels of every wall, bool: its iteration did not settle).  The host routine raises when any wall of the
    batch is still moving after its 200 passes, as the reference does; the device marks that wall instead.  Which walls they are is
    found by halving a batch that raised; their medians are left at zero and not compared."""
    try:
        return geometry.median_voxels(coords, count).reshape(-1, 3), np.zeros(count.size, dtype=bool)
    except ValueError:
        if count.size == 1:
            return np.zeros((1, 3), dtype=np.int64), np.ones(1, dtype=bool)
    h = count.size // 2
    cut = int(count[:h].sum())
    a, b = _medians(geometry, coords[:cut], count[:h]), _medians(geometry, coords[cut:], count[h:])
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
