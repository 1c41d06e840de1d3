"""The launch plans of the component, junction, distance and nearest-label passes, and label volumes that take them past their limits.

kernels_components.hip, kernels_junctions.hip, kernels_distance.hip and kernels_nearest.hip cap the grids of the kernels that stride over their work: a
workgroup then takes a second trip through its loop.  This file restates, in plain Python and without the library, (1) the grid each
launcher computes for a shape and which loop takes a second trip, (2) where inside a tile, a task or a chunk a voxel or a block lies,
and (3) label volumes that are cheap to make at the shapes that cross each limit, with the closed forms of their tables where the
references of tests/ would take too long.  test_launch_limits_cpu.py checks the restatement and the closed forms against the
references at small shapes; test_gpu_component_limits.py, test_gpu_junction_limits.py and test_gpu_distance_limits.py run the volumes
through the kernels and compare the plan with what the device reports (ta_components_debug, ta_junctions_debug, ta_distance_debug).  The nearest-label pass
has its plan here and its volumes in tests/nearest_cases.py; test_gpu_nearest_limits.py compares with ta_nearest_debug.
"""
import collections

import numpy as np

from tissue_analysis_amd import components

TP, TR, TC = components.TILE                              # the tile of the components' local pass: planes, rows, columns
THREADS = 256                                             # of every workgroup below

# csrc/ta_components.h, csrc/kernels_components.hip
CC_SEAM_MAX_GROUPS = 1 << 18                              # seam pass: one workgroup per row, at most this many
CC_STREAM_MAX_GROUPS = 65536                              # key, row, image and relabel kernels: 256 items a workgroup at a time
CC_STATS_CHUNK, CC_STATS_CHUNKS = 256, 32                 # statistics: voxels of a chunk, chunks a wave walks
# csrc/ta_junctions.h, csrc/kernels_junctions.hip
JN_RPW, JN_PLANES, JN_WAVES = 2, 16, 4                    # block rows and block planes of a task, tasks of a workgroup
JN_KEY_MAX_GROUPS = 8192                                  # key kernel: 256 records a workgroup at a time
# csrc/ta_distance.h, csrc/kernels_distance.hip
DIST_ROW_MAX_GROUPS, DIST_VOXEL_MAX_GROUPS, DIST_INIT_MAX_GROUPS = 1 << 16, 1 << 14, 1 << 12
DIST_ROWS_PER_GROUP, DIST_CHUNK = 4, 64                   # row pass: one wave a row, 64 voxels at a time
# csrc/ta_nearest.h, csrc/kernels_nearest.hip
NEAR_ROW_MAX_GROUPS, NEAR_VOXEL_MAX_GROUPS = 1 << 16, 1 << 14
NEAR_ROWS_PER_GROUP = 4                                   # row pass: one wave a row
NEAR_WORK_CAP, NEAR_STACK_ENTRY = 1 << 30, 28             # bytes of the column passes' stacks, bytes of an entry


def _ceil(a, b):
    return (a + b - 1) // b


def vpl(itemsize):
    """Voxels of a 16-byte strip."""
    return 16 // int(itemsize)


def vector_path(dims, itemsize):
    """Whole 16-byte strips (of an aligned buffer): the local pass and the junction walk take the vector loads."""
    return int(dims[2]) % vpl(itemsize) == 0


def strided_groups(items, cap, per_group=THREADS):
    """(workgroups, trips of the busiest workgroup) of a kernel whose workgroups take per_group items at a time behind a cap."""
    groups = min(max(_ceil(int(items), per_group), 1), cap)
    return groups, _ceil(int(items), groups * per_group)


# ---- components -------------------------------------------------------------------------------------------------------------------
ComponentPlan = collections.namedtuple("ComponentPlan", "tiles rows seam_groups seam_row_trips column_seams column_trips")


def component_plan(dims):
    """The local pass has one workgroup per tile.  The seam pass has one per row behind its cap: workgroup g takes the rows g,
    g + groups, ...; in a row, thread t unites across the tile faces at the columns (t + 1) * TC, (t + 1 + THREADS) * TC, ..."""
    n0, n1, n2 = (int(d) for d in dims)
    rows = n0 * n1
    groups = min(rows, CC_SEAM_MAX_GROUPS)
    seams = (n2 - 1) // TC
    return ComponentPlan(_ceil(n0, TP) * _ceil(n1, TR) * _ceil(n2, TC), rows, groups, _ceil(rows, groups), seams, _ceil(seams, THREADS))


def component_waves(dims):
    """The waves of the kernels that count and hand out the slots (the counts the scan takes): four per 1024 voxels."""
    return 4 * _ceil(int(dims[0]) * int(dims[1]) * int(dims[2]), 1024)


def column_seams_of_trip(dims, trip):
    """The columns c (the voxel behind a tile face along the fast axis) that the seam pass's threads reach in trip `trip` (from 0)."""
    n2 = int(dims[2])
    return [c for c in range((trip * THREADS + 1) * TC, min(n2, ((trip + 1) * THREADS + 1) * TC), TC)]


def seam_rows_of_trip(dims, trip):
    """The rows (q * n1 + r) the seam pass's workgroups take in trip `trip` (from 0)."""
    p = component_plan(dims)
    return range(min(trip * p.seam_groups, p.rows), min((trip + 1) * p.seam_groups, p.rows))


def is_face_row(dims, row):
    """The row lies behind a tile face along axis 0 or 1: the seam pass looks at every voxel of it."""
    q, r = divmod(int(row), int(dims[1]))
    return (q > 0 and q % TP == 0) or (r > 0 and r % TR == 0)


def face_links(V, rows):
    """Voxels of the rows `rows` (q * n1 + r) that share their label with the voxel across a tile face along axis 0 or 1: the pairs
    the seam pass has to unite when it takes those rows."""
    rows = np.asarray(list(rows), dtype=np.int64)
    q, r = rows // V.shape[1], rows % V.shape[1]
    total = 0
    for face, (dq, dr) in (((q > 0) & (q % TP == 0), (1, 0)), ((r > 0) & (r % TR == 0), (0, 1))):
        total += int(np.count_nonzero(V[q[face], r[face]] == V[q[face] - dq, r[face] - dr]))
    return total


def column_links(V, columns):
    """Per row kind (rows behind a tile face, other rows): the rows whose label goes on across one of `columns` (c - 1 -> c)."""
    n0, n1, _ = V.shape
    face = np.array([[is_face_row(V.shape, q * n1 + r) for r in range(n1)] for q in range(n0)])
    joined = np.zeros((n0, n1), dtype=bool)
    for c in columns:
        joined |= V[:, :, c] == V[:, :, c - 1]
    return int(np.count_nonzero(joined & face)), int(np.count_nonzero(joined & ~face))


def stream_groups(items):
    return strided_groups(items, CC_STREAM_MAX_GROUPS)


def stats_chunks(ids, own_begin):
    """Per 256-voxel chunk of the statistics kernel, from the image of component ids (any shape, memory order) and the first owned
    voxel: (one component: bool, owned voxels of the chunk, halo voxels of the chunk).  A chunk of one component whose voxels are
    all owned is kept in registers; one that holds own_begin folds its owned lanes across the wave."""
    flat = np.asarray(ids).reshape(-1)
    n = _ceil(flat.size, CC_STATS_CHUNK)
    one = np.zeros(n, dtype=bool)
    owned = np.zeros(n, dtype=np.int64)
    for k in range(n):
        part = flat[k * CC_STATS_CHUNK:(k + 1) * CC_STATS_CHUNK]
        one[k] = bool((part == part[0]).all())
        owned[k] = int(np.count_nonzero(np.arange(k * CC_STATS_CHUNK, k * CC_STATS_CHUNK + part.size) >= own_begin))
    sizes = np.minimum(CC_STATS_CHUNK, flat.size - np.arange(n) * CC_STATS_CHUNK)
    return one, owned, sizes - owned


def long_rows_blocks(dtype, seed=11):
    """Input A of the long rows: blocks of 300 columns of two labels in rows of 66 000 voxels."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.repeat(rng.integers(1, 3, (2, 5, 221)), 300, axis=2)[:, :, :66000].astype(dtype))


LONG_ROW_DIMS = (2, 5, 66000)
LONG_ROW_SPECK = (1, 2, 65536)                            # input B: the voxel of another label


def long_rows_speck(dtype, dims=LONG_ROW_DIMS, at=LONG_ROW_SPECK):
    """Input B: label 4 everywhere and one voxel of label 9."""
    V = np.full(dims, 4, dtype=dtype)
    V[at] = 9
    return V


MANY_ROWS_DIMS = (520, 510, 4)


def serpentine(dims, dtype=np.uint16):
    """Label 1 winds through the whole volume between walls of label 2: every second row of every second plane, neighbouring rows
    joined at alternating ends, neighbouring planes at alternating corners.  One component of label 1."""
    n0, n1, n2 = dims
    V = np.full(dims, 2, dtype=dtype)
    rows = list(range(0, n1, 2))
    for q in range(0, n0, 2):
        V[q, ::2, :] = 1
        for a, r in enumerate(rows[:-1]):
            V[q, r + 1, n2 - 1 if a % 2 == 0 else 0] = 1
        if q + 2 < n0:
            if (q // 2) % 2 == 0:                         # the snake leaves where the plane's last row ends
                V[q + 1, rows[-1], n2 - 1 if (len(rows) - 1) % 2 == 0 else 0] = 1
            else:
                V[q + 1, 0, 0] = 1
    return V


def run_lengths(itemsize):
    v = vpl(itemsize)
    return sorted(set(list(range(1, 2 * v + 2)) + [63 * v - 1, 63 * v, 64 * v - 1, 64 * v, 64 * v + 1, 255, 256, 257]))


def run_row_length(itemsize):
    return 2 * TC + vpl(itemsize) + 3


def run_rows(itemsize, shift=0):
    """int64 [rows, n2]: one row per (L, o), labels 1 / 2 alternating in runs of L voxels, the first run cut by o + shift voxels."""
    c = np.arange(run_row_length(itemsize))
    return np.stack([1 + ((c + o + shift) // L) % 2 for L in run_lengths(itemsize) for o in range(vpl(itemsize))])


def runs_isolated(dtype):
    """(1, 2 * rows, n2): every second row holds label 3 only, so no run is joined to another one through a neighbouring row."""
    rows = run_rows(np.dtype(dtype).itemsize)
    V = np.full((1, 2 * rows.shape[0], rows.shape[1]), 3, dtype=dtype)
    V[0, ::2] = rows
    return V


def runs_joined(dtype):
    """(3, rows, n2): the same rows, shifted by one voxel per plane: the runs of neighbouring rows and planes overlap at every
    alignment of their ends to the 16-byte strips."""
    itemsize = np.dtype(dtype).itemsize
    return np.ascontiguousarray(np.stack([run_rows(itemsize, p) for p in range(3)]).astype(dtype))


HALO_DIMS, HALO_SLAB = (9, 6, 520), slice(3, 9)


def halo_blocks(dtype):
    """(9, 6, 520), to be adopted as the slab V[3:9] with a low halo.  Odd planes: rows 0 .. 2 label 1, rows 3 .. 5 label 2; even
    planes label 2: label 2 is one component that runs from the halo plane into the owned planes, and whole planes of it are many
    consecutive chunks of one component.  And single voxels of label 3: one in the halo plane only, two among the owned ones."""
    V = np.full(HALO_DIMS, 2, dtype=dtype)
    V[1::2, :3, :] = 1
    V[3, 1, 100] = 3                                      # halo plane of the slab: no row
    V[4, 2, 300] = 3                                      # inside a plane of label 2
    V[6, 4, 519] = 3                                      # the last voxel of a row
    return V


GRID_DIMS, GRID_SPLIT, GRID_LABELS = (66, 500, 512), 33, (5, 8)


def split_planes(dims, split, labels, dtype):
    V = np.full(dims, labels[0], dtype=dtype)
    V[split:] = labels[1]
    return V


def split_planes_table(dims, split, labels):
    """The component table of split_planes(): the rows of components_reference.table()."""
    n0, n1, n2 = (int(d) for d in dims)
    rows = []
    for lo, hi in ((0, split), (split, n0)):
        n = (hi - lo) * n1 * n2
        sums = [n1 * n2 * (lo + hi - 1) * (hi - lo) // 2, (hi - lo) * n2 * n1 * (n1 - 1) // 2, (hi - lo) * n1 * n2 * (n2 - 1) // 2]
        rows.append((n, [lo, 0, 0], [lo, 0, 0, hi, n1, n2], sums))
    assert labels[0] < labels[1]
    return (np.array(labels, dtype=np.int64), np.array([r[0] for r in rows], dtype=np.uint64), np.array([r[1] for r in rows], dtype=np.int64),
            np.array([r[2] for r in rows], dtype=np.int64), np.array([r[3] for r in rows], dtype=np.uint64))


# ---- junctions --------------------------------------------------------------------------------------------------------------------
JunctionPlan = collections.namedtuple("JunctionPlan", "blocks ncb nrb npb tasks groups")
BlockSite = collections.namedtuple("BlockSite", "task lane column far plane_in_task last_plane row_in_task last_row")


def junction_plan(dims, itemsize):
    n0, n1, n2 = (int(d) for d in dims)
    b = (max(n0 - 1, 1), max(n1 - 1, 1), max(n2 - 1, 1))
    ncb, nrb, npb = _ceil(b[2], 64 * vpl(itemsize)), _ceil(b[1], JN_RPW), _ceil(b[0], JN_PLANES)
    return JunctionPlan(b, ncb, nrb, npb, ncb * nrb * npb, _ceil(ncb * nrb * npb, JN_WAVES))


def junction_block_site(dims, itemsize, origin):
    """Where the walk meets the block at `origin`: its task (pb, rb, cb), lane and column within the lane's strip; where the block's far
    column comes from ('strip': the lane's own registers, 'lane': the next lane's, 'load': lane 63's separate load); its block
    plane and block row within the task, and whether they are the task's last (the voxels behind them belong to the next task too)."""
    v = vpl(itemsize)
    q, r, c = (int(x) for x in origin)
    p = junction_plan(dims, itemsize)
    lane, j = (c // v) % 64, c % v
    far = "strip" if j + 1 < v else ("load" if lane == 63 else "lane")
    return BlockSite((q // JN_PLANES, r // JN_RPW, c // (64 * v)), lane, j, far, q % JN_PLANES,
                     q % JN_PLANES == JN_PLANES - 1 and q + 1 < p.blocks[0], r % JN_RPW, r % JN_RPW == JN_RPW - 1 and r + 1 < p.blocks[1])


def junction_key_groups(records):
    return strided_groups(records, JN_KEY_MAX_GROUPS) if records else (0, 0)


CORNER_Q, CORNER_R = (15, 16, 17, 31, 32), (1, 2, 3)


def corner_columns(itemsize):
    v = vpl(itemsize)
    return (v - 1, v, v + 1, 64 * v - 1, 64 * v, 64 * v + 1)


def corner_row_lengths(itemsize):
    """Rows of whole strips (the vector loads) and rows that are not (the scalar loads).  1100 is a multiple of 4, not of 8: the
    uint16 walk takes its vector loads at 1104."""
    return (1100, 1101) if itemsize == 4 else (1100, 1101, 1104)


def corner(Q, R, C, n2, dtype):
    """Four cells that meet in the one block with origin (Q - 1, R - 1, C - 1)."""
    V = np.full((34, 6, n2), 3, dtype=dtype)
    V[:, :R, :C] = 1
    V[:, R:, :C] = 2
    V[Q:, :R, :C] = 4
    return V


STRIPES_DIMS = (66, 130, 260)


def stripes(dims, dtype):
    """(r + c) % 3: every 2 x 2 x 2 block holds exactly the labels 0, 1 and 2."""
    q, r, c = np.indices(dims, sparse=True)
    return np.ascontiguousarray(np.broadcast_to((r + c) % 3, dims).astype(dtype))


def stripes_tables(dims):
    """junction_reference.tables() of stripes(dims): one edge row of every block, no vertex, no degenerate block."""
    B = [int(d) - 1 for d in dims]
    n = B[0] * B[1] * B[2]
    sums = [B[k] * n for k in range(3)]                   # the positions 2 o + 1 over o < B_k add up to B_k^2
    edges = (np.array([[0, 1, 2]], dtype=np.int64), np.array([n], dtype=np.uint64), np.array([sums], dtype=np.uint64))
    none = (np.zeros((0, 4), dtype=np.int64), np.zeros(0, dtype=np.uint64), np.zeros((0, 3), dtype=np.uint64))
    return edges, none, 0


# ---- distance ---------------------------------------------------------------------------------------------------------------------
DistancePlan = collections.namedtuple("DistancePlan", "rows row_groups row_trips voxels voxel_groups voxel_trips table_rows init_groups init_trips")


def distance_plan(dims, table_rows):
    """dims in memory order."""
    n0, n1, n2 = (int(d) for d in dims)
    rows, voxels = n0 * n1, n0 * n1 * n2
    rg, rt = strided_groups(rows, DIST_ROW_MAX_GROUPS, DIST_ROWS_PER_GROUP)
    vg, vt = strided_groups(voxels, DIST_VOXEL_MAX_GROUPS)
    ig, it = strided_groups(table_rows, DIST_INIT_MAX_GROUPS)
    return DistancePlan(rows, rg, rt, voxels, vg, vt, int(table_rows), ig, it)


DIST_WORK_CAP, DIST_STACK_ENTRY = 1 << 30, 20            # bytes of the column passes' stacks, bytes of an entry


def distance_column_launches(dims):
    """Launches of the column kernel along memory axis 1 and along memory axis 0 together, with the automatic batch."""
    n0, n1, n2 = (int(d) for d in dims)
    total = 0
    for length, columns in ((n1, n2 * n0), (n0, n2 * n1)):
        batch = min(max(64, DIST_WORK_CAP // (length * DIST_STACK_ENTRY) // 64 * 64), _ceil(columns, 64) * 64)
        total += _ceil(columns, batch)
    return total


def distance_table(V, d2, rows):
    """distance_reference.table() in whole-array operations, for volumes of many labels: (min2, max2, pole) of the labels
    0 .. rows - 1, the pole the first voxel in the C order of the array axes among those at the label's maximum."""
    V, d2 = np.asarray(V), np.asarray(d2)
    lab = np.ascontiguousarray(V).reshape(-1).astype(np.int64)
    val = np.ascontiguousarray(d2).reshape(-1)
    min2, max2 = np.full(rows, np.inf), np.full(rows, -np.inf)
    np.minimum.at(min2, lab, val)
    np.maximum.at(max2, lab, val)
    at = np.flatnonzero(val == max2[lab])                 # ascending: the first per label is its pole
    labels, first = np.unique(lab[at], return_index=True)
    pole = np.full((rows, 3), -1, dtype=np.int32)
    pole[labels] = np.stack(np.unravel_index(at[first], V.shape), axis=1)
    max2[max2 == -np.inf] = np.inf
    return min2, max2, pole


def run_ends(row):
    """(columns at which a run of the row begins, columns at which one ends): the row pass holds DIST_CHUNK of them at a time."""
    row = np.asarray(row)
    change = np.flatnonzero(row[1:] != row[:-1])
    return set([0] + (change + 1).tolist()), set(change.tolist() + [row.size - 1])


MANY_VOXELS_DIMS, MANY_VOXELS_SPLIT = (66, 250, 256), 125


def half_space_axis1(dims, split, dtype):
    V = np.ones(dims, dtype=dtype)
    V[:, split:, :] = 2
    return V


def half_space_axis1_answer(dims, split, w):
    """(D2 image, (min2, max2, pole) for the rows 0 .. 2) of half_space_axis1() with spacing w along axis 1, without the image margin
    as a site: the distance to the other half, and the pole the first voxel in array order among the farthest."""
    n1 = int(dims[1])
    i = np.arange(n1)
    line = (w * np.where(i < split, split - i, i - split + 1)) ** 2
    d2 = np.broadcast_to(line.reshape(1, -1, 1), dims)
    inf = np.inf
    table = (np.array([inf, w * w, w * w]), np.array([inf, (split * w) ** 2, ((n1 - split) * w) ** 2]),
             np.array([[-1, -1, -1], [0, 0, 0], [0, n1 - 1, 0]], dtype=np.int32))
    return d2, table


MANY_TABLE_ROWS_DIMS, MANY_TABLE_ROWS_LABEL = (4, 8, 64), 1048700


def far_label(dtype=np.uint32):
    V = np.ones(MANY_TABLE_ROWS_DIMS, dtype=dtype)
    V[1:3, 2:6, 20:40] = MANY_TABLE_ROWS_LABEL
    return V


# ---- nearest labels ---------------------------------------------------------------------------------------------------------------
NearestPlan = collections.namedtuple("NearestPlan", "rows row_groups row_trips voxels voxel_groups voxel_trips")


def nearest_plan(dims):
    """dims in memory order.  The row pass gives a workgroup four rows at a time; the counting and the apply pass 256 voxels."""
    n0, n1, n2 = (int(d) for d in dims)
    rows, voxels = n0 * n1, n0 * n1 * n2
    rg, rt = strided_groups(rows, NEAR_ROW_MAX_GROUPS, NEAR_ROWS_PER_GROUP)
    vg, vt = strided_groups(voxels, NEAR_VOXEL_MAX_GROUPS)
    return NearestPlan(rows, rg, rt, voxels, vg, vt)


def nearest_second_trip(dims):
    """(the first row of the row pass's second trip, the first voxel of the streaming kernels' second trip), None where there is none."""
    p = nearest_plan(dims)
    return (p.row_groups * NEAR_ROWS_PER_GROUP if p.row_trips > 1 else None, p.voxel_groups * THREADS if p.voxel_trips > 1 else None)


def nearest_column_launches(dims):
    """Launches of the column kernel along memory axis 1 and along memory axis 0 together, with the automatic batch."""
    n0, n1, n2 = (int(d) for d in dims)
    total = 0
    for length, columns in ((n1, n2 * n0), (n0, n2 * n1)):
        batch = min(max(64, NEAR_WORK_CAP // (length * NEAR_STACK_ENTRY) // 64 * 64), _ceil(columns, 64) * 64)
        total += _ceil(columns, batch)
    return total


def nearest_stack_bytes(dims):
    """Bytes of the envelope stacks with the automatic batch: the larger of the two column passes'."""
    n0, n1, n2 = (int(d) for d in dims)
    return max(length * min(max(64, NEAR_WORK_CAP // (length * NEAR_STACK_ENTRY) // 64 * 64), _ceil(columns, 64) * 64) * NEAR_STACK_ENTRY
               for length, columns in ((n1, n2 * n0), (n0, n2 * n1)))
