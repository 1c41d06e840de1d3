"""CPU model of the device-global adjacency hash (PairTable, csrc/ta_device.h) and builders of the inputs that take it and the
exchange blocks to their limits.  No GPU, no torch: the hash is restated in uint32 arithmetic, everything else comes from the
C oracle and from distributed.slab_exclusive.

The table: open addressing, key = lo << 32 | hi, home slot hash_pair(lo, hi) & (cap - 1), linear probing h = (h + 1) & mask,
at most 512 probes, then FLAG_PAIR_OVERFLOW; finish_extract then grows the table by a factor of four and sweeps again."""
import numpy as np

M32 = 0xFFFFFFFF
PROBES = 512               # probes of one insert before it gives up
GROW_LOG2 = 2              # a table that overflowed grows by 2^2


def hash_u32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def hash_pair(lo, hi):
    return hash_u32(((int(lo) * 0x9E3779B1) & M32) ^ hash_u32(int(hi)))


def home(lo, hi, log2):
    return hash_pair(lo, hi) & ((1 << log2) - 1)


def wraps(lo, hi, log2):
    """True when some probe sequence must cross the end of a table of 2^log2 slots that holds the pairs (lo[i], hi[i]): for
    some slot t more keys have their home in [t, cap) than there are slots in [t, cap).  Whatever the insertion order."""
    cap = 1 << log2
    per_slot = np.zeros(cap, dtype=np.int64)
    for a, b in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist()):
        per_slot[home(a, b, log2)] += 1
    suffix = np.cumsum(per_slot[::-1])[::-1]            # keys at home in [t, cap)
    return bool(np.any(suffix > cap - np.arange(cap)))


def grown_log2(npairs, start):
    """The size a table that starts at 2^start slots ends at, for npairs <= 512 distinct pairs: a key probes at most npairs
    slots before it meets a free one or its own, so the table overflows if and only if it has fewer slots than pairs."""
    if not 0 <= npairs <= PROBES:
        raise ValueError("%d pairs: above %d the probe limit decides, not the slot count" % (npairs, PROBES))
    log2 = start
    while (1 << log2) < npairs:
        log2 += GROW_LOG2
    return log2


def longest_cluster(lo, hi, log2):
    """The longest run of occupied slots (around the end too) of a table of 2^log2 slots that holds these pairs, at most as many
    as slots.  The set of occupied slots does not depend on the insertion order, and an insert probes no further than the end of
    the run its home lies in: with a longest run of at most 512 slots no insertion order overflows."""
    cap = 1 << log2
    slots, _ = probe_insert(list(zip(np.asarray(lo).tolist(), np.asarray(hi).tolist())), log2, probes=cap)
    used = np.array([s is not None for s in slots])
    if used.all():
        return cap
    first_free = int(np.argmin(used))
    best = run = 0
    for u in np.roll(used, -first_free):
        run = run + 1 if u else 0
        best = max(best, run)
    return best


def final_log2(lo, hi, start):
    """The size a table that starts at 2^start ends at, for any number of pairs, where the model can tell: it grows while it has
    fewer slots than pairs, and stays where the longest cluster is within the probe limit.  Refuses the cases in between."""
    n, log2 = len(lo), start
    while (1 << log2) < n:
        log2 += GROW_LOG2
    if longest_cluster(lo, hi, log2) > PROBES:
        raise ValueError("a cluster beyond the probe limit at 2^%d slots: the insertion order decides" % log2)
    return log2


def probe_insert(keys, log2, probes=PROBES):
    """Sequential linear probing with the probe limit, in plain Python: (slots, overflowed)."""
    mask = (1 << log2) - 1
    slots = [None] * (mask + 1)
    overflow = False
    for a, b in keys:
        h = hash_pair(a, b) & mask
        for _ in range(probes):
            if slots[h] is None:
                slots[h] = (a, b)
            if slots[h] == (a, b):
                break
            h = (h + 1) & mask
        else:
            overflow = True
    return slots, overflow


def chain_volume(K, axis, dtype, width=2, other=(3, 4)):
    """Labels 1 .. K + 1 in bands of `width` voxels along `axis`, the two other axes `other` long: exactly K pairs (i, i + 1),
    every one of other[0] * other[1] faces of that axis."""
    labels = np.repeat(np.arange(1, K + 2, dtype=dtype), width)
    shape = list(other)
    shape.insert(axis, labels.size)
    view = [1, 1, 1]
    view[axis] = labels.size
    return np.ascontiguousarray(np.broadcast_to(labels.reshape(view), shape))


def chain_pairs(K):
    return np.arange(1, K + 1, dtype=np.uint32), np.arange(2, K + 2, dtype=np.uint32)


def slab_local(vol, lo, hi, L):
    """The oracle's result for the Z-slab [lo, hi) of `vol`: the slab with one low halo plane (a face belongs to the slab that
    owns its higher voxel along axis 0), in global coordinates."""
    from oracle import onepass_c
    halo = 1 if lo > 0 else 0
    return onepass_c.extract(vol[lo - halo:hi], max_label=L, origin=(lo - halo, 0, 0), own_first_plane=not halo)


def device_boxes(bbox):
    """The device layout of the boxes (min0..2, -max0..2 inclusive, INT32_MAX when absent) from the getter's layout
    (min0..2, max0+1..2+1, -1 when absent): what distributed.slab_exclusive reads."""
    bbox = np.asarray(bbox)
    out = np.full(bbox.shape, np.iinfo(np.int32).max, dtype=np.int32)
    present = bbox[:, 0] >= 0
    out[present, :3] = bbox[present, :3]
    out[present, 3:] = -(bbox[present, 3:] - 1)
    return out


def travelling(local, boxes, lo, hi):
    """The pairs of the slab result `local` that must be in the rank's shared block: neither label exclusive to [lo, hi).
    `boxes`: the GLOBAL boxes in the device layout.  (lo u32[n], hi u32[n], faces u64[n, 3]), sorted as `local` is."""
    from tissue_analysis_amd.distributed import slab_exclusive
    excl = slab_exclusive(boxes, lo, hi)
    go = ~(excl[local["pair_lo"]] | excl[local["pair_hi"]])
    return local["pair_lo"][go], local["pair_hi"][go], local["pair_faces"][go]


def private(local, boxes, lo, hi):
    """... and the pairs that stay at home."""
    from tissue_analysis_amd.distributed import slab_exclusive
    excl = slab_exclusive(boxes, lo, hi)
    stay = excl[local["pair_lo"]] | excl[local["pair_hi"]]
    return local["pair_lo"][stay], local["pair_hi"][stay], local["pair_faces"][stay]


# ---- the cases of test_gpu_pair_table_limits.py and test_gpu_exchange_blocks.py (test_pair_table_cpu.py checks on the CPU that
# each does what its name says)
FULL = [(16, 4), (64, 6), (256, 8), (512, 9)]            # (pairs of the chain, log2 of the table it starts in): exactly full
ONE_MORE = [(17, 4), (65, 6), (257, 8), (513, 9)]        # one pair more than slots
VORONOI_GROWS = ((36, 40, 264), 70, 41)                  # 254 pairs: 2^4 -> 2^6 -> 2^8, and wraps there
SPILL_VOLUME = ((24, 16, 520), 3000, 17)                 # random_blocks: thousands of cells of 30 voxels, 2^4 -> ... -> 2^16
EXCHANGE_VOLUME = ((12, 16, 72), 20, 51)                 # 46 pairs, labels that begin and end near most planes
EVERY_CUT = [[0, c, 12] for c in range(1, 12)]
MORE_SLABS = [[0, 1, 2, 7, 12], [0, 4, 8, 12]]


def wide_chain_volume(K, axis):
    """A uint32 chain whose rows hold whole 512-column tiles of the wide sweep shape and a partial one."""
    if axis == 2:
        return chain_volume(K, 2, np.uint32, width=4 * max(1, -(-130 // (K + 1))), other=(3, 4))
    return chain_volume(K, axis, np.uint32, width=1, other=(2, 516))


def exchange_volume(dtype):
    from tissue_analysis_amd import synth
    dims, n_cells, seed = EXCHANGE_VOLUME
    return synth.voronoi_labels(dims, n_cells, seed, dtype)
