// kernels_overlap.hip -- the label-overlap table between the resident label volume A and a second label volume B of the same
// grid (include/tissue_scan_overlap.h): for every pair (a, b) the voxels p with A[p] == a and B[p] == b, in one streaming pass.
//
// Layout of the pass (the tiling of kernels_signal.hip).  A tile is OV_WAVES rows x (64 lanes x VPL columns) x OV_PLANES planes;
// every wave owns one row of it and walks the planes, each lane holding a strip of VPL = 16 / sizeof(label of A) voxels along
// memory axis 2 (16 bytes of A a lane: 8 uint16 or 4 uint32 labels) and the same voxels of B.  The next plane's strips are
// loaded while the current one is folded.  A workgroup takes a contiguous range of tiles (row blocks of one plane block first,
// so that its pairs stay few) and keeps ONE open-addressed LDS table key -> count for the whole range, which it flushes into
// the device-global open-addressed table once, at its end.
//   A lane folds its voxels into ONE running record (a << 32 | b, n) for as long as the pair does not change -- along its strip
//   and from plane to plane -- and hands it to the LDS table only when it does (inside cells, almost never); the lanes' last
//   records are reduced across the wave pair by pair before they go to the table.  A record that finds no LDS slot within the
//   probe limit goes to the global table directly; a global table that fills up raises OV_FLAG_OVERFLOW (the host runs the
//   pass again into a larger one).
// Any 32-bit value is a label on either side, so the key of the pair (2^32 - 1, 2^32 - 1) IS the empty-slot mark: that one
// pair is counted in a word of its own (OverlapArgs::top) and never enters a table.
// All counts are integers: the results are bit-exact whatever the order of the atomics.
#include "ta_overlap.h"

#include <algorithm>

namespace ta {
namespace {

constexpr int OV_WAVES = 4;                        // rows of a tile = waves of a workgroup
constexpr int OV_THREADS = OV_WAVES * 64;
constexpr int OV_PLANES = 16;                      // planes of a tile
constexpr int OV_SLOTS = 2048;                     // LDS table slots (24 KB: a workgroup's tiles of two C4 frames touch ~1000 pairs)
constexpr int OV_PROBE = 32;                       // LDS probes before a record goes to the global table directly
constexpr uint32_t OV_GLOBAL_PROBE = 512u;         // global probes before the table counts as full
constexpr int64_t OV_MAX_GROUPS = 1024;            // four workgroups a CU
// a lane's record and a workgroup's LDS slots count voxels in u32: fewer than 2^31 voxels a workgroup
constexpr RangeShape OV_RANGE = {OV_WAVES, OV_PLANES, OV_MAX_GROUPS, 31};

struct OvTable {
    unsigned long long key[OV_SLOTS];
    uint32_t n[OV_SLOTS];                          // (a workgroup walks fewer than 2^31 voxels: launch_overlap)
};

__device__ void pair_count_global(const OverlapArgs& A, uint64_t key, uint64_t n) {
    uint32_t h = hash_pair((uint32_t)(key >> 32), (uint32_t)key) & A.mask;
#pragma unroll 1
    for (uint32_t probe = 0; probe < OV_GLOBAL_PROBE; ++probe) {
        unsigned long long k = __hip_atomic_load(&A.keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == EMPTY_KEY) {              // (slots only ever go EMPTY -> key inside a launch: a stale EMPTY is repaired by the CAS)
            k = atomicCAS(&A.keys[h], (unsigned long long)EMPTY_KEY, (unsigned long long)key);
            if (k == EMPTY_KEY) k = key;
        }
        if (k == key) { atomicAdd(&A.counts[h], (unsigned long long)n); return; }
        h = (h + 1) & A.mask;
    }
    atomicOr(&A.flags[OV_FLAG_OVERFLOW], 1u);
}

__device__ __forceinline__ void pair_count_lds(OvTable& S, const OverlapArgs& A, uint64_t key, uint32_t n) {
    if (key == EMPTY_KEY) { atomicAdd(A.top, (unsigned long long)n); return; }
    uint32_t h = hash_pair((uint32_t)(key >> 32), (uint32_t)key) & (OV_SLOTS - 1);
#pragma unroll 1
    for (int probe = 0; probe < OV_PROBE; ++probe) {
        const unsigned long long k = atomicCAS(&S.key[h], (unsigned long long)EMPTY_KEY, (unsigned long long)key);
        if (k == EMPTY_KEY || k == key) { atomicAdd(&S.n[h], n); return; }
        h = (h + 1) & (OV_SLOTS - 1);
    }
    atomicAdd(&A.flags[OV_FLAG_LDS_SPILL], 1u);
    pair_count_global(A, key, n);
}

// N consecutive labels of E from an address aligned to min(16, N * sizeof(E)): loads of 8 or 16 bytes
template <typename E, int N>
__device__ __forceinline__ void load_labels(const E* p, uint32_t (&out)[N]) {
    constexpr int BYTES = N * (int)sizeof(E);
    static_assert(BYTES == 8 || BYTES == 16 || BYTES == 32, "a strip of B is 8, 16 or 32 bytes");
    uint32_t w[BYTES / 4];
    if (BYTES == 8) {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        w[0] = v.x; w[1] = v.y;
    } else {
#pragma unroll
        for (int q = 0; q < BYTES / 16; ++q) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[q];
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = sizeof(E) == 4 ? w[j] : ((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
}

// the strips of row r of plane p that start at column c0; `valid` of their VPL voxels lie inside the row (the others read as 0
// and are never folded).  VEC: every strip is whole or wholly outside the row (n2 % VPL == 0) and both buffers are aligned.
template <typename TA, typename TB, int VPL, bool VEC>
__device__ __forceinline__ void load_strips(const OverlapArgs& A, int64_t p, int64_t r, int64_t c0, int valid, uint32_t (&a)[VPL], uint32_t (&b)[VPL]) {
    const int64_t base = (p * A.n1 + r) * A.n2 + c0;
    if (VEC) {
        if (valid) {
            load_labels<TA, VPL>((const TA*)A.a + base, a);
            load_labels<TB, VPL>((const TB*)A.b + base, b);
        } else {
#pragma unroll
            for (int j = 0; j < VPL; ++j) { a[j] = 0u; b[j] = 0u; }
        }
    } else {
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const bool in = j < valid;
            a[j] = in ? (uint32_t)((const TA*)A.a)[base + j] : 0u;
            b[j] = in ? (uint32_t)((const TB*)A.b)[base + j] : 0u;
        }
    }
}

template <typename TA, typename TB, bool VEC>
__global__ __launch_bounds__(OV_THREADS) void overlap_kernel(const OverlapArgs A) {
    constexpr int VPL = 16 / (int)sizeof(TA);
    __shared__ OvTable S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < OV_SLOTS; i += OV_THREADS) { S.key[i] = EMPTY_KEY; S.n[i] = 0u; }
    __syncthreads();

    const int64_t cols = 64 * VPL;
    const int64_t ncb = (A.n2 + cols - 1) / cols, nrb = (A.n1 + OV_WAVES - 1) / OV_WAVES;
    const int64_t npb = (A.n0 - A.first_owned + OV_PLANES - 1) / OV_PLANES;
    const int64_t tiles = ncb * nrb * npb;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_group;
    const int64_t t1 = t0 + A.tiles_per_group < tiles ? t0 + A.tiles_per_group : tiles;

    // the lane's running record: acc_n voxels of the pair acc_k (acc_n == 0: none yet, acc_k means nothing)
    uint64_t acc_k = 0ull;
    uint32_t acc_n = 0u;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t cb = t % ncb, rb = (t / ncb) % nrb, pb = t / (ncb * nrb);
        const int64_t r = rb * OV_WAVES + wave;
        if (r >= A.n1) continue;                                   // (wave-uniform)
        const int64_t c0 = cb * cols + (int64_t)lane * VPL;
        const int64_t left = A.n2 - c0;
        const int valid = left >= VPL ? VPL : (left > 0 ? (int)left : 0);
        const int64_t pbeg = A.first_owned + pb * OV_PLANES;
        const int64_t pend = pbeg + OV_PLANES < A.n0 ? pbeg + OV_PLANES : A.n0;
        uint32_t ca[VPL], cbl[VPL];                                // this plane
        load_strips<TA, TB, VPL, VEC>(A, pbeg, r, c0, valid, ca, cbl);
        for (int64_t p = pbeg; p < pend; ++p) {
            const bool more = p + 1 < pend;                        // (wave-uniform)
            uint32_t na[VPL], nb[VPL];                             // the next plane, in flight while this one is folded
            if (more) load_strips<TA, TB, VPL, VEC>(A, p + 1, r, c0, valid, na, nb);
            // a whole strip of the running pair (the inside of a cell): one add
            bool same = valid == VPL && acc_n != 0u;
#pragma unroll
            for (int j = 0; j < VPL; ++j) same = same && ca[j] == (uint32_t)(acc_k >> 32) && cbl[j] == (uint32_t)acc_k;
            if (same) {
                acc_n += (uint32_t)VPL;
            } else {
#pragma unroll
                for (int j = 0; j < VPL; ++j) {
                    if (j >= valid) continue;
                    const uint64_t key = ((uint64_t)ca[j] << 32) | cbl[j];
                    if (key != acc_k) {
                        if (acc_n) pair_count_lds(S, A, acc_k, acc_n);
                        acc_k = key; acc_n = 0u;
                    }
                    acc_n += 1u;
                }
            }
            if (more) {
#pragma unroll
                for (int j = 0; j < VPL; ++j) { ca[j] = na[j]; cbl[j] = nb[j]; }
            }
        }
    }

    // the lanes' last records: reduced across the wave one pair at a time, the first lane of the pair adds them to the table
    for (;;) {
        const uint64_t pending = __ballot(acc_n != 0u);
        if (!pending) break;
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const uint64_t K = __shfl(acc_k, leader);
        const bool mine = acc_n != 0u && acc_k == K;
        uint32_t n = mine ? acc_n : 0u;
        for (int o = 32; o > 0; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o);
        if (lane == leader) pair_count_lds(S, A, K, n);
        if (mine) acc_n = 0u;
    }
    __syncthreads();
    for (int i = tid; i < OV_SLOTS; i += OV_THREADS) {
        const uint64_t k = S.key[i];
        if (k != EMPTY_KEY) pair_count_global(A, k, S.n[i]);
    }
}

// ---- compaction of the occupied slots: count, (scan by the caller,) emit ---------------------------------------------------------

__global__ __launch_bounds__(256) void overlap_count_kernel(const unsigned long long* keys, uint64_t slots, uint32_t* block_counts) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * OV_COMPACT_BLOCK;
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t k = 0; k < OV_COMPACT_BLOCK / 256; ++k) {
        const uint64_t i = base + k * 256u + threadIdx.x;
        mine += (i < slots && keys[i] != EMPTY_KEY) ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void overlap_emit_kernel(const unsigned long long* keys, uint64_t slots, const uint64_t* block_offsets,
                                                           int shift_b, uint64_t* sort_keys, uint32_t* slot_of) {
    __shared__ uint32_t cursor;
    if (threadIdx.x == 0) cursor = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * OV_COMPACT_BLOCK, out0 = block_offsets[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < OV_COMPACT_BLOCK / 256; ++k) {
        const uint64_t i = base + k * 256u + threadIdx.x;
        if (i >= slots) continue;
        const uint64_t key = keys[i];
        if (key == EMPTY_KEY) continue;
        const uint64_t at = out0 + atomicAdd(&cursor, 1u);         // (any order inside the block: the rows are sorted afterwards)
        sort_keys[at] = ((key >> 32) << shift_b) | (key & 0xffffffffull);
        slot_of[at] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void overlap_rows_kernel(const uint64_t* sorted_keys, const uint32_t* slot_of, uint64_t n,
                                                           const unsigned long long* counts, int shift_b, uint64_t top, uint32_t* a_out,
                                                           uint32_t* b_out, uint64_t* n_out) {
    const uint64_t bmask = shift_b >= 32 ? 0xffffffffull : ((1ull << shift_b) - 1);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t k = sorted_keys[i];
        a_out[i] = (uint32_t)(k >> shift_b);
        b_out[i] = (uint32_t)(k & bmask);
        n_out[i] = counts[slot_of[i]];
    }
    if (top && blockIdx.x == 0 && threadIdx.x == 0) {              // the pair of the two largest ids: the last row
        a_out[n] = 0xffffffffu; b_out[n] = 0xffffffffu; n_out[n] = top;
    }
}

template <typename TA, typename TB>
void launch_types(hipStream_t s, const OverlapArgs& a, bool vec, int64_t groups) {
    if (vec) hipLaunchKernelGGL((overlap_kernel<TA, TB, true>), dim3((unsigned)groups), dim3(OV_THREADS), 0, s, a);
    else hipLaunchKernelGGL((overlap_kernel<TA, TB, false>), dim3((unsigned)groups), dim3(OV_THREADS), 0, s, a);
}

}  // namespace

RangePlan launch_overlap(hipStream_t s, OverlapArgs a, int itemsize_a, int itemsize_b) {
    const RangeTiles t = range_tiles(a.n0, a.n1, a.n2, a.first_owned, itemsize_a, OV_RANGE);
    const RangePlan plan = plan_ranges(t.tiles, t.tile_voxels, OV_RANGE);
    if (!plan.groups) return plan;
    a.tiles_per_group = plan.tiles_per_group;
    const bool vec = strips_vectorize(a.n2, itemsize_a, {{a.a, itemsize_a}, {a.b, itemsize_b}});      // (a lane's strip of B: 8, 16 or 32 bytes)
    if (itemsize_a == 2 && itemsize_b == 2) launch_types<uint16_t, uint16_t>(s, a, vec, plan.groups);
    else if (itemsize_a == 2) launch_types<uint16_t, uint32_t>(s, a, vec, plan.groups);
    else if (itemsize_b == 2) launch_types<uint32_t, uint16_t>(s, a, vec, plan.groups);
    else launch_types<uint32_t, uint32_t>(s, a, vec, plan.groups);
    return plan;
}

void launch_overlap_count(hipStream_t s, const unsigned long long* keys, uint64_t slots, uint32_t* block_counts) {
    if (!slots) return;
    hipLaunchKernelGGL(overlap_count_kernel, dim3((unsigned)overlap_compact_blocks(slots)), dim3(256), 0, s, keys, slots, block_counts);
}

void launch_overlap_emit(hipStream_t s, const unsigned long long* keys, uint64_t slots, const uint64_t* block_offsets, int shift_b,
                         uint64_t* sort_keys, uint32_t* slot_of) {
    if (!slots) return;
    hipLaunchKernelGGL(overlap_emit_kernel, dim3((unsigned)overlap_compact_blocks(slots)), dim3(256), 0, s, keys, slots, block_offsets,
                       shift_b, sort_keys, slot_of);
}

void launch_overlap_rows(hipStream_t s, const uint64_t* sorted_keys, const uint32_t* slot_of, uint64_t n, const unsigned long long* counts,
                         int shift_b, uint64_t top, uint32_t* a_out, uint32_t* b_out, uint64_t* n_out) {
    if (!n && !top) return;
    const uint64_t blocks = std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 4096);
    hipLaunchKernelGGL(overlap_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, sorted_keys, slot_of, n, counts, shift_b, top, a_out,
                       b_out, n_out);
}

}  // namespace ta
