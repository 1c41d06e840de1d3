// kernels_junctions.hip -- cell junctions (include/tissue_scan_junctions.h): the 2 x 2 x 2 blocks of the resident label volume
// that hold three distinct labels (edges of the cell complex) or four (its vertices), reduced to one row per label set.
//
// The walk.  A task is JN_RPW block rows x (64 lanes x VPL block columns) x JN_PLANES block planes, and one wave walks one task
// plane by plane.  A lane holds, of every one of the task's JN_RPW + 1 rows, a strip of VPL = 16 / sizeof(label) voxels along
// memory axis 2 (16 bytes a lane: 8 uint16 or 4 uint32 labels; rows that are not whole strips take the scalar path) and the
// voxel behind the strip, which comes from the next lane's registers by __shfl (the last lane loads it).  The strips of the
// lower and of the upper plane of the blocks stay in registers: a step loads one new plane, which is the upper plane of this
// step and the lower plane of the next.  Every voxel is read JN_RPW + 1 times for JN_RPW block rows, by waves of one
// workgroup that run side by side (the rows they share come from the cache), and once more at the seam of two plane ranges.
//   Nearly all blocks hold one label.  A lane first compares everything it holds with its first voxel (XOR / OR over the
//   registers): a lane that sees a single label has no block to look at, and that is where ~9 lanes in 10 leave.  The others
//   take the minimum and the maximum of each block's eight voxels; a block with a voxel that is neither has three labels or
//   more, and only there the distinct labels are taken out in ascending order by repeated "smallest above" (at most four).
// Count, scan, emit: the walk runs twice.  The first time every wave counts its blocks of order 3 and 4 (and adds those of
// order >= 5 to one word); the counts are scanned; the second time the wave writes one record per block -- the labels
// ascending and the buffer index of the block's origin -- at its own offset, lanes ordered by a prefix sum across the wave.
// No atomics and nothing to overflow: the records are allocated at their exact number in between.
// After the walks: stable LSD radix sorts (kernels_wallsort.hip) over the label columns from last to first, a kernel that
// marks and counts the first record of every label set, a scan, and a segmented reduce that adds (1, position) of every
// record to its row: partial sums of equal rows inside a wave by shuffles, one atomic add per wave and row.  All integers:
// bit-exact whatever the order.
#include "ta_junctions.h"

#include <algorithm>

namespace ta {
namespace {

constexpr int JN_WAVES = 4;                        // waves of a workgroup: consecutive tasks, neighbours along the rows
constexpr int JN_THREADS = JN_WAVES * 64;
constexpr int JN_RPW = 2;                          // block rows of a task
constexpr int JN_ROWS = JN_RPW + 1;                // rows of voxels a wave holds
constexpr int JN_PLANES = 16;                      // block planes of a task

// one plane of a task as a lane holds it: the strips of the rows and the voxel behind each strip
template <int VPL>
struct Strips {
    uint32_t v[JN_ROWS][VPL];
    uint32_t e[JN_ROWS];
    __device__ __forceinline__ uint32_t at(int i, int j) const { return j < VPL ? v[i][j] : e[i]; }
};

template <typename E, int VPL>
__device__ __forceinline__ void load_vec(const E* p, uint32_t (&out)[VPL]) {
    static_assert(VPL * (int)sizeof(E) == 16, "a strip is 16 bytes");
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < VPL; ++j) out[j] = sizeof(E) == 4 ? w[j] : ((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
}

// plane q, rows r0 .. r0 + JN_RPW, columns c0 .. c0 + VPL: every index is clamped into the volume, so a block that is not
// wholly inside reads copies of voxels that are (it is never counted), and so does the one block layer of a flat axis.
// VEC: n2 is a multiple of VPL and the buffer is 16-byte aligned -- a strip is whole or wholly outside (and then reads as 0).
template <typename E, int VPL, bool VEC>
__device__ __forceinline__ void load_plane(const JunctionArgs& A, int64_t q, int64_t r0, int64_t c0, int lane, Strips<VPL>& S) {
    const E* vol = (const E*)A.vol;
    const int64_t ce = c0 + VPL < A.n2 ? c0 + VPL : A.n2 - 1;      // the voxel behind the strip (last lane only)
#pragma unroll
    for (int i = 0; i < JN_ROWS; ++i) {
        const int64_t r = r0 + i < A.n1 ? r0 + i : A.n1 - 1;
        const E* row = vol + (q * A.n1 + r) * A.n2;
        if (VEC) {
            if (c0 < A.n2) {
                load_vec<E, VPL>(row + c0, S.v[i]);
            } else {
#pragma unroll
                for (int j = 0; j < VPL; ++j) S.v[i][j] = 0u;
            }
        } else {
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int64_t c = c0 + j < A.n2 ? c0 + j : A.n2 - 1;
                S.v[i][j] = (uint32_t)row[c];
            }
        }
        uint32_t last = 0u;
        if (lane == 63) last = (uint32_t)row[ce];
        const uint32_t next = (uint32_t)__shfl_down((int)S.v[i][0], 1);
        S.e[i] = lane == 63 ? last : next;
    }
}

// the smallest of x above t (0xffffffff when there is none: callers know that there is one)
__device__ __forceinline__ uint32_t smallest_above(const uint32_t (&x)[8], uint32_t t) {
    uint32_t r = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < 8; ++k) r = min(r, x[k] > t ? x[k] : 0xffffffffu);
    return r;
}

// 0 for a block of one or two labels, else 3, 4 or 5 (= five or more); m: the three or four labels ascending
__device__ __forceinline__ int block_order(const uint32_t (&x)[8], uint32_t (&m)[4]) {
    uint32_t lo = x[0], hi = x[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) { lo = min(lo, x[k]); hi = max(hi, x[k]); }
    bool other = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) other = other || (x[k] != lo && x[k] != hi);
    if (!other) return 0;
    m[0] = lo;
    m[1] = smallest_above(x, lo);                  // (strictly between lo and hi)
    m[2] = smallest_above(x, m[1]);
    m[3] = m[2];
    if (m[2] == hi) return 3;
    m[3] = smallest_above(x, m[2]);
    return m[3] == hi ? 4 : 5;
}

template <int VPL>
__device__ __forceinline__ void block_voxels(const Strips<VPL>& lo, const Strips<VPL>& hi, int i, int j, uint32_t (&x)[8]) {
    x[0] = lo.at(i, j); x[1] = lo.at(i, j + 1); x[2] = lo.at(i + 1, j); x[3] = lo.at(i + 1, j + 1);
    x[4] = hi.at(i, j); x[5] = hi.at(i, j + 1); x[6] = hi.at(i + 1, j); x[7] = hi.at(i + 1, j + 1);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// exclusive prefix sum of v across the wave; total: the sum over all lanes
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, int lane, uint32_t& total) {
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= d) inc += t;
    }
    total = (uint32_t)__shfl((int)inc, 63);
    return inc - v;
}

template <typename E, bool VEC, bool EMIT>
__global__ __launch_bounds__(JN_THREADS) void junction_pass_kernel(const JunctionArgs A) {
    constexpr int VPL = 16 / (int)sizeof(E);
    constexpr int NB = JN_RPW * VPL;               // blocks of a lane in one step: bit i * VPL + j of the masks below
    const int lane = threadIdx.x & 63;
    const int64_t task = (int64_t)blockIdx.x * JN_WAVES + (threadIdx.x >> 6);
    if (task >= A.ncb * A.nrb * A.npb) return;     // (wave-uniform; no barrier in this kernel)
    const int64_t cb = task % A.ncb, rb = (task / A.ncb) % A.nrb, pb = task / (A.ncb * A.nrb);
    const int64_t r0 = rb * JN_RPW, c0 = (cb * 64 + lane) * VPL;
    const int64_t qbeg = pb * JN_PLANES, qend = qbeg + JN_PLANES < A.b0 ? qbeg + JN_PLANES : A.b0;

    uint32_t valid = 0u;                           // the lane's blocks that lie inside the volume
#pragma unroll
    for (int i = 0; i < JN_RPW; ++i)
#pragma unroll
        for (int j = 0; j < VPL; ++j)
            if (r0 + i < A.b1 && c0 + j < A.b2) valid |= 1u << (i * VPL + j);

    uint32_t cnt3 = 0u, cnt4 = 0u, cnt5 = 0u;      // (a task has fewer than 2^31 blocks)
    uint64_t base3 = 0ull, base4 = 0ull;           // EMIT: where the wave's next records go (wave-uniform)
    if (EMIT) { base3 = A.wave_offsets3[task]; base4 = A.wave_offsets4[task]; }

    Strips<VPL> lo, hi;
    load_plane<E, VPL, VEC>(A, qbeg, r0, c0, lane, lo);
    for (int64_t q = qbeg; q < qend; ++q) {
        const int64_t qu = q + 1 < A.n0 ? q + 1 : A.n0 - 1;       // (a flat axis 0: the block's one plane twice)
        load_plane<E, VPL, VEC>(A, qu, r0, c0, lane, hi);
        // one label in everything the lane holds: none of its blocks is a junction
        const uint32_t first = lo.v[0][0];
        uint32_t diff = 0u;
#pragma unroll
        for (int i = 0; i < JN_ROWS; ++i) {
#pragma unroll
            for (int j = 0; j < VPL; ++j) diff |= (lo.v[i][j] ^ first) | (hi.v[i][j] ^ first);
            diff |= (lo.e[i] ^ first) | (hi.e[i] ^ first);
        }
        uint32_t mask3 = 0u, mask4 = 0u;
        if (diff != 0u && valid != 0u) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                uint32_t x[8], m[4];
                block_voxels<VPL>(lo, hi, b / VPL, b % VPL, x);
                const int order = (valid >> b) & 1u ? block_order(x, m) : 0;
                if (order == 3) mask3 |= 1u << b;
                if (order == 4) mask4 |= 1u << b;
                if (order == 5) cnt5 += 1u;
            }
        }
        if (!EMIT) {
            cnt3 += (uint32_t)__popc(mask3);
            cnt4 += (uint32_t)__popc(mask4);
        } else if (__ballot((mask3 | mask4) != 0u)) {             // (wave-uniform)
            uint32_t tot3, tot4;
            uint64_t at3 = base3 + wave_exclusive((uint32_t)__popc(mask3), lane, tot3);
            uint64_t at4 = base4 + wave_exclusive((uint32_t)__popc(mask4), lane, tot4);
            base3 += tot3; base4 += tot4;
            if ((mask3 | mask4) != 0u) {
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if (!(((mask3 | mask4) >> b) & 1u)) continue;
                    uint32_t x[8], m[4];
                    block_voxels<VPL>(lo, hi, b / VPL, b % VPL, x);
                    const int order = block_order(x, m);
                    const uint64_t origin = (uint64_t)((q * A.n1 + r0 + b / VPL) * A.n2 + c0 + b % VPL);
                    if (order == 3) {
                        A.labels3[3 * at3] = m[0]; A.labels3[3 * at3 + 1] = m[1]; A.labels3[3 * at3 + 2] = m[2];
                        A.origin3[at3] = origin;
                        ++at3;
                    } else {
                        A.labels4[4 * at4] = m[0]; A.labels4[4 * at4 + 1] = m[1]; A.labels4[4 * at4 + 2] = m[2]; A.labels4[4 * at4 + 3] = m[3];
                        A.origin4[at4] = origin;
                        ++at4;
                    }
                }
            }
        }
        lo = hi;
    }
    if (!EMIT) {
        cnt3 = wave_sum(cnt3); cnt4 = wave_sum(cnt4); cnt5 = wave_sum(cnt5);
        if (lane == 0) {
            A.wave_counts3[task] = cnt3;
            A.wave_counts4[task] = cnt4;
            if (cnt5) atomicAdd(A.degenerate, (unsigned long long)cnt5);
        }
    }
}

// ---- after the walks ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void junction_keys_kernel(const uint32_t* labels, int K, uint64_t n, const uint32_t* order, int col_hi,
                                                            int col_lo, int label_bits, uint64_t* keys_out, uint32_t* index_out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t rec = order ? order[i] : i;
        const uint32_t* l = labels + rec * (uint64_t)K;
        uint64_t key = l[col_lo];
        if (col_hi >= 0) key |= (uint64_t)l[col_hi] << label_bits;
        keys_out[i] = key;
        if (!order) index_out[i] = (uint32_t)i;
    }
}

// record i of the sorted order starts a row: it is the first, or its labels differ from those of record i - 1
__device__ __forceinline__ bool row_head(const uint32_t* labels, int K, const uint32_t* order, uint64_t i) {
    if (i == 0) return true;
    const uint32_t* a = labels + (uint64_t)order[i] * K;
    const uint32_t* b = labels + (uint64_t)order[i - 1] * K;
    bool differ = false;
    for (int k = 0; k < K; ++k) differ = differ || a[k] != b[k];
    return differ;
}

__global__ __launch_bounds__(JN_ROW_BLOCK) void junction_heads_kernel(const uint32_t* labels, int K, const uint32_t* order, uint64_t n,
                                                                      uint32_t* block_counts) {
    __shared__ uint32_t part[JN_ROW_BLOCK / 64];
    const uint64_t i = (uint64_t)blockIdx.x * JN_ROW_BLOCK + threadIdx.x;
    const bool head = i < n && row_head(labels, K, order, i);
    const uint64_t m = __ballot(head);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0u;
        for (int w = 0; w < (int)(JN_ROW_BLOCK / 64); ++w) t += part[w];
        block_counts[blockIdx.x] = t;
    }
}

__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d), hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(JN_ROW_BLOCK) void junction_reduce_kernel(const uint32_t* labels, const uint64_t* origins, int K,
                                                                       const uint32_t* order, uint64_t n, const uint64_t* block_offsets,
                                                                       const JunctionRows R) {
    __shared__ uint32_t part[JN_ROW_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * JN_ROW_BLOCK + threadIdx.x;
    const bool live = i < n;
    const bool head = live && row_head(labels, K, order, i);
    const uint64_t m = __ballot(head);
    if (lane == 0) part[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0u;                          // rows that start in the block's earlier waves
    for (int w = 0; w < wave; ++w) before += part[w];
    // heads up to and including this record, minus one: the record's row (record 0 is a head, so this is never negative)
    const uint64_t upto = m & (lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1));
    uint64_t row = ~0ull;                          // (a lane behind the last record: a row of its own that is never written)
    uint64_t cnt = 0ull, s[3] = {0ull, 0ull, 0ull};
    if (live) {
        row = block_offsets[blockIdx.x] + before + (uint64_t)__popcll(upto) - 1;
        const uint64_t rec = order[i];
        if (head)
            for (int k = 0; k < K; ++k) R.labels[row * K + k] = labels[rec * K + k];
        const uint64_t o = origins[rec];
        const uint64_t o2 = o % (uint64_t)R.n2, o1 = (o / (uint64_t)R.n2) % (uint64_t)R.n1, o0 = o / ((uint64_t)R.n2 * (uint64_t)R.n1);
        cnt = 1ull;
        s[0] = R.flat[0] ? 0ull : 2 * ((uint64_t)R.origin0 + o0) + 1;
        s[1] = R.flat[1] ? 0ull : 2 * o1 + 1;
        s[2] = R.flat[2] ? 0ull : 2 * o2 + 1;
    }
    // rows ascend along the wave: after the step of distance d a lane holds the sum of its row's records in [lane, lane + 2d)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t orow = shfl_down_u64(row, d);
        const uint64_t oc = shfl_down_u64(cnt, d), o0 = shfl_down_u64(s[0], d), o1 = shfl_down_u64(s[1], d), o2 = shfl_down_u64(s[2], d);
        if (lane + d < 64 && orow == row) { cnt += oc; s[0] += o0; s[1] += o1; s[2] += o2; }
    }
    const uint64_t prow = (uint64_t)(((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(row >> 32), 1) << 32) | (uint32_t)__shfl_up((int)(uint32_t)row, 1));
    if (live && (lane == 0 || prow != row)) {      // the first lane of a row inside this wave
        atomicAdd(&R.n[row], (unsigned long long)cnt);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (s[k]) atomicAdd(&R.sums[row * 3 + R.axis[k]], (unsigned long long)s[k]);
    }
}

template <typename E>
void launch_pass_type(hipStream_t s, const JunctionArgs& a, bool vec, bool emit, unsigned groups) {
    if (vec && emit) hipLaunchKernelGGL((junction_pass_kernel<E, true, true>), dim3(groups), dim3(JN_THREADS), 0, s, a);
    else if (vec) hipLaunchKernelGGL((junction_pass_kernel<E, true, false>), dim3(groups), dim3(JN_THREADS), 0, s, a);
    else if (emit) hipLaunchKernelGGL((junction_pass_kernel<E, false, true>), dim3(groups), dim3(JN_THREADS), 0, s, a);
    else hipLaunchKernelGGL((junction_pass_kernel<E, false, false>), dim3(groups), dim3(JN_THREADS), 0, s, a);
}

unsigned grid_for(uint64_t n) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), JN_KEY_MAX_GROUPS); }

}  // namespace

uint64_t junction_plan(JunctionArgs& a, int itemsize) {
    const int64_t cols = 64 * (16 / itemsize);
    a.b0 = a.n0 > 1 ? a.n0 - 1 : 1;
    a.b1 = a.n1 > 1 ? a.n1 - 1 : 1;
    a.b2 = a.n2 > 1 ? a.n2 - 1 : 1;
    a.ncb = (a.b2 + cols - 1) / cols;
    a.nrb = (a.b1 + JN_RPW - 1) / JN_RPW;
    a.npb = (a.b0 + JN_PLANES - 1) / JN_PLANES;
    return (uint64_t)a.ncb * (uint64_t)a.nrb * (uint64_t)a.npb;
}

void launch_junction_pass(hipStream_t s, const JunctionArgs& a, int itemsize, bool emit) {
    const uint64_t waves = (uint64_t)a.ncb * (uint64_t)a.nrb * (uint64_t)a.npb;
    if (!waves) return;
    const unsigned groups = (unsigned)((waves + JN_WAVES - 1) / JN_WAVES);
    const bool vec = a.n2 % (16 / itemsize) == 0 && ((uintptr_t)a.vol % 16) == 0;
    if (itemsize == 2) launch_pass_type<uint16_t>(s, a, vec, emit, groups);
    else launch_pass_type<uint32_t>(s, a, vec, emit, groups);
}

uint32_t launch_junction_keys(hipStream_t s, const uint32_t* labels, int K, uint64_t n, const uint32_t* order, int col_hi, int col_lo,
                              int label_bits, uint64_t* keys_out, uint32_t* index_out) {
    if (!n) return 0u;
    hipLaunchKernelGGL(junction_keys_kernel, dim3(grid_for(n)), dim3(256), 0, s, labels, K, n, order, col_hi, col_lo, label_bits, keys_out,
                       index_out);
    return grid_for(n);
}

void launch_junction_heads(hipStream_t s, const uint32_t* labels, int K, const uint32_t* order, uint64_t n, uint32_t* block_counts) {
    if (!n) return;
    hipLaunchKernelGGL(junction_heads_kernel, dim3((unsigned)junction_row_blocks(n)), dim3(JN_ROW_BLOCK), 0, s, labels, K, order, n,
                       block_counts);
}

void launch_junction_reduce(hipStream_t s, const uint32_t* labels, const uint64_t* origins, int K, const uint32_t* order, uint64_t n,
                            const uint64_t* block_offsets, const JunctionRows& rows) {
    if (!n) return;
    hipLaunchKernelGGL(junction_reduce_kernel, dim3((unsigned)junction_row_blocks(n)), dim3(JN_ROW_BLOCK), 0, s, labels, origins, K, order,
                       n, block_offsets, rows);
}

}  // namespace ta
