// kernels_topology.hip -- the twelve block counts per label behind the Euler numbers (include/tissue_scan_topology.h): n0, n1[3],
// n2[3], n3, v, e[3] over the 2 x 2 x 2 blocks of the resident label volume, the blocks that reach over its faces included.
//
// Positions and ownership.  A block is named by the position p = origin + 1 of its voxel 7, p in [0, N0] x [0, N1] x [0, N2]: its
// voxels are p - {0,1}^3, bit 4a + 2b + c at p - 1 + (a, b, c); whatever lies outside the volume reads as INVALID_LABEL and is
// never fetched.  The tile that owns a block is the tile that owns its position:
//   - along axes 0 and 1 the tiles cover the positions 0 .. N0 and 0 .. N1, one more than there are planes and rows: the blocks
//     beyond the high faces fall to the tiles there as positions of their own (a row or plane of INVALID_LABEL);
//   - along axis 2 the tiles cover the columns 0 .. N2 - 1, and the lane that holds column N2 - 1 also takes the block at N2.
// So every block of the header's range is counted exactly once, whatever the dims.
//
// The walk is that of kernels_junctions.hip.  A tile is TP_WAVES positions along axis 1 x (64 lanes x VPL columns) x TP_PLANES
// positions along axis 0; a wave owns one row position p1 of it and walks the plane positions.  A lane holds, of the rows
// p1 - 1 and p1, a strip of VPL = 16 / sizeof(label) voxels and the voxel before the strip, which comes from the previous
// lane's registers by __shfl (the first lane loads it); the lower and the upper plane of the blocks stay in registers, a step
// loads one plane, and the plane after it is in flight while the step is worked on.  Rows that are whole strips of an aligned
// buffer take one 16-byte load a strip, the others element loads.
//
// Accumulation is that of the range passes (ta_range_plan.h): a workgroup takes a contiguous range of tiles, keeps one LDS hash
// table label -> twelve u32 counters for it and flushes the table with u64 global atomics once, at its end; a record whose probe
// fails goes to the global rows and counts in the spill flag.
//   Nearly all blocks hold one label.  A block that is wholly of one label adds one to each of the twelve counters, so a lane
//   only counts them (`full`) in its running record; a lane that sees a single label in everything it holds adds VPL at once.
//   The running record goes to the LDS table only when the label changes; the lanes' last records are reduced across the wave.
//   A mixed block forms, for each of its distinct labels (at most eight), the 8-bit membership mask; the twelve contributions
//   are tests of that mask.  Those of the running record's label stay in registers, the others go to the table at once.
// All integers: bit-exact whatever the order of the atomics.  Widths: a workgroup walks at most 2^31 positions (TP_RANGE) and one
// block more per row and plane of a tile, so its u32 counters hold; the global rows are u64.
#include "ta_topology.h"

namespace ta {
namespace {

constexpr int TP_WAVES = 4;                        // row positions of a tile = waves of a workgroup
constexpr int TP_THREADS = TP_WAVES * 64;
constexpr int TP_PLANES = 16;                      // plane positions of a tile
constexpr int TP_PROBE = 32;                       // probes before a record goes to the global rows directly
constexpr int TP_NC = 12;                          // counters of a row: n0 | n1[3] | n2[3] | n3 | v | e[3]
constexpr RangeShape TP_RANGE = {TP_WAVES, TP_PLANES, TP_MAX_GROUPS, 31};

struct TopoTable {
    uint32_t key[TP_SLOTS];
    uint32_t c[TP_NC][TP_SLOTS];
};
static_assert(sizeof(TopoTable) == 52 * TP_SLOTS && 4 * sizeof(TopoTable) <= 160 * 1024, "four workgroups a CU");

// what a block adds for the label whose voxels are the bits of m
__device__ __forceinline__ void mask_counts(uint32_t m, uint32_t (&c)[TP_NC]) {
    c[0] = m >> 7;                                                             // voxel 7
    c[1] = (m & 0x88u) == 0x88u; c[2] = (m & 0xA0u) == 0xA0u; c[3] = (m & 0xC0u) == 0xC0u;   // voxel 7 and bit 3, 5, 6
    c[4] = (m & 0xF0u) == 0xF0u; c[5] = (m & 0xCCu) == 0xCCu; c[6] = (m & 0xAAu) == 0xAAu;   // the upper half along axis 0, 1, 2
    c[7] = m == 0xFFu;
    c[8] = m != 0u;
    c[9] = (m & 0xF0u) != 0u; c[10] = (m & 0xCCu) != 0u; c[11] = (m & 0xAAu) != 0u;
}

// (the counters by value: in registers across the call, not through the stack)
struct Counts { uint32_t c[TP_NC]; };

__device__ void rec_add_global(const TopologyArgs& A, uint32_t l, const Counts C) {
    const uint32_t (&c)[TP_NC] = C.c;
    if (l > A.max_label) { atomicOr(&A.flags[TP_FLAG_RANGE], 1u); return; }
    if (c[0]) atomicAdd(&A.n0c[l], (unsigned long long)c[0]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (c[1 + k]) atomicAdd(&A.n1c[3 * (uint64_t)l + k], (unsigned long long)c[1 + k]);
        if (c[4 + k]) atomicAdd(&A.n2c[3 * (uint64_t)l + k], (unsigned long long)c[4 + k]);
        if (c[9 + k]) atomicAdd(&A.ec[3 * (uint64_t)l + k], (unsigned long long)c[9 + k]);
    }
    if (c[7]) atomicAdd(&A.n3c[l], (unsigned long long)c[7]);
    if (c[8]) atomicAdd(&A.vc[l], (unsigned long long)c[8]);
}

__device__ __forceinline__ void rec_add_lds(TopoTable& S, const TopologyArgs& A, uint32_t l, const uint32_t (&c)[TP_NC]) {
    uint32_t h = __umulhi(hash_u32(l), (uint32_t)TP_SLOTS);
    for (int probe = 0; probe < TP_PROBE; ++probe) {
        const uint32_t k = atomicCAS(&S.key[h], INVALID_LABEL, l);
        if (k == INVALID_LABEL || k == l) {
#pragma unroll
            for (int i = 0; i < TP_NC; ++i)
                if (c[i]) atomicAdd(&S.c[i][h], c[i]);
            return;
        }
        h = h + 1 == (uint32_t)TP_SLOTS ? 0u : h + 1;
    }
    atomicAdd(&A.flags[TP_FLAG_SPILL], 1u);
    Counts C;
#pragma unroll
    for (int i = 0; i < TP_NC; ++i) C.c[i] = c[i];
    rec_add_global(A, l, C);
}

// a lane's running record: the blocks of one label
struct Rec {
    uint32_t full;                                 // blocks wholly of the label: one to every counter
    uint32_t c[TP_NC];                             // what its mixed blocks added
    __device__ __forceinline__ void clear() {
        full = 0u;
#pragma unroll
        for (int i = 0; i < TP_NC; ++i) c[i] = 0u;
    }
    __device__ __forceinline__ void total(uint32_t (&t)[TP_NC]) const {
#pragma unroll
        for (int i = 0; i < TP_NC; ++i) t[i] = c[i] + full;
    }
};

// one plane as a lane holds it: of the rows p1 - 1 (i = 0) and p1 (i = 1), v[i][0] the voxel before the strip and v[i][1 + j]
// column c0 + j
template <int VPL>
struct Plane {
    uint32_t v[2][VPL + 1];
    // column c0 - 1 + k of row i; behind the strip (k == VPL + 1, the block at N2 only) there is no voxel
    __device__ __forceinline__ uint32_t at(int i, int k) const { return k <= VPL ? v[i][k] : INVALID_LABEL; }
};

template <typename E, int VPL>
__device__ __forceinline__ void load_vec(const E* p, uint32_t* out) {
    static_assert(VPL * (int)sizeof(E) == 16, "a strip is 16 bytes");
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < VPL; ++j) out[j] = sizeof(E) == 4 ? w[j] : ((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
}

// Plane p, rows p1 - 1 and p1, columns c0 - 1 .. c0 + VPL - 1; a plane, a row or a column outside the volume is INVALID_LABEL
// and not fetched (p and p1 are wave-uniform).  VEC: n2 is a multiple of VPL and the buffer is 16-byte aligned -- a strip is
// whole or wholly outside.
template <typename E, int VPL, bool VEC>
__device__ __forceinline__ void load_plane(const TopologyArgs& A, int64_t p, int64_t p1, int64_t c0, int lane, Plane<VPL>& P) {
    const E* vol = (const E*)A.vol;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t r = p1 - 1 + i;
        if (p < 0 || p >= A.n0 || r < 0 || r >= A.n1) {
#pragma unroll
            for (int k = 0; k <= VPL; ++k) P.v[i][k] = INVALID_LABEL;
            continue;
        }
        const E* row = vol + (p * A.n1 + r) * A.n2;
        if (VEC) {
            if (c0 < A.n2) {
                load_vec<E, VPL>(row + c0, &P.v[i][1]);
            } else {
#pragma unroll
                for (int j = 0; j < VPL; ++j) P.v[i][1 + j] = INVALID_LABEL;
            }
        } else {
#pragma unroll
            for (int j = 0; j < VPL; ++j) P.v[i][1 + j] = c0 + j < A.n2 ? (uint32_t)row[c0 + j] : INVALID_LABEL;
        }
        uint32_t first = INVALID_LABEL;            // the first lane's: column c0 - 1 < n2 of the tile before, or none
        if (lane == 0 && c0 > 0) first = (uint32_t)row[c0 - 1];
        const uint32_t prev = (uint32_t)__shfl_up((int)P.v[i][VPL], 1);
        P.v[i][0] = lane == 0 ? first : prev;
    }
}

// the smallest label among the voxels of x whose bit is set in `left` (there is one)
__device__ __forceinline__ uint32_t smallest_left(const uint32_t (&x)[8], uint32_t left) {
    uint32_t r = INVALID_LABEL;
#pragma unroll
    for (int b = 0; b < 8; ++b) r = min(r, (left >> b) & 1u ? x[b] : INVALID_LABEL);
    return r;
}

template <typename E, bool VEC>
__global__ __launch_bounds__(TP_THREADS, 4) void topology_kernel(const TopologyArgs A) {
    constexpr int VPL = 16 / (int)sizeof(E);
    __shared__ TopoTable S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < TP_SLOTS; i += TP_THREADS) {
        S.key[i] = INVALID_LABEL;
#pragma unroll
        for (int k = 0; k < TP_NC; ++k) S.c[k][i] = 0u;
    }
    __syncthreads();

    const int64_t cols = 64 * VPL;
    const int64_t ncb = (A.n2 + cols - 1) / cols, nrb = (A.n1 + 1 + TP_WAVES - 1) / TP_WAVES;
    const int64_t npb = (A.n0 + 1 + TP_PLANES - 1) / TP_PLANES;
    const int64_t tiles = ncb * nrb * npb;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_group;
    const int64_t t1 = t0 + A.tiles_per_group < tiles ? t0 + A.tiles_per_group : tiles;

    uint32_t acc_l = INVALID_LABEL;                // the label of the lane's running record
    Rec R;
    R.clear();
    uint32_t nmixed = 0u;                          // blocks of two labels or more

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t cb = t % ncb, rb = (t / ncb) % nrb, pb = t / (ncb * nrb);
        const int64_t p1 = rb * TP_WAVES + wave;
        if (p1 > A.n1) continue;                   // (wave-uniform)
        const int64_t c0 = cb * cols + (int64_t)lane * VPL;
        const int64_t pbeg = pb * TP_PLANES;
        const int64_t pend = pbeg + TP_PLANES < A.n0 + 1 ? pbeg + TP_PLANES : A.n0 + 1;

        uint32_t valid = 0u;                       // the lane's blocks: bit j at column c0 + j, bit VPL the block at N2
#pragma unroll
        for (int j = 0; j <= VPL; ++j)
            if ((j < VPL && c0 + j < A.n2) || (j > 0 && c0 + j == A.n2)) valid |= 1u << j;

        Plane<VPL> lo, hi;
        load_plane<E, VPL, VEC>(A, pbeg - 1, p1, c0, lane, lo);
        load_plane<E, VPL, VEC>(A, pbeg, p1, c0, lane, hi);
        uint32_t lo_diff = 0u;                     // 0: everything the lane holds of the lower plane is lo.v[0][0]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int k = 0; k <= VPL; ++k) lo_diff |= lo.v[i][k] ^ lo.v[0][0];

        for (int64_t p = pbeg; p < pend; ++p) {
            const bool more = p + 1 < pend;        // (wave-uniform)
            Plane<VPL> nx;                         // the next plane, in flight while this step is worked on
            if (more) load_plane<E, VPL, VEC>(A, p + 1, p1, c0, lane, nx);

            const uint32_t first = hi.v[0][0];
            uint32_t hi_diff = 0u;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int k = 0; k <= VPL; ++k) hi_diff |= hi.v[i][k] ^ first;

            uint32_t todo = valid;                 // blocks to look at one by one
            if ((lo_diff | hi_diff | (lo.v[0][0] ^ first)) == 0u && first != INVALID_LABEL) {
                // one label in everything the lane holds: the VPL blocks in front of the strip's columns are wholly of it
                if (first != acc_l) {
                    if (acc_l != INVALID_LABEL) { uint32_t tot[TP_NC]; R.total(tot); rec_add_lds(S, A, acc_l, tot); }
                    R.clear();
                    acc_l = first;
                }
                R.full += (uint32_t)VPL;
                todo &= 1u << VPL;                 // (the block at N2 is never whole)
            }
            if (todo) {
#pragma unroll
                for (int j = 0; j <= VPL; ++j) {
                    if (!((todo >> j) & 1u)) continue;
                    uint32_t x[8];
#pragma unroll
                    for (int b = 0; b < 8; ++b) x[b] = (b & 4 ? hi : lo).at((b >> 1) & 1, j + (b & 1));
                    uint32_t diff = 0u;
#pragma unroll
                    for (int b = 1; b < 8; ++b) diff |= x[b] ^ x[0];
                    if (diff == 0u) {
                        if (x[0] == INVALID_LABEL) continue;
                        if (x[0] != acc_l) {
                            if (acc_l != INVALID_LABEL) { uint32_t tot[TP_NC]; R.total(tot); rec_add_lds(S, A, acc_l, tot); }
                            R.clear();
                            acc_l = x[0];
                        }
                        R.full += 1u;
                        continue;
                    }
                    uint32_t left = 0u;            // voxels whose label has not been taken yet
#pragma unroll
                    for (int b = 0; b < 8; ++b) left |= (x[b] != INVALID_LABEL ? 1u : 0u) << b;
                    int distinct = 0;
                    while (left) {
                        const uint32_t l = smallest_left(x, left);         // (ascending: no register is indexed)
                        uint32_t m = 0u;
#pragma unroll
                        for (int b = 0; b < 8; ++b) m |= (x[b] == l ? 1u : 0u) << b;
                        left &= ~m;
                        ++distinct;
                        uint32_t c[TP_NC];
                        mask_counts(m, c);
                        if (l == acc_l) {
#pragma unroll
                            for (int i = 0; i < TP_NC; ++i) R.c[i] += c[i];
                        } else {
                            rec_add_lds(S, A, l, c);
                        }
                    }
                    if (distinct > 1) nmixed += 1u;
                }
            }
            lo = hi;
            lo_diff = hi_diff;
            if (more) hi = nx;
        }
    }

    // the lanes' last records: reduced across the wave one label at a time, the first lane of the label adds them to the table
    for (;;) {
        const uint64_t pending = __ballot(acc_l != INVALID_LABEL);
        if (!pending) break;
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const uint32_t L = (uint32_t)__shfl((int)acc_l, leader);
        const bool mine = acc_l == L;
        uint32_t X[TP_NC];
#pragma unroll
        for (int i = 0; i < TP_NC; ++i) X[i] = mine ? R.c[i] + R.full : 0u;
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int i = 0; i < TP_NC; ++i) X[i] += (uint32_t)__shfl_xor((int)X[i], o);
        }
        if (lane == leader) rec_add_lds(S, A, L, X);
        if (mine) acc_l = INVALID_LABEL;
    }
    for (int o = 32; o > 0; o >>= 1) nmixed += (uint32_t)__shfl_xor((int)nmixed, o);
    if (lane == 0 && nmixed) atomicAdd(A.mixed, (unsigned long long)nmixed);
    __syncthreads();
    for (int i = tid; i < TP_SLOTS; i += TP_THREADS) {
        const uint32_t l = S.key[i];
        if (l == INVALID_LABEL) continue;
        Counts C;
#pragma unroll
        for (int k = 0; k < TP_NC; ++k) C.c[k] = S.c[k][i];
        rec_add_global(A, l, C);
    }
}

template <typename E>
void launch_type(hipStream_t s, const TopologyArgs& a, bool vec, uint32_t groups) {
    if (vec) hipLaunchKernelGGL((topology_kernel<E, true>), dim3(groups), dim3(TP_THREADS), 0, s, a);
    else hipLaunchKernelGGL((topology_kernel<E, false>), dim3(groups), dim3(TP_THREADS), 0, s, a);
}

}  // namespace

RangePlan topology_plan(const int64_t dims[3], int label_itemsize) {
    if (dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0) return RangePlan();
    const RangeTiles t = range_tiles(dims[0] + 1, dims[1] + 1, dims[2], 0, label_itemsize, TP_RANGE);
    return plan_ranges(t.tiles, t.tile_voxels, TP_RANGE);
}

void launch_topology(hipStream_t s, TopologyArgs a, int label_itemsize, const RangePlan& plan) {
    if (!plan.groups) return;
    a.tiles_per_group = plan.tiles_per_group;
    const bool vec = strips_vectorize(a.n2, label_itemsize, {{a.vol, label_itemsize}});
    if (label_itemsize == 2) launch_type<uint16_t>(s, a, vec, plan.groups);
    else launch_type<uint32_t>(s, a, vec, plan.groups);
}

}  // namespace ta
