// kernels_sigmoments.hip -- signal-weighted moments per label (include/tissue_scan_sigmoments.h): n, w = sum S, m1 = sum S x_k and
// m2 = sum S x_j x_k of an intensity image over the resident label volume, in one streaming pass over labels + signal.
//
// Layout of the pass: that of the per-label half of kernels_signal.hip.  A tile is SM_WAVES rows x (64 lanes x VPL columns) x
// SM_PLANES planes; every wave owns one row of it and walks the planes, each lane holding a strip of VPL = 16 / sizeof(label)
// voxels along memory axis 2.  The next plane's strips are loaded while the current one is worked on.  A workgroup takes a
// contiguous range of tiles and keeps one LDS table label -> (n, w, m1[3], m2[6]) for the whole range, which it flushes with
// global atomics once, at its end.
//
// The closed form.  Inside a tile a lane's row r and column base c0 are fixed and the plane is P0 + q, q < SM_PLANES.  So a voxel
// of column c0 + j costs three 32-bit operations, on the plane step's  w += s, a += j s, b += j^2 s  (j is a constant of the
// unrolled strip), and a plane step three more multiplies, on the tile record
//     W += w   Q += q w   QQ += q^2 w   A += a   QA += q a   B += b
// all of which fit 32 bits (static_asserts below).  The tile record is unfolded into the lane's running record of absolute 64-bit
// sums (fold_tile: x0 = P0 + q, x1 = r, x2 = c0 + j multiplied out) when the label changes or the tile ends, and the running record
// goes to the LDS table only when the label changes; the lanes' last records are reduced across the wave label by label.
//
// Widths.  All sums are integers: the results are bit-exact whatever the order of the atomics.  m2 is 128-bit in global memory:
// the add to the low word returns the old value, and an add that wraps it carries one into the high word.  The running record and
// the LDS rows are 64-bit: every one of them is a sum of non-negative terms over voxels of ONE workgroup, at most
// voxels x g^2 x smax with g the largest coordinate, and sigmoments_plan gives a workgroup no more voxels than keep that below
// 2^64 (and refuses dims at which one tile is too many).  n is u32 in the LDS row under the 2^31-voxel cap of the other passes.
#include "ta_sigmoments.h"

#include <algorithm>

namespace ta {
namespace {

constexpr int SM_WAVES = 4;                        // rows of a tile = waves of a workgroup
constexpr int SM_THREADS = SM_WAVES * 64;
constexpr int SM_PLANES = 16;                      // planes of a tile
constexpr int SM_PROBE = 32;                       // probes before a record goes to the global rows directly
// n is u32 in a workgroup's LDS row: fewer than 2^31 voxels a workgroup (sigmoments_plan adds the cap that keeps the 64-bit sums exact)
constexpr RangeShape SM_RANGE = {SM_WAVES, SM_PLANES, SM_MAX_GROUPS, 31};

// the 32-bit tile record at its largest: 8 voxels of 65535 a plane step, q <= 15, j <= 7
static_assert(65535ull * 8 * (SM_PLANES - 1) * (SM_PLANES - 1) * SM_PLANES < (1ull << 32), "QQ wraps");
static_assert(65535ull * (7 * 8 / 2) * (SM_PLANES - 1) * SM_PLANES < (1ull << 32), "QA wraps");
static_assert(65535ull * (7 * 8 * 15 / 6) * SM_PLANES < (1ull << 32), "B wraps");

struct MomTable {
    uint32_t key[SM_SLOTS], n[SM_SLOTS];
    unsigned long long w[SM_SLOTS], m1[3][SM_SLOTS], m2[6][SM_SLOTS];
};
static_assert(sizeof(MomTable) == 88 * SM_SLOTS && 4 * sizeof(MomTable) <= 160 * 1024, "four workgroups a CU");

// a lane's running record: absolute sums of the voxels of one label
struct Rec {
    uint32_t n;
    uint64_t w, m1[3], m2[6];
    __device__ __forceinline__ void clear() {
        n = 0u; w = 0ull;
#pragma unroll
        for (int k = 0; k < 3; ++k) m1[k] = 0ull;
#pragma unroll
        for (int k = 0; k < 6; ++k) m2[k] = 0ull;
    }
};

// the voxels of one label in one tile, relative to the tile's first plane and the lane's first column
struct TileRec {
    uint32_t n, W, Q, QQ, A, QA, B;
    __device__ __forceinline__ void clear() { n = W = Q = QQ = A = QA = B = 0u; }
    __device__ __forceinline__ void step(uint32_t q, uint32_t sn, uint32_t w, uint32_t a, uint32_t b) {
        n += sn; W += w; Q += q * w; QQ += q * q * w; A += a; QA += q * a; B += b;
    }
};

// R += T with x0 = P0 + q, x1 = r, x2 = c0 + j multiplied out
__device__ __forceinline__ void fold_tile(Rec& R, const TileRec& T, uint64_t P0, uint64_t r, uint64_t c0) {
    const uint64_t W = T.W, A = T.A;
    const uint64_t sp = P0 * W + T.Q;                          // sum of S x0
    const uint64_t sc = c0 * W + A;                            // sum of S x2
    R.n += T.n;
    R.w += W;
    R.m1[0] += sp; R.m1[1] += r * W; R.m1[2] += sc;
    R.m2[0] += P0 * (sp + T.Q) + T.QQ;                         // P0^2 W + 2 P0 Q + QQ
    R.m2[1] += r * sp;
    R.m2[2] += c0 * sp + P0 * A + T.QA;                        // P0 c0 W + c0 Q + P0 A + QA
    R.m2[3] += r * r * W;
    R.m2[4] += r * sc;
    R.m2[5] += c0 * (sc + A) + T.B;                            // c0^2 W + 2 c0 A + B
}

__device__ void rec_add_global(const SigMomArgs& A, uint32_t l, uint64_t n, uint64_t w, const uint64_t (&m1)[3], const uint64_t (&m2)[6]) {
    if (l > A.max_label) { atomicOr(&A.flags[SM_FLAG_RANGE], 1u); return; }
    atomicAdd(&A.n[l], (unsigned long long)n);
    atomicAdd(&A.w[l], (unsigned long long)w);
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(&A.m1[3 * (uint64_t)l + k], (unsigned long long)m1[k]);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        unsigned long long* lo = &A.m2[2 * (6 * (uint64_t)l + k)];
        const unsigned long long old = atomicAdd(lo, (unsigned long long)m2[k]);
        if (old + m2[k] < old) atomicAdd(lo + 1, 1ull);        // the low word wrapped: carry
    }
}

__device__ __forceinline__ void rec_add_lds(MomTable& S, const SigMomArgs& A, uint32_t l, const Rec& R) {
    uint32_t h = __umulhi(hash_u32(l), (uint32_t)SM_SLOTS);
    for (int probe = 0; probe < SM_PROBE; ++probe) {
        const uint32_t k = atomicCAS(&S.key[h], INVALID_LABEL, l);
        if (k == INVALID_LABEL || k == l) {
            atomicAdd(&S.n[h], R.n);
            atomicAdd(&S.w[h], (unsigned long long)R.w);
#pragma unroll
            for (int i = 0; i < 3; ++i) atomicAdd(&S.m1[i][h], (unsigned long long)R.m1[i]);
#pragma unroll
            for (int i = 0; i < 6; ++i) atomicAdd(&S.m2[i][h], (unsigned long long)R.m2[i]);
            return;
        }
        h = h + 1 == (uint32_t)SM_SLOTS ? 0u : h + 1;
    }
    atomicAdd(&A.flags[SM_FLAG_SPILL], 1u);
    rec_add_global(A, l, R.n, R.w, R.m1, R.m2);
}

template <int BYTES> struct VecOf;
template <> struct VecOf<4> { typedef uint32_t T; };
template <> struct VecOf<8> { typedef uint2 T; };
template <> struct VecOf<16> { typedef uint4 T; };

// N consecutive elements of E from an address aligned to N * sizeof(E): one load of 4, 8 or 16 bytes
template <typename E, int N>
__device__ __forceinline__ void load_vec(const E* p, uint32_t (&out)[N]) {
    constexpr int BYTES = N * (int)sizeof(E);
    typedef typename VecOf<BYTES>::T V;
    const V v = *reinterpret_cast<const V*>(p);
    uint32_t w[BYTES / 4];
    __builtin_memcpy(w, &v, BYTES);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (sizeof(E) == 4) out[j] = w[j];
        else if (sizeof(E) == 2) out[j] = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        else out[j] = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
    }
}

// the strip of row r of plane p that starts at column c0: labels (INVALID_LABEL past the row's end) and signal.  VEC: every strip
// is whole or wholly outside the row (n2 % VPL == 0) and both buffers are aligned for the vector loads.
template <typename TL, typename TS, int VPL, bool VEC>
__device__ __forceinline__ void load_strip(const SigMomArgs& A, int64_t p, int64_t r, int64_t c0, uint32_t (&l)[VPL], uint32_t (&s)[VPL]) {
    const int64_t base = (p * A.n1 + r) * A.n2 + c0;
    if (VEC) {
        if (c0 < A.n2) {
            load_vec<TL, VPL>((const TL*)A.vol + base, l);
            load_vec<TS, VPL>((const TS*)A.sig + base, s);
        } else {
#pragma unroll
            for (int j = 0; j < VPL; ++j) { l[j] = INVALID_LABEL; s[j] = 0u; }
        }
    } else {
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const bool in = c0 + j < A.n2;
            l[j] = in ? (uint32_t)((const TL*)A.vol)[base + j] : INVALID_LABEL;
            s[j] = in ? (uint32_t)((const TS*)A.sig)[base + j] : 0u;
        }
    }
}

template <typename TL, typename TS, bool VEC>
__global__ __launch_bounds__(SM_THREADS) void sigmoments_kernel(const SigMomArgs A) {
    constexpr int VPL = 16 / (int)sizeof(TL);
    __shared__ MomTable S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < SM_SLOTS; i += SM_THREADS) {
        S.key[i] = INVALID_LABEL; S.n[i] = 0u; S.w[i] = 0ull;
#pragma unroll
        for (int k = 0; k < 3; ++k) S.m1[k][i] = 0ull;
#pragma unroll
        for (int k = 0; k < 6; ++k) S.m2[k][i] = 0ull;
    }
    __syncthreads();

    const int64_t cols = 64 * VPL;
    const int64_t ncb = (A.n2 + cols - 1) / cols, nrb = (A.n1 + SM_WAVES - 1) / SM_WAVES;
    const int64_t npb = (A.n0 - A.first_owned + SM_PLANES - 1) / SM_PLANES;
    const int64_t tiles = ncb * nrb * npb;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_group;
    const int64_t t1 = t0 + A.tiles_per_group < tiles ? t0 + A.tiles_per_group : tiles;

    uint32_t acc_l = INVALID_LABEL;                                // the label of the lane's running record
    Rec R;
    R.clear();

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t cb = t % ncb, rb = (t / ncb) % nrb, pb = t / (ncb * nrb);
        const int64_t r = rb * SM_WAVES + wave;
        if (r >= A.n1) continue;                                   // (wave-uniform)
        const int64_t c0 = cb * cols + (int64_t)lane * VPL;
        const int64_t pbeg = A.first_owned + pb * SM_PLANES;
        const int64_t pend = pbeg + SM_PLANES < A.n0 ? pbeg + SM_PLANES : A.n0;
        const uint64_t P0 = (uint64_t)(pb * SM_PLANES);           // x0 of the tile's first plane: counted from the first owned plane
        TileRec T;
        T.clear();
        uint32_t cl[VPL], cs[VPL];                                 // this plane
        load_strip<TL, TS, VPL, VEC>(A, pbeg, r, c0, cl, cs);
        for (int64_t p = pbeg; p < pend; ++p) {
            const bool more = p + 1 < pend;                        // (wave-uniform)
            uint32_t nl[VPL], ns[VPL];                             // the next plane, in flight while this one is worked on
            if (more) load_strip<TL, TS, VPL, VEC>(A, p + 1, r, c0, nl, ns);
            const uint32_t q = (uint32_t)(p - pbeg);
            uint32_t sn = 0u, w = 0u, a = 0u, b = 0u;              // this plane step, this label
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const uint32_t x = cl[j], s = cs[j];
                if (x == INVALID_LABEL) continue;
                if (x != acc_l) {
                    T.step(q, sn, w, a, b);
                    sn = w = a = b = 0u;
                    if (T.n) fold_tile(R, T, P0, (uint64_t)r, (uint64_t)c0);
                    T.clear();
                    if (acc_l != INVALID_LABEL) rec_add_lds(S, A, acc_l, R);
                    R.clear();
                    acc_l = x;
                }
                sn += 1u; w += s; a += (uint32_t)j * s; b += (uint32_t)(j * j) * s;
            }
            T.step(q, sn, w, a, b);
            if (more) {
#pragma unroll
                for (int j = 0; j < VPL; ++j) { cl[j] = nl[j]; cs[j] = ns[j]; }
            }
        }
        if (T.n) fold_tile(R, T, P0, (uint64_t)r, (uint64_t)c0);
    }

    // the lanes' last records: reduced across the wave one label at a time, the first lane of the label adds them to the table
    for (;;) {
        const uint64_t pending = __ballot(acc_l != INVALID_LABEL);
        if (!pending) break;
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const uint32_t L = (uint32_t)__shfl((int)acc_l, leader);
        const bool mine = acc_l == L;
        Rec X;
        X.clear();
        if (mine) X = R;
        for (int o = 32; o > 0; o >>= 1) {
            X.n += (uint32_t)__shfl_xor((int)X.n, o);
            X.w += __shfl_xor(X.w, o);
#pragma unroll
            for (int k = 0; k < 3; ++k) X.m1[k] += __shfl_xor(X.m1[k], o);
#pragma unroll
            for (int k = 0; k < 6; ++k) X.m2[k] += __shfl_xor(X.m2[k], o);
        }
        if (lane == leader) rec_add_lds(S, A, L, X);
        if (mine) acc_l = INVALID_LABEL;
    }
    __syncthreads();
    for (int i = tid; i < SM_SLOTS; i += SM_THREADS) {
        const uint32_t l = S.key[i];
        if (l == INVALID_LABEL) continue;
        const uint64_t m1[3] = {S.m1[0][i], S.m1[1][i], S.m1[2][i]};
        const uint64_t m2[6] = {S.m2[0][i], S.m2[1][i], S.m2[2][i], S.m2[3][i], S.m2[4][i], S.m2[5][i]};
        rec_add_global(A, l, S.n[i], S.w[i], m1, m2);
    }
}

template <typename TL, typename TS>
void launch_types(hipStream_t s, const SigMomArgs& a, bool vec, uint32_t groups) {
    if (vec) hipLaunchKernelGGL((sigmoments_kernel<TL, TS, true>), dim3(groups), dim3(SM_THREADS), 0, s, a);
    else hipLaunchKernelGGL((sigmoments_kernel<TL, TS, false>), dim3(groups), dim3(SM_THREADS), 0, s, a);
}

}  // namespace

int sigmoments_plan(const int64_t dims[3], int first_owned, int label_itemsize, int signal_itemsize, RangePlan* plan) {
    typedef unsigned __int128 u128;
    *plan = RangePlan();
    const RangeTiles t = range_tiles(dims[0], dims[1], dims[2], first_owned, label_itemsize, SM_RANGE);
    if (!t.tiles) return 0;
    const uint64_t gmax = (uint64_t)std::max(dims[0], std::max(dims[1], dims[2]));
    const uint64_t g = std::max<uint64_t>(gmax - 1, 1), smax = signal_itemsize == 1 ? 255u : 65535u;
    const u128 two64 = (u128)1 << 64;
    // the u64 first moments: nvox g smax < 2^64
    const u128 nvox = (u128)((uint64_t)dims[0] * (uint64_t)dims[1]) * (uint64_t)dims[2];       // (every dim <= 2^30)
    if (nvox > (two64 - 1) / (u128)(g * smax)) return 1;
    // a workgroup's 64-bit rows: voxels g^2 smax <= 2^64 (never equal: smax is odd), beside the u32 n
    const u128 exact = two64 / ((u128)g * g * smax) / (u128)t.tile_voxels;
    *plan = plan_ranges(t.tiles, t.tile_voxels, SM_RANGE, (int64_t)std::min<u128>(exact, (u128)INT64_MAX));
    return plan->groups ? 0 : 2;                               // (no group: not one tile fits)
}

void launch_sigmoments(hipStream_t s, SigMomArgs a, int label_itemsize, int signal_itemsize, const RangePlan& plan) {
    if (!plan.groups) return;
    a.tiles_per_group = plan.tiles_per_group;
    const bool vec = strips_vectorize(a.n2, label_itemsize, {{a.vol, label_itemsize}, {a.sig, signal_itemsize}});
    if (label_itemsize == 2 && signal_itemsize == 1) launch_types<uint16_t, uint8_t>(s, a, vec, plan.groups);
    else if (label_itemsize == 2) launch_types<uint16_t, uint16_t>(s, a, vec, plan.groups);
    else if (signal_itemsize == 1) launch_types<uint32_t, uint8_t>(s, a, vec, plan.groups);
    else launch_types<uint32_t, uint16_t>(s, a, vec, plan.groups);
}

}  // namespace ta
