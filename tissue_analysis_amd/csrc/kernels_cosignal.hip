// kernels_cosignal.hip -- the joint sums per label of two intensity images A and B over the resident label volume
// (include/tissue_scan_cosignal.h): n, sum A, sum B, sum A^2, sum B^2, sum A B, the voxels over a threshold in A, in B and in both,
// and the sum of each channel over the voxels where the other one is over its threshold -- in one streaming pass over labels + A + B.
//
// Layout of the pass: that of the per-label half of kernels_signal.hip.  A tile is CO_WAVES rows x (64 lanes x VPL columns) x
// CO_PLANES planes; every wave owns one row of it and walks the planes, each lane holding a strip of VPL = 16 / sizeof(label)
// voxels along memory axis 2 (16 bytes of labels a lane, and as many values of A and of B).  The next plane's strips are loaded
// while the current one is worked on.  A workgroup takes a contiguous range of tiles and keeps one LDS table label -> record for
// the whole range, which it flushes with global atomics once, at its end.  A lane folds its voxels into ONE running record for as
// long as the label does not change -- along its strip, from plane to plane and from tile to tile -- and hands it to the LDS
// table only when it does; the lanes' last records are reduced across the wave label by label before they go to the table.  A
// record that finds no slot within CO_PROBE probes goes to the global rows directly and is counted in COSIG_FLAG_SPILL.
//
// Widths.  All sums are integers: the results are bit-exact whatever the order of the atomics.  A value is at most 65535, so a
// product is below 2^32.  A workgroup walks fewer than 2^31 voxels (CO_RANGE's cap, which plan_ranges keeps): its u32 counts
// cannot wrap, and its u64 sums of products stay below 2^31 x 2^32 = 2^63 < 2^64 -- in the lane's running record and in the LDS
// rows alike.  The sums of one strip of a plane (at most 8 voxels: 8 x 65535 < 2^32) are 32-bit until the strip ends.  In global
// memory the three sums of products are 128-bit: the add to the low word returns the old value, and an add that wraps it carries
// one into the high word.  The other columns are u64, as n and sum of the signal pass are.
#include "ta_cosignal.h"

namespace ta {
namespace {

constexpr int CO_WAVES = 4;                        // rows of a tile = waves of a workgroup
constexpr int CO_THREADS = CO_WAVES * 64;
constexpr int CO_PLANES = 16;                      // planes of a tile
constexpr int CO_PROBE = 32;                       // probes before a record goes to the global rows directly
// a workgroup's LDS rows count voxels in u32 and sum products below 2^32 in u64: fewer than 2^31 voxels a workgroup
constexpr RangeShape CO_RANGE = {CO_WAVES, CO_PLANES, COSIG_MAX_GROUPS, 31};
static_assert((COSIG_SLOTS & (COSIG_SLOTS - 1)) == 0, "the home slot is hash & (slots - 1)");

struct CoTable {
    unsigned long long sa[COSIG_SLOTS], sb[COSIG_SLOTS], qaa[COSIG_SLOTS], qbb[COSIG_SLOTS], qab[COSIG_SLOTS], oa[COSIG_SLOTS], ob[COSIG_SLOTS];
    uint32_t key[COSIG_SLOTS], n[COSIG_SLOTS], na[COSIG_SLOTS], nb[COSIG_SLOTS], nab[COSIG_SLOTS];
};
static_assert(sizeof(CoTable) == 76 * COSIG_SLOTS && 4 * sizeof(CoTable) <= 160 * 1024, "four workgroups a CU");

// the voxels of one label in one strip of one plane: 32-bit
struct Step {
    uint32_t n, na, nb, nab, sa, sb, oa, ob;
    __device__ __forceinline__ void clear() { n = na = nb = nab = sa = sb = oa = ob = 0u; }
};

// a lane's running record: the voxels of one label
struct Rec {
    uint32_t n, na, nb, nab;
    uint64_t sa, sb, qaa, qbb, qab, oa, ob;
    __device__ __forceinline__ void clear() { n = na = nb = nab = 0u; sa = sb = qaa = qbb = qab = oa = ob = 0ull; }
    __device__ __forceinline__ void add(const Step& t) {
        n += t.n; na += t.na; nb += t.nb; nab += t.nab; sa += t.sa; sb += t.sb; oa += t.oa; ob += t.ob;
    }
};

__device__ __forceinline__ void wide_add_global(unsigned long long* lo, uint64_t q) {
    const unsigned long long old = atomicAdd(lo, (unsigned long long)q);
    if (old + q < old) atomicAdd(lo + 1, 1ull);                // the low word wrapped: carry
}

__device__ void rec_add_global(const CoSigArgs& A, uint32_t l, uint64_t n, uint64_t na, uint64_t nb, uint64_t nab, uint64_t sa, uint64_t sb,
                               uint64_t qaa, uint64_t qbb, uint64_t qab, uint64_t oa, uint64_t ob) {
    if (l > A.max_label) { atomicOr(&A.flags[COSIG_FLAG_RANGE], 1u); return; }
    atomicAdd(&A.n[l], (unsigned long long)n);
    atomicAdd(&A.sum_a[l], (unsigned long long)sa);
    atomicAdd(&A.sum_b[l], (unsigned long long)sb);
    wide_add_global(&A.sq_aa[2 * (uint64_t)l], qaa);
    wide_add_global(&A.sq_bb[2 * (uint64_t)l], qbb);
    wide_add_global(&A.sq_ab[2 * (uint64_t)l], qab);
    if (na) atomicAdd(&A.n_a[l], (unsigned long long)na);
    if (nb) atomicAdd(&A.n_b[l], (unsigned long long)nb);
    if (nab) atomicAdd(&A.n_ab[l], (unsigned long long)nab);
    if (oa) atomicAdd(&A.over_a[l], (unsigned long long)oa);
    if (ob) atomicAdd(&A.over_b[l], (unsigned long long)ob);
}

__device__ __forceinline__ void rec_add_lds(CoTable& S, const CoSigArgs& A, uint32_t l, const Rec& R) {
    uint32_t h = hash_u32(l) & (COSIG_SLOTS - 1);
    for (int probe = 0; probe < CO_PROBE; ++probe) {
        const uint32_t k = atomicCAS(&S.key[h], INVALID_LABEL, l);
        if (k == INVALID_LABEL || k == l) {
            atomicAdd(&S.n[h], R.n);
            atomicAdd(&S.na[h], R.na);
            atomicAdd(&S.nb[h], R.nb);
            atomicAdd(&S.nab[h], R.nab);
            atomicAdd(&S.sa[h], (unsigned long long)R.sa);
            atomicAdd(&S.sb[h], (unsigned long long)R.sb);
            atomicAdd(&S.qaa[h], (unsigned long long)R.qaa);
            atomicAdd(&S.qbb[h], (unsigned long long)R.qbb);
            atomicAdd(&S.qab[h], (unsigned long long)R.qab);
            atomicAdd(&S.oa[h], (unsigned long long)R.oa);
            atomicAdd(&S.ob[h], (unsigned long long)R.ob);
            return;
        }
        h = (h + 1) & (COSIG_SLOTS - 1);
    }
    atomicAdd(&A.flags[COSIG_FLAG_SPILL], 1u);
    rec_add_global(A, l, R.n, R.na, R.nb, R.nab, R.sa, R.sb, R.qaa, R.qbb, R.qab, R.oa, R.ob);
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

// the strip of row r of plane p that starts at column c0: labels (INVALID_LABEL past the row's end), A and B.  VEC: every strip is
// whole or wholly outside the row (n2 % VPL == 0) and the three buffers are aligned for the vector loads.
template <typename TL, typename TA, typename TB, int VPL, bool VEC>
__device__ __forceinline__ void load_strip(const CoSigArgs& A, int64_t p, int64_t r, int64_t c0, uint32_t (&l)[VPL], uint32_t (&a)[VPL],
                                           uint32_t (&b)[VPL]) {
    const int64_t base = (p * A.n1 + r) * A.n2 + c0;
    if (VEC) {
        if (c0 < A.n2) {
            load_vec<TL, VPL>((const TL*)A.vol + base, l);
            load_vec<TA, VPL>((const TA*)A.a + base, a);
            load_vec<TB, VPL>((const TB*)A.b + base, b);
        } else {
#pragma unroll
            for (int j = 0; j < VPL; ++j) { l[j] = INVALID_LABEL; a[j] = 0u; b[j] = 0u; }
        }
    } else {
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const bool in = c0 + j < A.n2;
            l[j] = in ? (uint32_t)((const TL*)A.vol)[base + j] : INVALID_LABEL;
            a[j] = in ? (uint32_t)((const TA*)A.a)[base + j] : 0u;
            b[j] = in ? (uint32_t)((const TB*)A.b)[base + j] : 0u;
        }
    }
}

template <typename TL, typename TA, typename TB, bool VEC>
__global__ __launch_bounds__(CO_THREADS) void cosignal_kernel(const CoSigArgs A) {
    constexpr int VPL = 16 / (int)sizeof(TL);
    __shared__ CoTable S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < COSIG_SLOTS; i += CO_THREADS) {
        S.key[i] = INVALID_LABEL; S.n[i] = 0u; S.na[i] = 0u; S.nb[i] = 0u; S.nab[i] = 0u;
        S.sa[i] = 0ull; S.sb[i] = 0ull; S.qaa[i] = 0ull; S.qbb[i] = 0ull; S.qab[i] = 0ull; S.oa[i] = 0ull; S.ob[i] = 0ull;
    }
    __syncthreads();

    const int64_t cols = 64 * VPL;
    const int64_t ncb = (A.n2 + cols - 1) / cols, nrb = (A.n1 + CO_WAVES - 1) / CO_WAVES;
    const int64_t npb = (A.n0 - A.first_owned + CO_PLANES - 1) / CO_PLANES;
    const int64_t tiles = ncb * nrb * npb;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_group;
    const int64_t t1 = t0 + A.tiles_per_group < tiles ? t0 + A.tiles_per_group : tiles;
    const uint32_t thr_a = A.thr_a, thr_b = A.thr_b;

    uint32_t acc_l = INVALID_LABEL;                                // the label of the lane's running record
    Rec R;
    R.clear();

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t cb = t % ncb, rb = (t / ncb) % nrb, pb = t / (ncb * nrb);
        const int64_t r = rb * CO_WAVES + wave;
        if (r >= A.n1) continue;                                   // (wave-uniform)
        const int64_t c0 = cb * cols + (int64_t)lane * VPL;
        const int64_t pbeg = A.first_owned + pb * CO_PLANES;
        const int64_t pend = pbeg + CO_PLANES < A.n0 ? pbeg + CO_PLANES : A.n0;
        uint32_t cl[VPL], ca[VPL], cbv[VPL];                       // this plane
        load_strip<TL, TA, TB, VPL, VEC>(A, pbeg, r, c0, cl, ca, cbv);
        for (int64_t p = pbeg; p < pend; ++p) {
            const bool more = p + 1 < pend;                        // (wave-uniform)
            uint32_t nl[VPL], na[VPL], nb[VPL];                    // the next plane, in flight while this one is worked on
            if (more) load_strip<TL, TA, TB, VPL, VEC>(A, p + 1, r, c0, nl, na, nb);
            Step T;                                                // this strip, this label
            T.clear();
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const uint32_t x = cl[j], a = ca[j], b = cbv[j];
                if (x == INVALID_LABEL) continue;
                if (x != acc_l) {
                    R.add(T);
                    T.clear();
                    if (acc_l != INVALID_LABEL) rec_add_lds(S, A, acc_l, R);
                    R.clear();
                    acc_l = x;
                }
                const bool ia = a > thr_a, ib = b > thr_b;
                T.n += 1u; T.sa += a; T.sb += b;
                T.na += ia ? 1u : 0u; T.nb += ib ? 1u : 0u; T.nab += (ia && ib) ? 1u : 0u;
                T.oa += ib ? a : 0u; T.ob += ia ? b : 0u;
                // (values below 2^16: the 24-bit multiply is exact; it is declared int, so to u32 first -- a product can pass 2^31)
                R.qaa += (uint64_t)(uint32_t)__umul24(a, a); R.qbb += (uint64_t)(uint32_t)__umul24(b, b); R.qab += (uint64_t)(uint32_t)__umul24(a, b);
            }
            R.add(T);
            if (more) {
#pragma unroll
                for (int j = 0; j < VPL; ++j) { cl[j] = nl[j]; ca[j] = na[j]; cbv[j] = nb[j]; }
            }
        }
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
            X.na += (uint32_t)__shfl_xor((int)X.na, o);
            X.nb += (uint32_t)__shfl_xor((int)X.nb, o);
            X.nab += (uint32_t)__shfl_xor((int)X.nab, o);
            X.sa += __shfl_xor(X.sa, o); X.sb += __shfl_xor(X.sb, o);
            X.qaa += __shfl_xor(X.qaa, o); X.qbb += __shfl_xor(X.qbb, o); X.qab += __shfl_xor(X.qab, o);
            X.oa += __shfl_xor(X.oa, o); X.ob += __shfl_xor(X.ob, o);
        }
        if (lane == leader) rec_add_lds(S, A, L, X);
        if (mine) acc_l = INVALID_LABEL;
    }
    __syncthreads();
    for (int i = tid; i < COSIG_SLOTS; i += CO_THREADS) {
        const uint32_t l = S.key[i];
        if (l != INVALID_LABEL) rec_add_global(A, l, S.n[i], S.na[i], S.nb[i], S.nab[i], S.sa[i], S.sb[i], S.qaa[i], S.qbb[i], S.qab[i], S.oa[i], S.ob[i]);
    }
}

template <typename TL, typename TA, typename TB>
void launch_vec(hipStream_t s, const CoSigArgs& a, bool vec, uint32_t groups) {
    if (vec) hipLaunchKernelGGL((cosignal_kernel<TL, TA, TB, true>), dim3(groups), dim3(CO_THREADS), 0, s, a);
    else hipLaunchKernelGGL((cosignal_kernel<TL, TA, TB, false>), dim3(groups), dim3(CO_THREADS), 0, s, a);
}

template <typename TL>
void launch_types(hipStream_t s, const CoSigArgs& a, int a_itemsize, int b_itemsize, bool vec, uint32_t groups) {
    if (a_itemsize == 1 && b_itemsize == 1) launch_vec<TL, uint8_t, uint8_t>(s, a, vec, groups);
    else if (a_itemsize == 1) launch_vec<TL, uint8_t, uint16_t>(s, a, vec, groups);
    else if (b_itemsize == 1) launch_vec<TL, uint16_t, uint8_t>(s, a, vec, groups);
    else launch_vec<TL, uint16_t, uint16_t>(s, a, vec, groups);
}

}  // namespace

RangePlan launch_cosignal(hipStream_t s, CoSigArgs a, int label_itemsize, int a_itemsize, int b_itemsize) {
    const RangeTiles t = range_tiles(a.n0, a.n1, a.n2, a.first_owned, label_itemsize, CO_RANGE);
    const RangePlan plan = plan_ranges(t.tiles, t.tile_voxels, CO_RANGE);
    if (!plan.groups) return plan;
    a.tiles_per_group = plan.tiles_per_group;
    const bool vec = strips_vectorize(a.n2, label_itemsize, {{a.vol, label_itemsize}, {a.a, a_itemsize}, {a.b, b_itemsize}});
    if (label_itemsize == 2) launch_types<uint16_t>(s, a, a_itemsize, b_itemsize, vec, plan.groups);
    else launch_types<uint32_t>(s, a, a_itemsize, b_itemsize, vec, plan.groups);
    return plan;
}

}  // namespace ta
