// kernels_profile.hip -- distance-shell profiles (include/tissue_scan_profile.h): per (label, shell of squared distance) the voxels
// and the statistics of the signal image, in one streaming pass over labels + D2 (+ signal).
//
// Layout of the pass: the tile shape and the walk of kernels_signal.hip.  A tile is PRF_WAVES rows x (64 lanes x VPL columns) x
// PRF_PLANES planes; every wave owns one row of it and walks the planes, each lane holding a strip of VPL = 16 / sizeof(label)
// voxels along memory axis 2: 16 bytes of labels, the VPL doubles of D2 behind them (two or four 16-byte loads) and as many signal
// values.  The next plane's strips are loaded while the current one is worked on.  A workgroup takes a contiguous range of tiles
// (ceil(tiles / 4096) of them, the launch plan of kernels_wallgeo.hip: with 1024 workgroups a range of C4 held more keys than
// the table has slots) and keeps ONE LDS table for the whole range, key = row * K + shell -> (n, sum, sum of
// squares, min, max), which it flushes with global atomics once, at its end; a record that finds no slot within PRF_PROBE probes
// goes to the global rows directly and is counted.
//   shells: the edges lie in LDS, K + 1 of them and +inf behind, 65 in all.  A lane keeps the two edges around its previous voxel
//     in registers and tests them first: inside a cell D2 changes slowly along a row, so most voxels stay in the shell before.
//     Otherwise six steps of a binary search, each one LDS read and a select: the same instructions in every lane.
//   records: a lane folds its voxels into ONE running record (key, n, sum, sumsq, min, max) for as long as the key does not change
//     -- along its strip and from plane to plane -- and hands it to the LDS table only when it does; the lanes' last records are
//     reduced across the wave key by key before they go to the table.
// A label above max_label (the volume changed since ta_extract) raises PROF_FLAG_RANGE at its voxel, before a key is formed: every
// key that reaches a table is below rows * K.  All sums are integers and every comparison of doubles is exact: the results are
// bit-exact whatever the order of the atomics.  sumsq is 128-bit in global memory, with the carry rule of kernels_signal.hip: the
// add to the low word returns the old value, and an add that wraps it carries one into the high word.
// (The strip-load helpers are copies of those of kernels_signal.hip, by decision: the feature kernels share no code.)
#include "ta_profile.h"

#include <algorithm>

namespace ta {
namespace {

constexpr int PRF_WAVES = 4;                       // rows of a tile = waves of a workgroup
constexpr int PRF_THREADS = PRF_WAVES * 64;
constexpr int PRF_PLANES = 16;                     // planes of a tile
constexpr int PRF_PROBE = 32;                      // probes before a record goes to the global rows directly
constexpr int64_t PRF_MAX_GROUPS = 4096;           // 16 a CU, four of them resident: a range short enough for its keys to fit the table
// a workgroup's LDS rows count voxels in u32: 2^30 voxels a workgroup at most
constexpr RangeShape PRF_RANGE = {PRF_WAVES, PRF_PLANES, PRF_MAX_GROUPS, 30};
constexpr uint32_t NO_KEY = 0xffffffffu;           // rows * K <= 2^31: never a key
constexpr uint32_t NO_SIGNAL_MIN = 0xffffffffu;

// (a pass without signal keeps keys and counts only: 8.5 KB of LDS instead of 32.5)
template <bool SIG>
struct ProfTable {
    static constexpr int SS = SIG ? PROF_SLOTS : 1;
    double edge[PROF_MAX_BINS + 1];
    uint32_t key[PROF_SLOTS], n[PROF_SLOTS];
    uint32_t vmin[SS], vmax[SS];
    unsigned long long sum[SS], sq[SS];
};

template <bool SIG>
__device__ void add_global(const ProfileArgs& A, uint32_t key, uint64_t n, uint64_t s, uint64_t q, uint32_t mn, uint32_t mx) {
    atomicAdd(&A.n[key], (unsigned long long)n);
    if (SIG) {
        atomicAdd(&A.sum[key], (unsigned long long)s);
        const unsigned long long old = atomicAdd(&A.sumsq[2 * (uint64_t)key], (unsigned long long)q);
        if (old + q < old) atomicAdd(&A.sumsq[2 * (uint64_t)key + 1], 1ull);        // the low word wrapped: carry
        atomicMin(&A.vmin[key], mn);
        atomicMax(&A.vmax[key], mx);
    }
}

template <bool SIG>
__device__ __forceinline__ void add_lds(ProfTable<SIG>& S, const ProfileArgs& A, uint32_t key, uint32_t n, uint64_t s, uint64_t q,
                                        uint32_t mn, uint32_t mx) {
    uint32_t h = hash_u32(key) & (PROF_SLOTS - 1);
    for (int probe = 0; probe < PRF_PROBE; ++probe) {
        const uint32_t k = atomicCAS(&S.key[h], NO_KEY, key);
        if (k == NO_KEY || k == key) {
            atomicAdd(&S.n[h], n);
            if (SIG) {
                atomicAdd(&S.sum[h], (unsigned long long)s);
                atomicAdd(&S.sq[h], (unsigned long long)q);
                atomicMin(&S.vmin[h], mn);
                atomicMax(&S.vmax[h], mx);
            }
            return;
        }
        h = (h + 1) & (PROF_SLOTS - 1);
    }
    atomicAdd(&A.flags[PROF_FLAG_SPILL], 1u);
    add_global<SIG>(A, key, n, s, q, mn, mx);
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

// the signal type of an instantiation: SB = bytes of a signal value, 0 = a pass without signal (the type is not used then)
template <int SB> struct SigOf { typedef uint8_t T; };
template <> struct SigOf<2> { typedef uint16_t T; };

// the strip of row r of plane p that starts at column c0: labels (INVALID_LABEL past the row's end), D2 and signal.  VEC: every
// strip is whole or wholly outside the row (n2 % VPL == 0) and the buffers are aligned for the vector loads (D2 is the library's own
// allocation: a whole strip of it starts on a multiple of VPL * 8 >= 32 bytes).
template <typename TL, int SB, int VPL, bool VEC>
__device__ __forceinline__ void load_strip(const ProfileArgs& A, int64_t p, int64_t r, int64_t c0, uint32_t (&l)[VPL], double (&d)[VPL],
                                           uint32_t (&s)[VPL]) {
    typedef typename SigOf<SB>::T TS;
    const int64_t base = (p * A.n1 + r) * A.n2 + c0;
    if (VEC) {
        if (c0 < A.n2) {
            load_vec<TL, VPL>((const TL*)A.vol + base, l);
#pragma unroll
            for (int j = 0; j < VPL; j += 2) {
                const double2 v = *reinterpret_cast<const double2*>(A.d2 + base + j);
                d[j] = v.x; d[j + 1] = v.y;
            }
            if (SB) load_vec<TS, VPL>((const TS*)A.sig + base, s);
        } else {
#pragma unroll
            for (int j = 0; j < VPL; ++j) { l[j] = INVALID_LABEL; d[j] = 0.0; }
        }
    } else {
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const bool in = c0 + j < A.n2;
            l[j] = in ? (uint32_t)((const TL*)A.vol)[base + j] : INVALID_LABEL;
            d[j] = in ? A.d2[base + j] : 0.0;
            if (SB) s[j] = in ? (uint32_t)((const TS*)A.sig)[base + j] : 0u;
        }
    }
    if (!SB || (VEC && c0 >= A.n2)) {
#pragma unroll
        for (int j = 0; j < VPL; ++j) s[j] = 0u;
    }
}

template <typename TL, int SB, bool VEC>
__global__ __launch_bounds__(PRF_THREADS) void profile_kernel(const ProfileArgs A) {
    constexpr int VPL = 16 / (int)sizeof(TL);
    constexpr bool SIG = SB != 0;
    __shared__ ProfTable<SIG> S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < PROF_SLOTS; i += PRF_THREADS) {
        S.key[i] = NO_KEY; S.n[i] = 0u;
        if (SIG) { S.vmin[i] = NO_SIGNAL_MIN; S.vmax[i] = 0u; S.sum[i] = 0ull; S.sq[i] = 0ull; }
    }
    if (tid <= PROF_MAX_BINS) S.edge[tid] = A.edges[tid];
    __syncthreads();

    const uint32_t K = A.bins;
    const double e_first = S.edge[0], e_last = S.edge[K];

    const int64_t cols = 64 * VPL;
    const int64_t ncb = (A.n2 + cols - 1) / cols, nrb = (A.n1 + PRF_WAVES - 1) / PRF_WAVES;
    const int64_t npb = (A.n0 + PRF_PLANES - 1) / PRF_PLANES;
    const int64_t tiles = ncb * nrb * npb;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_group;
    const int64_t t1 = t0 + A.tiles_per_group < tiles ? t0 + A.tiles_per_group : tiles;

    // the lane's running record, and the shell of its previous counted voxel with the two edges around it (none yet: lo > hi)
    uint32_t acc_k = NO_KEY, acc_n = 0u, acc_mn = NO_SIGNAL_MIN, acc_mx = 0u;
    uint64_t acc_s = 0ull, acc_q = 0ull;
    uint32_t shell = 0u;
    double lo = __builtin_inf(), hi = 0.0;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t cb = t % ncb, rb = (t / ncb) % nrb, pb = t / (ncb * nrb);
        const int64_t r = rb * PRF_WAVES + wave;
        if (r >= A.n1) continue;                                   // (wave-uniform)
        const int64_t c0 = cb * cols + (int64_t)lane * VPL;
        const int64_t pbeg = pb * PRF_PLANES;
        const int64_t pend = pbeg + PRF_PLANES < A.n0 ? pbeg + PRF_PLANES : A.n0;
        uint32_t cl[VPL], cs[VPL];                                 // this plane
        double cd[VPL];
        load_strip<TL, SB, VPL, VEC>(A, pbeg, r, c0, cl, cd, cs);
        for (int64_t p = pbeg; p < pend; ++p) {
            const bool more = p + 1 < pend;                        // (wave-uniform)
            uint32_t nl[VPL], ns[VPL];                             // the next plane, in flight while this one is worked on
            double nd[VPL];
            if (more) load_strip<TL, SB, VPL, VEC>(A, p + 1, r, c0, nl, nd, ns);
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const uint32_t x = cl[j], s = cs[j];
                const double d = cd[j];
                if (x == INVALID_LABEL) continue;
                uint32_t key = NO_KEY;
                if (x > A.max_label) {
                    atomicOr(&A.flags[PROF_FLAG_RANGE], 1u);
                } else {
                    bool in = d >= lo && d < hi;
                    if (!in && d >= e_first && d < e_last) {       // (+inf fails the second test, whatever the last edge is)
                        uint32_t pos = 0u;                         // the edges at or below d, less one: d is finite, +inf lies behind edge K
#pragma unroll
                        for (uint32_t step = 32u; step > 0u; step >>= 1) pos += S.edge[pos + step] <= d ? step : 0u;
                        shell = pos; lo = S.edge[pos]; hi = S.edge[pos + 1u];
                        in = true;
                    }
                    if (in) key = x * K + shell;
                }
                if (key != acc_k) {
                    if (acc_k != NO_KEY) add_lds<SIG>(S, A, acc_k, acc_n, acc_s, acc_q, acc_mn, acc_mx);
                    acc_k = key; acc_n = 0u; acc_s = 0ull; acc_q = 0ull; acc_mn = NO_SIGNAL_MIN; acc_mx = 0u;
                }
                acc_n += 1u;
                if (SIG) {
                    acc_s += s; acc_q += (uint64_t)(s * s);
                    acc_mn = s < acc_mn ? s : acc_mn;
                    acc_mx = s > acc_mx ? s : acc_mx;
                }
            }
            if (more) {
#pragma unroll
                for (int j = 0; j < VPL; ++j) { cl[j] = nl[j]; cs[j] = ns[j]; cd[j] = nd[j]; }
            }
        }
    }

    // the lanes' last records: reduced across the wave one key at a time, the first lane of the key adds them to the table
    for (;;) {
        const uint64_t pending = __ballot(acc_k != NO_KEY);
        if (!pending) break;
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const uint32_t key = (uint32_t)__shfl((int)acc_k, leader);
        const bool mine = acc_k == key;
        uint32_t n = mine ? acc_n : 0u, mn = mine ? acc_mn : NO_SIGNAL_MIN, mx = mine ? acc_mx : 0u;
        uint64_t s = mine ? acc_s : 0ull, q = mine ? acc_q : 0ull;
        for (int o = 32; o > 0; o >>= 1) {
            n += (uint32_t)__shfl_xor((int)n, o);
            if (SIG) {
                s += __shfl_xor(s, o);
                q += __shfl_xor(q, o);
                const uint32_t omn = (uint32_t)__shfl_xor((int)mn, o), omx = (uint32_t)__shfl_xor((int)mx, o);
                mn = omn < mn ? omn : mn;
                mx = omx > mx ? omx : mx;
            }
        }
        if (lane == leader) add_lds<SIG>(S, A, key, n, s, q, mn, mx);
        if (mine) acc_k = NO_KEY;
    }
    __syncthreads();
    for (int i = tid; i < PROF_SLOTS; i += PRF_THREADS) {
        const uint32_t key = S.key[i];
        if (key != NO_KEY) add_global<SIG>(A, key, S.n[i], SIG ? S.sum[i] : 0ull, SIG ? S.sq[i] : 0ull, SIG ? S.vmin[i] : 0u, SIG ? S.vmax[i] : 0u);
    }
}

template <typename TL, int SB>
void launch_kind(hipStream_t s, const ProfileArgs& a, bool vec, int64_t groups) {
    if (vec) hipLaunchKernelGGL((profile_kernel<TL, SB, true>), dim3((unsigned)groups), dim3(PRF_THREADS), 0, s, a);
    else hipLaunchKernelGGL((profile_kernel<TL, SB, false>), dim3((unsigned)groups), dim3(PRF_THREADS), 0, s, a);
}

template <typename TL>
void launch_types(hipStream_t s, const ProfileArgs& a, int signal_itemsize, bool vec, int64_t groups) {
    if (signal_itemsize == 0) launch_kind<TL, 0>(s, a, vec, groups);
    else if (signal_itemsize == 1) launch_kind<TL, 1>(s, a, vec, groups);
    else launch_kind<TL, 2>(s, a, vec, groups);
}

}  // namespace

RangePlan launch_profile(hipStream_t s, ProfileArgs a, int label_itemsize, int signal_itemsize) {
    const RangeTiles t = range_tiles(a.n0, a.n1, a.n2, 0, label_itemsize, PRF_RANGE);      // (the pass walks every plane: it takes no slab)
    const RangePlan plan = plan_ranges(t.tiles, t.tile_voxels, PRF_RANGE);
    if (!plan.groups) return plan;
    a.tiles_per_group = plan.tiles_per_group;
    // (without a signal a.sig is NULL and its item size 0: not a buffer of the pass)
    const bool vec = strips_vectorize(a.n2, label_itemsize, {{a.vol, label_itemsize}, {a.d2, 8}, {a.sig, signal_itemsize}});
    if (label_itemsize == 2) launch_types<uint16_t>(s, a, signal_itemsize, vec, plan.groups);
    else launch_types<uint32_t>(s, a, signal_itemsize, vec, plan.groups);
    return plan;
}

}  // namespace ta
