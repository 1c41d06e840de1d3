// kernels_signal.hip -- per-label and per-wall statistics of an intensity image over the resident label volume
// (include/tissue_scan_signal.h), in one streaming pass over labels + signal.
//
// Layout of the pass.  A tile is SIG_WAVES rows x (64 lanes x VPL columns) x SIG_PLANES planes; every wave owns one row of it
// and walks the planes, each lane holding a strip of VPL = 16 / sizeof(label) voxels along memory axis 2 (16 bytes of labels a
// lane: 8 uint16 or 4 uint32 labels, and as many signal values).  The next plane's strips are loaded while the current one is
// worked on.  A workgroup takes a contiguous range of tiles (row blocks of one plane block first, so that its labels stay few)
// and keeps two LDS tables for the whole range -- label -> (n, sum, sum of squares, min, max) and pair -> (side_lo, side_hi)
// -- which it flushes with global atomics once, at its end.
//   per label: a lane folds its voxels into ONE running record (label, n, sum, sumsq, min, max) for as long as the label does
//     not change -- along its strip and from plane to plane -- and hands it to the LDS table only when it does; the lanes'
//     last records are reduced across the wave label by label before they go to the table.
//   per wall: the faces of the voxel with its lower neighbours along the three memory axes -- axis 2 inside the strip (the
//     lane before gives element 0 its neighbour), axis 1 the row above (its own load, which the wave of that row has just
//     brought into the caches), axis 0 the plane before (kept in registers from the previous step; the tile's first plane
//     reads it) -- exactly the faces TA_F_ADJACENCY counts, a face belonging to the slab of its higher voxel.  Faces of one
//     pair in consecutive voxels of a strip are summed in registers before they reach the LDS table.  At the flush a pair is
//     found in an open-addressed device hash of the sorted pair list (pair -> row), built by signal_hash_kernel per call.
// All sums are integers: the results are bit-exact whatever the order of the atomics.  sumsq is 128-bit in global memory:
// the add to the low word returns the old value, and an add that wraps it carries one into the high word.
#include "ta_signal.h"

#include <algorithm>

namespace ta {
namespace {

constexpr int SIG_WAVES = 4;                       // rows of a tile = waves of a workgroup
constexpr int SIG_THREADS = SIG_WAVES * 64;
constexpr int SIG_PLANES = 16;                     // planes of a tile
constexpr int SIG_LSLOTS = 512, SIG_PSLOTS = 2048; // LDS table slots (16 + 48 KB: a workgroup's tiles of C4 touch ~750 pairs)
constexpr int SIG_LPROBE = 32, SIG_PPROBE = 32;    // probes before a record goes to the global rows directly
constexpr int64_t SIG_MAX_GROUPS = 1024;           // four workgroups a CU
// a workgroup's LDS rows count voxels in u32: fewer than 2^31 voxels a workgroup
constexpr RangeShape SIG_RANGE = {SIG_WAVES, SIG_PLANES, SIG_MAX_GROUPS, 31};
constexpr uint32_t NO_SIGNAL_MIN = 0xffffffffu;

// (a pass without walls has no pair table: 16 KB of LDS instead of 64, more workgroups a CU)
template <bool WALL>
struct SigTables {
    static constexpr int PS = WALL ? SIG_PSLOTS : 1;
    uint32_t lkey[SIG_LSLOTS], ln[SIG_LSLOTS], lmin[SIG_LSLOTS], lmax[SIG_LSLOTS];
    unsigned long long lsum[SIG_LSLOTS], lsq[SIG_LSLOTS];
    unsigned long long pkey[PS], pslo[PS], pshi[PS];
};

__device__ void label_add_global(const SignalArgs& A, uint32_t l, uint64_t n, uint64_t s, uint64_t q, uint32_t mn, uint32_t mx) {
    if (l > A.max_label) { atomicOr(&A.flags[SIG_FLAG_RANGE], 1u); return; }
    atomicAdd(&A.n[l], (unsigned long long)n);
    atomicAdd(&A.sum[l], (unsigned long long)s);
    const unsigned long long old = atomicAdd(&A.sumsq[2 * (uint64_t)l], (unsigned long long)q);
    if (old + q < old) atomicAdd(&A.sumsq[2 * (uint64_t)l + 1], 1ull);        // the low word wrapped: carry
    atomicMin(&A.vmin[l], mn);
    atomicMax(&A.vmax[l], mx);
}

__device__ void pair_add_global_row(const SignalArgs& A, uint64_t key, uint64_t slo, uint64_t shi) {
    if (!A.hkeys) { atomicOr(&A.flags[SIG_FLAG_PAIR_MISS], 1u); return; }      // an extraction without pairs has no index: every face is a miss
    uint32_t h = hash_pair((uint32_t)(key >> 32), (uint32_t)key) & A.hmask;
    for (uint32_t probe = 0; probe <= A.hmask; ++probe) {
        const uint64_t k = A.hkeys[h];
        if (k == key) {
            const uint32_t row = A.hrows[h];
            atomicAdd(&A.side_lo[row], (unsigned long long)slo);
            atomicAdd(&A.side_hi[row], (unsigned long long)shi);
            return;
        }
        if (k == EMPTY_KEY) break;
        h = (h + 1) & A.hmask;
    }
    atomicOr(&A.flags[SIG_FLAG_PAIR_MISS], 1u);            // a face of a pair the extraction does not have
}

template <typename TAB>
__device__ __forceinline__ void label_add_lds(TAB& S, const SignalArgs& A, uint32_t l, uint32_t n, uint64_t s, uint64_t q,
                                              uint32_t mn, uint32_t mx) {
    uint32_t h = hash_u32(l) & (SIG_LSLOTS - 1);
    for (int probe = 0; probe < SIG_LPROBE; ++probe) {
        const uint32_t k = atomicCAS(&S.lkey[h], INVALID_LABEL, l);
        if (k == INVALID_LABEL || k == l) {
            atomicAdd(&S.ln[h], n);
            atomicAdd(&S.lsum[h], (unsigned long long)s);
            atomicAdd(&S.lsq[h], (unsigned long long)q);
            atomicMin(&S.lmin[h], mn);
            atomicMax(&S.lmax[h], mx);
            return;
        }
        h = (h + 1) & (SIG_LSLOTS - 1);
    }
    atomicAdd(&A.flags[SIG_FLAG_LABEL_SPILL], 1u);
    label_add_global(A, l, n, s, q, mn, mx);
}

template <typename TAB>
__device__ __forceinline__ void pair_add_lds(TAB& S, const SignalArgs& A, uint64_t key, uint64_t slo, uint64_t shi) {
    uint32_t h = hash_pair((uint32_t)(key >> 32), (uint32_t)key) & (SIG_PSLOTS - 1);
    for (int probe = 0; probe < SIG_PPROBE; ++probe) {
        const unsigned long long k = atomicCAS(&S.pkey[h], (unsigned long long)EMPTY_KEY, (unsigned long long)key);
        if (k == EMPTY_KEY || k == key) {
            atomicAdd(&S.pslo[h], (unsigned long long)slo);
            atomicAdd(&S.pshi[h], (unsigned long long)shi);
            return;
        }
        h = (h + 1) & (SIG_PSLOTS - 1);
    }
    atomicAdd(&A.flags[SIG_FLAG_PAIR_SPILL], 1u);
    pair_add_global_row(A, key, slo, shi);
}

// one face between a voxel of label a (signal sa) and one of label b != a (signal sb): key lo << 32 | hi, and the signal on each side
__device__ __forceinline__ void face_of(uint32_t a, uint32_t sa, uint32_t b, uint32_t sb, uint64_t& key, uint32_t& slo, uint32_t& shi) {
    if (a < b) { key = ((uint64_t)a << 32) | b; slo = sa; shi = sb; }
    else { key = ((uint64_t)b << 32) | a; slo = sb; shi = sa; }
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

template <int VPL>
__device__ __forceinline__ void strip_outside(uint32_t (&l)[VPL], uint32_t (&s)[VPL]) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) { l[j] = INVALID_LABEL; s[j] = 0u; }
}

// the strip of row r of plane p that starts at column c0: labels (INVALID_LABEL past the row's end) and signal.  VEC: every strip
// is whole or wholly outside the row (n2 % VPL == 0) and both buffers are aligned for the vector loads.
template <typename TL, typename TS, int VPL, bool VEC>
__device__ __forceinline__ void load_strip(const SignalArgs& A, int64_t p, int64_t r, int64_t c0, uint32_t (&l)[VPL], uint32_t (&s)[VPL]) {
    const int64_t base = (p * A.n1 + r) * A.n2 + c0;
    if (VEC) {
        if (c0 < A.n2) {
            load_vec<TL, VPL>((const TL*)A.vol + base, l);
            load_vec<TS, VPL>((const TS*)A.sig + base, s);
        } else {
            strip_outside<VPL>(l, s);
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

template <typename TL, typename TS, bool LAB, bool WALL, bool VEC>
__global__ __launch_bounds__(SIG_THREADS) void signal_kernel(const SignalArgs A) {
    constexpr int VPL = 16 / (int)sizeof(TL);
    __shared__ SigTables<WALL> S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (LAB)
        for (int i = tid; i < SIG_LSLOTS; i += SIG_THREADS) {
            S.lkey[i] = INVALID_LABEL; S.ln[i] = 0u; S.lmin[i] = NO_SIGNAL_MIN; S.lmax[i] = 0u; S.lsum[i] = 0ull; S.lsq[i] = 0ull;
        }
    if (WALL)
        for (int i = tid; i < SIG_PSLOTS; i += SIG_THREADS) { S.pkey[i] = EMPTY_KEY; S.pslo[i] = 0ull; S.pshi[i] = 0ull; }
    __syncthreads();

    const int64_t cols = 64 * VPL;
    const int64_t ncb = (A.n2 + cols - 1) / cols, nrb = (A.n1 + SIG_WAVES - 1) / SIG_WAVES;
    const int64_t npb = (A.n0 - A.first_owned + SIG_PLANES - 1) / SIG_PLANES;
    const int64_t tiles = ncb * nrb * npb;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_group;
    const int64_t t1 = t0 + A.tiles_per_group < tiles ? t0 + A.tiles_per_group : tiles;

    // the lane's running per-label record
    uint32_t acc_l = INVALID_LABEL, acc_n = 0u, acc_mn = NO_SIGNAL_MIN, acc_mx = 0u;
    uint64_t acc_s = 0ull, acc_q = 0ull;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t cb = t % ncb, rb = (t / ncb) % nrb, pb = t / (ncb * nrb);
        const int64_t r = rb * SIG_WAVES + wave;
        if (r >= A.n1) continue;                                   // (wave-uniform)
        const int64_t c0 = cb * cols + (int64_t)lane * VPL;
        const int64_t pbeg = A.first_owned + pb * SIG_PLANES;
        const int64_t pend = pbeg + SIG_PLANES < A.n0 ? pbeg + SIG_PLANES : A.n0;
        uint32_t cl[VPL], cs[VPL];                                 // this plane
        uint32_t ul[VPL], us[VPL];                                 // the row above (walls)
        uint32_t bl[VPL], bs[VPL];                                 // the plane before (walls)
        load_strip<TL, TS, VPL, VEC>(A, pbeg, r, c0, cl, cs);
        if (WALL) {
            if (r > 0) load_strip<TL, TS, VPL, VEC>(A, pbeg, r - 1, c0, ul, us);
            else strip_outside<VPL>(ul, us);
            if (pbeg > 0) load_strip<TL, TS, VPL, VEC>(A, pbeg - 1, r, c0, bl, bs);
            else strip_outside<VPL>(bl, bs);
        }
        for (int64_t p = pbeg; p < pend; ++p) {
            const bool more = p + 1 < pend;                        // (wave-uniform)
            uint32_t nl[VPL], ns[VPL], nul[VPL], nus[VPL];         // the next plane, in flight while this one is worked on
            if (more) {
                load_strip<TL, TS, VPL, VEC>(A, p + 1, r, c0, nl, ns);
                if (WALL) {
                    if (r > 0) load_strip<TL, TS, VPL, VEC>(A, p + 1, r - 1, c0, nul, nus);
                    else strip_outside<VPL>(nul, nus);
                }
            }
            if (WALL) {
                // element 0's neighbour along axis 2: the last element of the lane before; lane 0 reads its own
                uint32_t ll = (uint32_t)__shfl_up((int)cl[VPL - 1], 1), ls = (uint32_t)__shfl_up((int)cs[VPL - 1], 1);
                if (lane == 0) {
                    ll = INVALID_LABEL; ls = 0u;
                    if (c0 > 0 && c0 <= A.n2) {
                        const int64_t i = (p * A.n1 + r) * A.n2 + c0 - 1;
                        ll = (uint32_t)((const TL*)A.vol)[i];
                        ls = (uint32_t)((const TS*)A.sig)[i];
                    }
                }
                uint64_t uk = EMPTY_KEY, bk = EMPTY_KEY, uslo = 0ull, ushi = 0ull, bslo = 0ull, bshi = 0ull;
#pragma unroll
                for (int j = 0; j < VPL; ++j) {
                    const uint32_t x = cl[j], sx = cs[j];
                    if (x == INVALID_LABEL) continue;
                    uint64_t key;
                    uint32_t slo, shi;
                    const uint32_t y2 = j ? cl[j - 1] : ll, s2 = j ? cs[j - 1] : ls;
                    if (y2 != INVALID_LABEL && y2 != x) {
                        face_of(y2, s2, x, sx, key, slo, shi);
                        pair_add_lds(S, A, key, slo, shi);
                    }
                    if (ul[j] != INVALID_LABEL && ul[j] != x) {
                        face_of(ul[j], us[j], x, sx, key, slo, shi);
                        if (key != uk) {
                            if (uk != EMPTY_KEY) pair_add_lds(S, A, uk, uslo, ushi);
                            uk = key; uslo = 0ull; ushi = 0ull;
                        }
                        uslo += slo; ushi += shi;
                    }
                    if (bl[j] != INVALID_LABEL && bl[j] != x) {
                        face_of(bl[j], bs[j], x, sx, key, slo, shi);
                        if (key != bk) {
                            if (bk != EMPTY_KEY) pair_add_lds(S, A, bk, bslo, bshi);
                            bk = key; bslo = 0ull; bshi = 0ull;
                        }
                        bslo += slo; bshi += shi;
                    }
                }
                if (uk != EMPTY_KEY) pair_add_lds(S, A, uk, uslo, ushi);
                if (bk != EMPTY_KEY) pair_add_lds(S, A, bk, bslo, bshi);
            }
            if (LAB) {
#pragma unroll
                for (int j = 0; j < VPL; ++j) {
                    const uint32_t x = cl[j], s = cs[j];
                    if (x == INVALID_LABEL) continue;
                    if (x != acc_l) {
                        if (acc_l != INVALID_LABEL) label_add_lds(S, A, acc_l, acc_n, acc_s, acc_q, acc_mn, acc_mx);
                        acc_l = x; acc_n = 0u; acc_s = 0ull; acc_q = 0ull; acc_mn = NO_SIGNAL_MIN; acc_mx = 0u;
                    }
                    acc_n += 1u; acc_s += s; acc_q += (uint64_t)(s * s);
                    acc_mn = s < acc_mn ? s : acc_mn;
                    acc_mx = s > acc_mx ? s : acc_mx;
                }
            }
            if (more) {
#pragma unroll
                for (int j = 0; j < VPL; ++j) {
                    if (WALL) { bl[j] = cl[j]; bs[j] = cs[j]; ul[j] = nul[j]; us[j] = nus[j]; }
                    cl[j] = nl[j]; cs[j] = ns[j];
                }
            }
        }
    }

    if (LAB) {
        // the lanes' last records: reduced across the wave one label at a time, the first lane of the label adds them to the table
        for (;;) {
            const uint64_t pending = __ballot(acc_l != INVALID_LABEL);
            if (!pending) break;
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const uint32_t L = (uint32_t)__shfl((int)acc_l, leader);
            const bool mine = acc_l == L;
            uint32_t n = mine ? acc_n : 0u, mn = mine ? acc_mn : NO_SIGNAL_MIN, mx = mine ? acc_mx : 0u;
            uint64_t s = mine ? acc_s : 0ull, q = mine ? acc_q : 0ull;
            for (int o = 32; o > 0; o >>= 1) {
                n += (uint32_t)__shfl_xor((int)n, o);
                s += __shfl_xor(s, o);
                q += __shfl_xor(q, o);
                const uint32_t omn = (uint32_t)__shfl_xor((int)mn, o), omx = (uint32_t)__shfl_xor((int)mx, o);
                mn = omn < mn ? omn : mn;
                mx = omx > mx ? omx : mx;
            }
            if (lane == leader) label_add_lds(S, A, L, n, s, q, mn, mx);
            if (mine) acc_l = INVALID_LABEL;
        }
    }
    __syncthreads();
    if (LAB)
        for (int i = tid; i < SIG_LSLOTS; i += SIG_THREADS) {
            const uint32_t l = S.lkey[i];
            if (l != INVALID_LABEL) label_add_global(A, l, S.ln[i], S.lsum[i], S.lsq[i], S.lmin[i], S.lmax[i]);
        }
    if (WALL)
        for (int i = tid; i < SIG_PSLOTS; i += SIG_THREADS) {
            const uint64_t k = S.pkey[i];
            if (k != EMPTY_KEY) pair_add_global_row(A, k, S.pslo[i], S.pshi[i]);
        }
}

__global__ void signal_hash_kernel(const uint64_t* keys, uint64_t n, unsigned long long* hkeys, uint32_t* hrows, uint32_t hmask) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i];
        uint32_t h = hash_pair((uint32_t)(key >> 32), (uint32_t)key) & hmask;
        for (uint32_t probe = 0; probe <= hmask; ++probe) {
            if (atomicCAS(&hkeys[h], (unsigned long long)EMPTY_KEY, (unsigned long long)key) == EMPTY_KEY) {
                hrows[h] = (uint32_t)i;
                break;
            }
            h = (h + 1) & hmask;
        }
    }
}

template <typename TL, typename TS, bool LAB, bool WALL>
void launch_kind(hipStream_t s, const SignalArgs& a, bool vec, int64_t groups) {
    if (vec) hipLaunchKernelGGL((signal_kernel<TL, TS, LAB, WALL, true>), dim3((unsigned)groups), dim3(SIG_THREADS), 0, s, a);
    else hipLaunchKernelGGL((signal_kernel<TL, TS, LAB, WALL, false>), dim3((unsigned)groups), dim3(SIG_THREADS), 0, s, a);
}

template <typename TL, typename TS>
void launch_types(hipStream_t s, const SignalArgs& a, uint32_t what, bool vec, int64_t groups) {
    if ((what & SIG_LABELS) && (what & SIG_WALLS)) launch_kind<TL, TS, true, true>(s, a, vec, groups);
    else if (what & SIG_LABELS) launch_kind<TL, TS, true, false>(s, a, vec, groups);
    else if (what & SIG_WALLS) launch_kind<TL, TS, false, true>(s, a, vec, groups);
}

}  // namespace

void launch_signal_hash(hipStream_t s, const uint64_t* keys, uint64_t n, uint64_t* hkeys, uint32_t* hrows, uint32_t hmask) {
    if (!n) return;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(signal_hash_kernel, dim3((unsigned)blocks), dim3(256), 0, s, keys, n, (unsigned long long*)hkeys, hrows, hmask);
}

RangePlan launch_signal(hipStream_t s, SignalArgs a, int label_itemsize, int signal_itemsize, uint32_t what) {
    if (!(what & (SIG_LABELS | SIG_WALLS))) return RangePlan();
    const RangeTiles t = range_tiles(a.n0, a.n1, a.n2, a.first_owned, label_itemsize, SIG_RANGE);
    const RangePlan plan = plan_ranges(t.tiles, t.tile_voxels, SIG_RANGE);
    if (!plan.groups) return plan;
    a.tiles_per_group = plan.tiles_per_group;
    const bool vec = strips_vectorize(a.n2, label_itemsize, {{a.vol, label_itemsize}, {a.sig, signal_itemsize}});
    if (label_itemsize == 2 && signal_itemsize == 1) launch_types<uint16_t, uint8_t>(s, a, what, vec, plan.groups);
    else if (label_itemsize == 2) launch_types<uint16_t, uint16_t>(s, a, what, vec, plan.groups);
    else if (signal_itemsize == 1) launch_types<uint32_t, uint8_t>(s, a, what, vec, plan.groups);
    else launch_types<uint32_t, uint16_t>(s, a, what, vec, plan.groups);
    return plan;
}

}  // namespace ta
