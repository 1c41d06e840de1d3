// kernels_wallgeo.hip -- per-wall face geometry of the resident label volume (include/tissue_scan_wallgeo.h): for every pair
// of labels the signed face counts per axis and the first and second sums of the doubled face centres, in one streaming pass
// over the labels.
//
// The walk is the wall part of kernels_signal.hip: a tile is WG_WAVES rows x (64 lanes x VPL columns) x WG_PLANES planes, a
// wave owns one row and walks the planes, a lane holds a strip of VPL = 16 / sizeof(label) voxels (one 16-byte load); the
// left voxel of a strip comes from the lane before, the row above from its own load, the plane before stays in registers.  A
// workgroup takes a contiguous range of tiles and keeps ONE LDS table pair -> row for the range, flushed with global integer
// atomics at its end (the pair's global row through the open-addressed hash launch_signal_hash builds).
// What differs is the size of a row: 15 numbers, not 2.
//   in registers  a lane folds the faces of one axis that lie in consecutive voxels of its strip and have the same two labels
//                 on the same sides into one run, and adds the run with the closed forms of an arithmetic progression (sum of
//                 c and of c^2).  Runs go into the lane's ONE running record (pair, 6 counts, 3 first sums, 6 second sums),
//                 which lives for a whole tile: its numbers are relative to the tile's origin and fit 32 bits (a lane sees at
//                 most 3 * VPL * WG_PLANES = 384 faces of c < 2^10.01, c^2 < 2^20.01: below 2^28.6).  A run of another pair
//                 sends the record on its way and starts a new one.
//   in the wave   at the end of a tile the lanes' records are reduced pair by pair (ballot, leader, butterfly; the second sums
//                 in 64 bits there) and the leader sends the sum on.
//   on its way    a record is shifted from the tile's origin o to global coordinates in exact integer arithmetic,
//                     S(c + o) = S(c) + n o,   S((c + o)(c + o)^T) = S(c c^T) + o S(c)^T + S(c) o^T + n o o^T,
//                 and added to the LDS table, whose sums are 64-bit (the counts are 32-bit: a range has fewer than 2^30
//                 voxels).  A record that finds no slot within WG_PROBE probes goes to the global rows directly and is counted
//                 in flags[WG_FLAG_SPILL].
// All sums are integers modulo 2^64 and the host has checked that the true sums stay below that: the results are bit-exact
// whatever the order of the atomics.
#include "ta_wallgeo.h"

#include <algorithm>

namespace ta {
namespace {

constexpr int WG_WAVES = 4;                        // rows of a tile = waves of a workgroup
constexpr int WG_THREADS = WG_WAVES * 64;
constexpr int WG_PLANES = 16;                      // planes of a tile
constexpr int WG_SLOTS = 512;                      // LDS rows: 512 x 104 bytes = 52 KB, three workgroups a CU
constexpr int WG_PROBE = 32;                       // probes before a record goes to the global rows directly
constexpr int64_t WG_MAX_GROUPS = 4096;            // (ranges a quarter of the signal pass's: a table a quarter of its slots)
// a workgroup's LDS rows count faces in u32: fewer than 2^30 voxels (three faces each) a workgroup
constexpr RangeShape WG_RANGE = {WG_WAVES, WG_PLANES, WG_MAX_GROUPS, 30};

struct WgTable {
    unsigned long long key[WG_SLOTS];
    unsigned long long s1[3][WG_SLOTS];
    unsigned long long s2[6][WG_SLOTS];
    uint32_t cnt[6][WG_SLOTS];
};

// a lane's running record, relative to the tile's origin
struct WgRec {
    uint64_t key;
    uint32_t cnt[6], s1[3], s2[6];
};

__device__ __forceinline__ void rec_clear(WgRec& R, uint64_t key) {
    R.key = key;
#pragma unroll
    for (int f = 0; f < 6; ++f) { R.cnt[f] = 0u; R.s2[f] = 0u; }
#pragma unroll
    for (int x = 0; x < 3; ++x) R.s1[x] = 0u;
}

// sums in global coordinates, to the pair's global row
__device__ void add_global(const WallGeoArgs& A, uint64_t key, const uint32_t (&cnt)[6], const uint64_t (&s1)[3], const uint64_t (&s2)[6]) {
    uint32_t h = hash_pair((uint32_t)(key >> 32), (uint32_t)key) & A.hmask;
    for (uint32_t probe = 0; probe <= A.hmask; ++probe) {
        const uint64_t k = A.hkeys[h];
        if (k == key) {
            unsigned long long* row = A.rows + (uint64_t)A.hrows[h] * WG_ROW;
#pragma unroll
            for (int f = 0; f < 6; ++f) if (cnt[f]) atomicAdd(&row[f], (unsigned long long)cnt[f]);
#pragma unroll
            for (int x = 0; x < 3; ++x) atomicAdd(&row[6 + x], (unsigned long long)s1[x]);
#pragma unroll
            for (int q = 0; q < 6; ++q) atomicAdd(&row[9 + q], (unsigned long long)s2[q]);
            return;
        }
        if (k == EMPTY_KEY) break;
        h = (h + 1) & A.hmask;
    }
    atomicOr(&A.flags[WG_FLAG_PAIR_MISS], 1u);             // a face of a pair the extraction does not have
}

// a record relative to the origin (o0, o1, o2) leaves the registers: shifted to global coordinates, into the LDS table
__device__ __forceinline__ void emit(WgTable& S, const WallGeoArgs& A, uint64_t key, const uint32_t (&cnt)[6], const uint64_t (&r1)[3],
                                     const uint64_t (&r2)[6], uint64_t o0, uint64_t o1, uint64_t o2) {
    const uint64_t n = (uint64_t)cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4] + cnt[5];
    const uint64_t o[3] = {o0, o1, o2};
    uint64_t s1[3], s2[6];
#pragma unroll
    for (int x = 0; x < 3; ++x) s1[x] = r1[x] + n * o[x];
    {
        int q = 0;
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = x; y < 3; ++y, ++q) s2[q] = r2[q] + o[x] * r1[y] + o[y] * r1[x] + n * o[x] * o[y];
    }
    uint32_t h = hash_pair((uint32_t)(key >> 32), (uint32_t)key) & (WG_SLOTS - 1);
    for (int probe = 0; probe < WG_PROBE; ++probe) {
        const unsigned long long k = atomicCAS(&S.key[h], (unsigned long long)EMPTY_KEY, (unsigned long long)key);
        if (k == EMPTY_KEY || k == key) {
#pragma unroll
            for (int f = 0; f < 6; ++f) if (cnt[f]) atomicAdd(&S.cnt[f][h], cnt[f]);
#pragma unroll
            for (int x = 0; x < 3; ++x) atomicAdd(&S.s1[x][h], (unsigned long long)s1[x]);
#pragma unroll
            for (int q = 0; q < 6; ++q) atomicAdd(&S.s2[q][h], (unsigned long long)s2[q]);
            return;
        }
        h = (h + 1) & (WG_SLOTS - 1);
    }
    atomicAdd(&A.flags[WG_FLAG_SPILL], 1u);
    add_global(A, key, cnt, s1, s2);
}

__device__ __forceinline__ void emit_rec(WgTable& S, const WallGeoArgs& A, const WgRec& R, uint64_t o0, uint64_t o1, uint64_t o2) {
    const uint64_t r1[3] = {R.s1[0], R.s1[1], R.s1[2]};
    const uint64_t r2[6] = {R.s2[0], R.s2[1], R.s2[2], R.s2[3], R.s2[4], R.s2[5]};
    emit(S, A, R.key, R.cnt, r1, r2, o0, o1, o2);
}

// A run of k faces of axis `ax` in consecutive voxels of a strip: low-side label dk >> 32, high-side label (uint32_t)dk; the
// centres are (c0, c1, a2 + 2 i), i = 0 .. k - 1, relative to the tile's origin.
__device__ __forceinline__ void close_run(WgTable& S, const WallGeoArgs& A, WgRec& R, uint64_t dk, int ax, uint32_t c0, uint32_t c1,
                                          uint32_t a2, uint32_t k, uint64_t o0, uint64_t o1, uint64_t o2) {
    const uint32_t y = (uint32_t)(dk >> 32), x = (uint32_t)dk;
    const bool rev = y > x;                                    // the pair's hi on the low-coordinate side
    const uint64_t key = rev ? (((uint64_t)x << 32) | y) : dk;
    if (key != R.key) {
        if (R.key != EMPTY_KEY) emit_rec(S, A, R, o0, o1, o2);
        rec_clear(R, key);
    }
    const uint32_t kf = rev ? 0u : k, kr = rev ? k : 0u;
    R.cnt[0] += ax == 0 ? kf : 0u; R.cnt[1] += ax == 1 ? kf : 0u; R.cnt[2] += ax == 2 ? kf : 0u;
    R.cnt[3] += ax == 0 ? kr : 0u; R.cnt[4] += ax == 1 ? kr : 0u; R.cnt[5] += ax == 2 ? kr : 0u;
    const uint32_t kk = k * (k - 1u);                          // 2 * sum of i
    const uint32_t t2 = k * a2 + kk;                           // sum of (a2 + 2 i)
    const uint32_t q2 = k * a2 * a2 + 2u * a2 * kk + 2u * (kk * (2u * k - 1u) / 3u);   // sum of (a2 + 2 i)^2
    R.s1[0] += k * c0; R.s1[1] += k * c1; R.s1[2] += t2;
    R.s2[0] += k * c0 * c0; R.s2[1] += k * c0 * c1; R.s2[2] += c0 * t2;
    R.s2[3] += k * c1 * c1; R.s2[4] += c1 * t2; R.s2[5] += q2;
}

template <int VPL>
__device__ __forceinline__ void strip_outside(uint32_t (&l)[VPL]) {
#pragma unroll
    for (int j = 0; j < VPL; ++j) l[j] = INVALID_LABEL;
}

// the strip of row r of plane p that starts at column c0 (INVALID_LABEL past the row's end).  VEC: every strip is whole or
// wholly outside the row (n2 % VPL == 0) and the buffer is aligned for the 16-byte load.
template <typename TL, int VPL, bool VEC>
__device__ __forceinline__ void load_strip(const WallGeoArgs& A, int64_t p, int64_t r, int64_t c0, uint32_t (&l)[VPL]) {
    const int64_t base = (p * A.n1 + r) * A.n2 + c0;
    if (VEC) {
        if (c0 < A.n2) {
            const uint4 v = *reinterpret_cast<const uint4*>((const TL*)A.vol + base);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < VPL; ++j) l[j] = sizeof(TL) == 4 ? w[j % 4] : (w[(j >> 1) % 4] >> (16 * (j & 1))) & 0xffffu;
        } else {
            strip_outside<VPL>(l);
        }
    } else {
#pragma unroll
        for (int j = 0; j < VPL; ++j) l[j] = c0 + j < A.n2 ? (uint32_t)((const TL*)A.vol)[base + j] : INVALID_LABEL;
    }
}

template <typename TL, bool VEC>
__global__ __launch_bounds__(WG_THREADS) void wallgeo_kernel(const WallGeoArgs A) {
    constexpr int VPL = 16 / (int)sizeof(TL);
    __shared__ WgTable S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < WG_SLOTS; i += WG_THREADS) {
        S.key[i] = EMPTY_KEY;
#pragma unroll
        for (int f = 0; f < 6; ++f) { S.cnt[f][i] = 0u; S.s2[f][i] = 0ull; }
#pragma unroll
        for (int x = 0; x < 3; ++x) S.s1[x][i] = 0ull;
    }
    __syncthreads();

    const int64_t cols = 64 * VPL;
    const int64_t ncb = (A.n2 + cols - 1) / cols, nrb = (A.n1 + WG_WAVES - 1) / WG_WAVES;
    const int64_t npb = (A.n0 - A.first_owned + WG_PLANES - 1) / WG_PLANES;
    const int64_t tiles = ncb * nrb * npb;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_group;
    const int64_t t1 = t0 + A.tiles_per_group < tiles ? t0 + A.tiles_per_group : tiles;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t cb = t % ncb, rb = (t / ncb) % nrb, pb = t / (ncb * nrb);
        const int64_t r = rb * WG_WAVES + wave;
        if (r >= A.n1) continue;                                   // (wave-uniform)
        const int64_t c0 = cb * cols + (int64_t)lane * VPL;
        const int64_t pbeg = A.first_owned + pb * WG_PLANES;
        const int64_t pend = pbeg + WG_PLANES < A.n0 ? pbeg + WG_PLANES : A.n0;
        // the tile's origin in doubled global coordinates, one voxel before its first: every relative centre is >= 1
        const uint64_t o0 = (uint64_t)(2 * (pbeg + A.origin0) - 2), o1 = (uint64_t)(2 * rb * WG_WAVES - 2), o2 = (uint64_t)(2 * cb * cols - 2);
        const uint32_t v1 = 2u * (uint32_t)wave + 2u, v2 = 2u * (uint32_t)(lane * VPL) + 2u;      // this lane's first voxel, relative
        WgRec R;
        rec_clear(R, EMPTY_KEY);
        uint32_t cl[VPL], ul[VPL], bl[VPL];                        // this plane, the row above, the plane before
        load_strip<TL, VPL, VEC>(A, pbeg, r, c0, cl);
        if (r > 0) load_strip<TL, VPL, VEC>(A, pbeg, r - 1, c0, ul);
        else strip_outside<VPL>(ul);
        if (pbeg > 0) load_strip<TL, VPL, VEC>(A, pbeg - 1, r, c0, bl);
        else strip_outside<VPL>(bl);
        for (int64_t p = pbeg; p < pend; ++p) {
            const bool more = p + 1 < pend;                        // (wave-uniform)
            uint32_t nl[VPL], nul[VPL];                            // the next plane, in flight while this one is worked on
            if (more) {
                load_strip<TL, VPL, VEC>(A, p + 1, r, c0, nl);
                if (r > 0) load_strip<TL, VPL, VEC>(A, p + 1, r - 1, c0, nul);
                else strip_outside<VPL>(nul);
            }
            // element 0's neighbour along axis 2: the last element of the lane before; lane 0 reads its own
            uint32_t ll = (uint32_t)__shfl_up((int)cl[VPL - 1], 1);
            if (lane == 0) {
                ll = INVALID_LABEL;
                if (c0 > 0 && c0 <= A.n2) ll = (uint32_t)((const TL*)A.vol)[(p * A.n1 + r) * A.n2 + c0 - 1];
            }
            const uint32_t v0 = 2u * (uint32_t)(p - pbeg) + 2u;
#pragma unroll 1
            for (int ax = 0; ax < 3; ++ax) {
                uint32_t nb[VPL];                                  // the lower neighbour of every voxel along this axis
#pragma unroll
                for (int j = 0; j < VPL; ++j) nb[j] = ax == 0 ? bl[j] : ax == 1 ? ul[j] : (j ? cl[j - 1] : ll);
                const uint32_t f0 = v0 - (ax == 0 ? 1u : 0u), f1 = v1 - (ax == 1 ? 1u : 0u), f2 = v2 - (ax == 2 ? 1u : 0u);
                uint64_t rk = EMPTY_KEY;                           // the open run: low-side label << 32 | high-side label
                uint32_t rstart = 0u, rlen = 0u;
#pragma unroll
                for (int j = 0; j <= VPL; ++j) {
                    uint64_t dk = EMPTY_KEY;
                    if (j < VPL) {
                        const uint32_t x = cl[j < VPL ? j : 0], y = nb[j < VPL ? j : 0];
                        if (x != INVALID_LABEL && y != INVALID_LABEL && x != y) dk = ((uint64_t)y << 32) | x;
                    }
                    if (dk != rk) {
                        if (rk != EMPTY_KEY) close_run(S, A, R, rk, ax, f0, f1, f2 + 2u * rstart, rlen, o0, o1, o2);
                        rk = dk; rstart = (uint32_t)j; rlen = 0u;
                    }
                    ++rlen;
                }
            }
            if (more) {
#pragma unroll
                for (int j = 0; j < VPL; ++j) { bl[j] = cl[j]; ul[j] = nul[j]; cl[j] = nl[j]; }
            }
        }
        // the lanes' records of this tile: reduced across the wave one pair at a time, the first lane of the pair sends the sum on
        for (;;) {
            const uint64_t pending = __ballot(R.key != EMPTY_KEY);
            if (!pending) break;
            const int leader = __ffsll((unsigned long long)pending) - 1;
            const uint64_t K = __shfl(R.key, leader);
            const bool mine = R.key == K;
            uint32_t cnt[6];
            uint64_t r1[3], r2[6];
#pragma unroll
            for (int f = 0; f < 6; ++f) { cnt[f] = mine ? R.cnt[f] : 0u; r2[f] = mine ? (uint64_t)R.s2[f] : 0ull; }
#pragma unroll
            for (int x = 0; x < 3; ++x) r1[x] = mine ? (uint64_t)R.s1[x] : 0ull;
            for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
                for (int f = 0; f < 6; ++f) { cnt[f] += (uint32_t)__shfl_xor((int)cnt[f], o); r2[f] += __shfl_xor(r2[f], o); }
#pragma unroll
                for (int x = 0; x < 3; ++x) r1[x] += (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)r1[x], o);
            }
            if (lane == leader) emit(S, A, K, cnt, r1, r2, o0, o1, o2);
            if (mine) R.key = EMPTY_KEY;
        }
    }

    __syncthreads();
    for (int i = tid; i < WG_SLOTS; i += WG_THREADS) {
        const uint64_t k = S.key[i];
        if (k == EMPTY_KEY) continue;
        uint32_t cnt[6];
        uint64_t s1[3], s2[6];
#pragma unroll
        for (int f = 0; f < 6; ++f) { cnt[f] = S.cnt[f][i]; s2[f] = S.s2[f][i]; }
#pragma unroll
        for (int x = 0; x < 3; ++x) s1[x] = S.s1[x][i];
        add_global(A, k, cnt, s1, s2);
    }
}

}  // namespace

RangePlan launch_wallgeo(hipStream_t s, WallGeoArgs a, int label_itemsize) {
    const RangeTiles t = range_tiles(a.n0, a.n1, a.n2, a.first_owned, label_itemsize, WG_RANGE);
    const RangePlan plan = plan_ranges(t.tiles, t.tile_voxels, WG_RANGE);
    if (!plan.groups) return plan;
    a.tiles_per_group = plan.tiles_per_group;
    const bool vec = strips_vectorize(a.n2, label_itemsize, {{a.vol, label_itemsize}});
    if (label_itemsize == 2) {
        if (vec) hipLaunchKernelGGL((wallgeo_kernel<uint16_t, true>), dim3(plan.groups), dim3(WG_THREADS), 0, s, a);
        else hipLaunchKernelGGL((wallgeo_kernel<uint16_t, false>), dim3(plan.groups), dim3(WG_THREADS), 0, s, a);
    } else {
        if (vec) hipLaunchKernelGGL((wallgeo_kernel<uint32_t, true>), dim3(plan.groups), dim3(WG_THREADS), 0, s, a);
        else hipLaunchKernelGGL((wallgeo_kernel<uint32_t, false>), dim3(plan.groups), dim3(WG_THREADS), 0, s, a);
    }
    return plan;
}

}  // namespace ta
