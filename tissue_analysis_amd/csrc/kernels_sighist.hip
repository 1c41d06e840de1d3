// kernels_sighist.hip -- per-label histograms of the signal image and exact order statistics by a radix select over them
// (include/tissue_scan_sighist.h).
//
// The digit kernel serves both.  Its tile walk is that of kernels_signal.hip: a tile is SH_WAVES rows x (64 lanes x VPL columns) x
// SH_PLANES planes, every wave owns one row of it and walks the planes, each lane holding a strip of VPL = 16 / sizeof(label)
// voxels along memory axis 2 and as many signal values; the next plane's strips are loaded while the current one is worked on.  A
// workgroup takes a contiguous range of tiles.  Per voxel it adds 1 to counts[key * stride + d], d = (S >> shift) & 255, where
//   without selectors  key = row: every voxel counts (a histogram, the first pass of a select);
//   with selectors     key = row * nsel + j for the j whose selector sel[key] equals S >> (shift + 8); a voxel that matches none
//                      counts nowhere.  The select kernel leaves the distinct high bytes of a row, so at most one j matches.
// The running record of the other feature passes does not help: the key (row, digit) changes at almost every voxel.  What is
// kept is the SLOT: the workgroup's LDS table is SH_SLOTS dense rows of 256 u32 counters behind an open-addressed key -> slot
// table of as many entries (the position of a key IS its slot); a lane looks its slot(s) up only when its label changes and
// keeps (label, slot) in registers along the strip and from plane to plane.  A key without a slot within SH_PROBE probes adds to
// the global counter directly, voxel by voxel, and counts that.  Equal (slot, digit) of neighbouring lanes are combined before
// the LDS atomic by the run trick of kernels_wallsort.hip: only the first lane of a run adds, the run's length (a constant
// signal would otherwise put 64 lanes on one address, which the CU serialises).  At its end the workgroup adds the non-zero
// counters of its occupied slots to the global table, one thread a digit.
// A label above max_label raises SH_FLAG_RANGE before a key is formed: every key that reaches a table is below its size.  All
// counts are integers: bit-exact whatever the order of the atomics.
// The select kernels: one wave a row; the 256 u64 counts are prefix-summed four a lane, the digit that holds the rank is found
// and the rank's remainder stays on the device.
// (The strip-load helpers are copies of those of kernels_signal.hip, by decision: the feature kernels share no code.)
#include "ta_sighist.h"

#include <algorithm>

namespace ta {
namespace {

constexpr int SH_WAVES = 4;                        // rows of a tile = waves of a workgroup
constexpr int SH_THREADS = SH_WAVES * 64;
constexpr int SH_PLANES = 16;                      // planes of a tile
constexpr int SH_PROBE = SH_SLOTS < 16 ? SH_SLOTS : 16;      // probes before a key goes without a slot
// a workgroup's LDS counters are u32: fewer than 2^31 voxels a workgroup
constexpr RangeShape SH_RANGE = {SH_WAVES, SH_PLANES, SH_MAX_GROUPS, 31};
constexpr uint32_t NO_KEY = 0xffffffffu;           // keys are below 2^23: never a key
constexpr uint32_t SLOT_GLOBAL = 0xfffffffeu;      // the key found no slot: its voxels go to the global counters
constexpr uint32_t SLOT_SKIP = 0xffffffffu;        // nothing to count (no selector, or a label out of range)
constexpr uint32_t NO_ADDR = 0xffffffffu;

static_assert(SH_THREADS == 256, "the flush takes one thread a digit");
static_assert(SH_SLOTS >= 1 && (SH_SLOTS * 257) * 4 <= 65536, "the table must fit a workgroup's 64 KB of LDS");

struct DigitTable {
    uint32_t key[SH_SLOTS];
    uint32_t cnt[SH_SLOTS][256];
};

__device__ __forceinline__ uint32_t find_slot(DigitTable& S, uint32_t key) {
    uint32_t h = hash_u32(key) % (uint32_t)SH_SLOTS;
    for (int probe = 0; probe < SH_PROBE; ++probe) {
        const uint32_t k = atomicCAS(&S.key[h], NO_KEY, key);
        if (k == NO_KEY || k == key) return h;
        h = h + 1u == (uint32_t)SH_SLOTS ? 0u : h + 1u;
    }
    return SLOT_GLOBAL;
}

// Only the first lane of a run of equal `a` in neighbouring lanes gets the run's length, the others 0: one DPP shift, one
// ballot, a count of trailing zeros (kernels_wallsort.hip).  The whole wave must be here.
__device__ __forceinline__ uint32_t run_length_at_head(const uint32_t a, const int lane) {
    const uint32_t before = (uint32_t)__builtin_amdgcn_update_dpp((int)~a, (int)a, 0x138, 0xf, 0xf, false);    // wave_shr:1 (lane 0: no lane before it)
    const bool head = a != before;
    const uint64_t heads = __builtin_amdgcn_ballot_w64(head);
    const uint64_t later = (heads >> 1) >> lane;                                  // the heads behind this lane
    const uint32_t len = later ? (uint32_t)__builtin_ctzll(later) + 1u : 64u - (uint32_t)lane;
    return head ? len : 0u;
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
__device__ __forceinline__ void load_strip(const DigitArgs& A, int64_t p, int64_t r, int64_t c0, uint32_t (&l)[VPL], uint32_t (&s)[VPL]) {
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

// NSEL: the selectors a row has room for in registers (0: a pass without selectors; 2: what a median needs; SH_MAX_RANKS)
template <typename TL, typename TS, int NSEL, bool VEC>
__global__ __launch_bounds__(SH_THREADS) void digit_kernel(const DigitArgs A) {
    constexpr int VPL = 16 / (int)sizeof(TL);
    constexpr bool SEL = NSEL != 0;
    constexpr int NS = SEL ? NSEL : 1;
    __shared__ DigitTable S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < SH_SLOTS; i += SH_THREADS) S.key[i] = NO_KEY;
    for (int i = 0; i < SH_SLOTS; ++i) S.cnt[i][tid] = 0u;
    __syncthreads();

    const int64_t cols = 64 * VPL;
    const int64_t ncb = (A.n2 + cols - 1) / cols, nrb = (A.n1 + SH_WAVES - 1) / SH_WAVES;
    const int64_t npb = (A.n0 - A.first_owned + SH_PLANES - 1) / SH_PLANES;
    const int64_t tiles = ncb * nrb * npb;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_group;
    const int64_t t1 = t0 + A.tiles_per_group < tiles ? t0 + A.tiles_per_group : tiles;
    const uint32_t shift = A.shift, nsel = A.nsel;

    // what survives of the running record: the lane's label, the slot of each of its keys and (SEL) their selectors
    uint32_t cur_l = INVALID_LABEL, spilled = 0u;
    uint32_t slot[NS], selv[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) { slot[k] = SLOT_SKIP; selv[k] = SH_NONE; }

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t cb = t % ncb, rb = (t / ncb) % nrb, pb = t / (ncb * nrb);
        const int64_t r = rb * SH_WAVES + wave;
        if (r >= A.n1) continue;                                   // (wave-uniform)
        const int64_t c0 = cb * cols + (int64_t)lane * VPL;
        const int64_t pbeg = A.first_owned + pb * SH_PLANES;
        const int64_t pend = pbeg + SH_PLANES < A.n0 ? pbeg + SH_PLANES : A.n0;
        uint32_t cl[VPL], cs[VPL];                                 // this plane
        load_strip<TL, TS, VPL, VEC>(A, pbeg, r, c0, cl, cs);
        for (int64_t p = pbeg; p < pend; ++p) {
            const bool more = p + 1 < pend;                        // (wave-uniform)
            uint32_t nl[VPL], ns[VPL];                             // the next plane, in flight while this one is worked on
            if (more) load_strip<TL, TS, VPL, VEC>(A, p + 1, r, c0, nl, ns);
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const uint32_t x = cl[j], s = cs[j];
                uint32_t addr = NO_ADDR;
                if (x != INVALID_LABEL) {
                    if (x != cur_l) {
                        cur_l = x;
                        if (x > A.max_label) {
                            atomicOr(&A.flags[SH_FLAG_RANGE], 1u);
#pragma unroll
                            for (int k = 0; k < NS; ++k) { slot[k] = SLOT_SKIP; selv[k] = SH_NONE; }
                        } else if (SEL) {
#pragma unroll
                            for (int k = 0; k < NS; ++k)                 // (all the loads first: one round trip to the L2, not nsel)
                                if ((uint32_t)k < nsel) selv[k] = A.sel[x * nsel + (uint32_t)k];
#pragma unroll
                            for (int k = 0; k < NS; ++k)
                                if ((uint32_t)k < nsel) slot[k] = selv[k] == SH_NONE ? SLOT_SKIP : find_slot(S, x * nsel + (uint32_t)k);
                        } else {
                            slot[0] = find_slot(S, x);
                        }
                    }
                    const uint32_t d = (s >> shift) & 255u;
                    uint32_t sl = SLOT_SKIP, k_of = 0u;
                    if (SEL) {
                        const uint32_t high = s >> (shift + 8u);
#pragma unroll
                        for (int k = 0; k < NS; ++k)
                            if (selv[k] == high) { sl = slot[k]; k_of = (uint32_t)k; }      // (SH_NONE is no high byte)
                    } else {
                        sl = slot[0];
                    }
                    if (sl == SLOT_GLOBAL) {
                        const uint64_t key = SEL ? (uint64_t)x * nsel + k_of : (uint64_t)x;
                        atomicAdd(&A.counts[key * A.stride + d], 1ull);
                        spilled += 1u;
                    } else if (sl != SLOT_SKIP) {
                        addr = sl * 256u + d;
                    }
                }
                // (lanes without a counter form runs of NO_ADDR, which nobody adds)
                const uint32_t len = run_length_at_head(addr, lane);
                if (len && addr != NO_ADDR) atomicAdd(&S.cnt[0][0] + addr, len);
            }
            if (more) {
#pragma unroll
                for (int j = 0; j < VPL; ++j) { cl[j] = nl[j]; cs[j] = ns[j]; }
            }
        }
    }

    // (the spill counter is one word for the whole device: a wave adds its sum once)
    for (int o = 32; o > 0; o >>= 1) spilled += (uint32_t)__shfl_xor((int)spilled, o);
    if (lane == 0 && spilled) atomicAdd(&A.flags[SH_FLAG_SPILL], spilled);
    __syncthreads();
    for (int i = 0; i < SH_SLOTS; ++i) {
        const uint32_t key = S.key[i];                             // (uniform)
        if (key == NO_KEY) continue;
        const uint32_t c = S.cnt[i][tid];
        if (c) atomicAdd(&A.counts[(uint64_t)key * A.stride + (uint32_t)tid], (unsigned long long)c);
    }
}

// The digit of hist[0 .. 256) that holds the 0-based `rank` and the rank inside it; false when rank >= the sum.  The whole wave.
__device__ __forceinline__ bool wave_select(const unsigned long long* hist, unsigned long long rank, int lane, uint32_t& digit,
                                            unsigned long long& rem) {
    unsigned long long c[4], sum = 0ull;
#pragma unroll
    for (int k = 0; k < 4; ++k) { c[k] = hist[4 * lane + k]; sum += c[k]; }
    unsigned long long incl = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    const unsigned long long total = __shfl(incl, 63);
    unsigned long long below = incl - sum;
    const bool here = rank < total && rank >= below && rank < incl;
    uint32_t d = 0u;
    unsigned long long left = 0ull;
    if (here) {
        d = 4u * (uint32_t)lane;
        left = rank - below;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (d == 4u * (uint32_t)lane + (uint32_t)k && left >= c[k]) { left -= c[k]; d += 1u; }
    }
    const uint64_t who = __builtin_amdgcn_ballot_w64(here);
    if (!who) return false;
    const int src = __builtin_ctzll(who);
    digit = (uint32_t)__shfl((int)d, src);
    rem = __shfl(left, src);
    return true;
}

template <bool FINAL>
__global__ __launch_bounds__(256) void select_first_kernel(const SelectArgs A) {
    const int lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= A.rows) return;                                     // (wave-uniform)
    const unsigned long long* hist = A.counts1 + row * 256;
    const uint64_t base = row * A.nranks;
    for (uint32_t j = 0; j < A.nranks; ++j) {
        uint32_t digit = SH_NONE;
        unsigned long long rem = 0ull;
        if (!wave_select(hist, A.ranks[base + j], lane, digit, rem)) digit = SH_NONE;
        if (lane == 0) {
            if (FINAL) {
                A.values[base + j] = digit;
            } else {
                // the distinct high bytes of the row stay as selectors, each at its first j
                uint32_t first = j;
                for (uint32_t k = 0; k < j; ++k)
                    if (A.hi[base + k] == digit) { first = k; break; }
                A.hi[base + j] = digit;
                A.rem[base + j] = rem;
                A.map[base + j] = first;
                A.sel[base + j] = first == j ? digit : SH_NONE;
            }
        }
    }
}

__global__ __launch_bounds__(256) void select_second_kernel(const SelectArgs A) {
    const int lane = threadIdx.x & 63;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= A.rows) return;                                     // (wave-uniform)
    const uint64_t base = row * A.nranks;
    for (uint32_t j = 0; j < A.nranks; ++j) {
        const uint32_t high = A.hi[base + j];                      // (uniform)
        uint32_t value = SH_NONE;
        if (high != SH_NONE) {
            uint32_t digit = 0u;
            unsigned long long rem = 0ull;
            if (wave_select(A.counts2 + (base + A.map[base + j]) * 256, A.rem[base + j], lane, digit, rem)) value = (high << 8) | digit;
        }
        if (lane == 0) A.values[base + j] = value;
    }
}

template <typename TL, typename TS, int NSEL>
void launch_sel(hipStream_t s, const DigitArgs& a, bool vec, int64_t groups) {
    if (vec) hipLaunchKernelGGL((digit_kernel<TL, TS, NSEL, true>), dim3((unsigned)groups), dim3(SH_THREADS), 0, s, a);
    else hipLaunchKernelGGL((digit_kernel<TL, TS, NSEL, false>), dim3((unsigned)groups), dim3(SH_THREADS), 0, s, a);
}

template <typename TL, typename TS>
void launch_kind(hipStream_t s, const DigitArgs& a, bool vec, int64_t groups) {
    if (a.nsel == 0) launch_sel<TL, TS, 0>(s, a, vec, groups);
    else if (a.nsel <= 2) launch_sel<TL, TS, 2>(s, a, vec, groups);
    else launch_sel<TL, TS, SH_MAX_RANKS>(s, a, vec, groups);
}

}  // namespace

RangePlan launch_sighist_digits(hipStream_t s, DigitArgs a, int label_itemsize, int signal_itemsize) {
    const RangeTiles t = range_tiles(a.n0, a.n1, a.n2, a.first_owned, label_itemsize, SH_RANGE);
    const RangePlan plan = plan_ranges(t.tiles, t.tile_voxels, SH_RANGE);
    if (!plan.groups) return plan;
    a.tiles_per_group = plan.tiles_per_group;
    const bool vec = strips_vectorize(a.n2, label_itemsize, {{a.vol, label_itemsize}, {a.sig, signal_itemsize}});
    if (label_itemsize == 2 && signal_itemsize == 1) launch_kind<uint16_t, uint8_t>(s, a, vec, plan.groups);
    else if (label_itemsize == 2) launch_kind<uint16_t, uint16_t>(s, a, vec, plan.groups);
    else if (signal_itemsize == 1) launch_kind<uint32_t, uint8_t>(s, a, vec, plan.groups);
    else launch_kind<uint32_t, uint16_t>(s, a, vec, plan.groups);
    return plan;
}

void launch_sighist_select_first(hipStream_t s, const SelectArgs& a, bool final) {
    if (!a.rows || !a.nranks) return;
    const unsigned groups = (a.rows + 3u) / 4u;
    if (final) hipLaunchKernelGGL(select_first_kernel<true>, dim3(groups), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(select_first_kernel<false>, dim3(groups), dim3(256), 0, s, a);
}

void launch_sighist_select_second(hipStream_t s, const SelectArgs& a) {
    if (!a.rows || !a.nranks) return;
    hipLaunchKernelGGL(select_second_kernel, dim3((a.rows + 3u) / 4u), dim3(256), 0, s, a);
}

}  // namespace ta
