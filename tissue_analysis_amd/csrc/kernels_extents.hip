// kernels_extents.hip -- oriented extents per label (include/tissue_scan_extents.h): lo = min p and hi = max p of three float64
// projections p = (x0 w[k][0] + x1 w[k][1]) + x2 w[k][2] of the voxel indices, the weights a row of a per-label table, in one
// streaming pass over the labels.
//
// Layout of the pass: that of kernels_sigmoments.hip.  A tile is EX_WAVES rows x (64 lanes x VPL columns) x EX_PLANES planes; every
// wave owns one row of it and walks the planes, each lane holding a strip of VPL = 16 / sizeof(label) voxels along memory axis 2.
// The next plane's strip is loaded while the current one is worked on.  A workgroup takes a contiguous range of tiles and keeps one
// LDS table label -> (lo[3], hi[3]) for the whole range, which it flushes with global atomics once, at its end.
//
// Arithmetic.  The file is compiled with -ffp-contract=off (build.EXTRA_FLAGS): __dmul_rn / __dadd_rn and a contract(off) pragma do
// not keep hipcc -O3 from fusing the products into v_fmac_f64, the flag does.  Inside a strip x0 and x1 are fixed, so
// a[k] = x0 w[k][0] + x1 w[k][1] is formed once per plane step and label, and a voxel costs one product, one sum, one v_min_f64
// and one v_max_f64 per direction.  Every voxel is evaluated.  (Every rounding step is monotone, so the two ends of a run of one
// label inside a strip would bound the run exactly; skipping the voxels between them was built and measured 1 - 2 % SLOWER: some
// lane of the 64 has a run end at nearly every column of the strip, so the wave skips nothing and pays for the tests.  DESIGN.md.)
//
// Merging.  A lane keeps the six float64 of the label it is on; when the label changes they become order-preserving u64 keys
// (ta_extents.h) and go to the LDS table with ds_min_u64 / ds_max_u64, at the end of the range to the global rows with
// global_atomic_umin_x2 / umax_x2.  Minima and maxima of integers: bit-identical whatever the order of the atomics.
#include "ta_extents.h"

namespace ta {
namespace {

constexpr int EX_WAVES = 4;                        // rows of a tile = waves of a workgroup
constexpr int EX_THREADS = EX_WAVES * 64;
constexpr int EX_PLANES = 16;                      // planes of a tile
constexpr int EX_PROBE = 32;                       // probes before a record goes to the global rows directly
// no u32 counter in the table: a workgroup's voxels are bounded by nothing but plan_ranges' own shift
constexpr RangeShape EX_RANGE = {EX_WAVES, EX_PLANES, EX_MAX_GROUPS, 62};

struct ExtTable {
    uint32_t key[EX_SLOTS];
    unsigned long long lo[3][EX_SLOTS], hi[3][EX_SLOTS];
};
// 39 936 bytes of LDS a workgroup; four workgroups of 256 threads a CU are four waves a SIMD: 128 VGPRs at most, the build takes
// 96 (uint16 labels) and 80 (uint32), no scratch
static_assert(sizeof(ExtTable) == 52 * EX_SLOTS && 4 * sizeof(ExtTable) <= 160 * 1024, "four workgroups a CU");

__device__ __forceinline__ unsigned long long key_of(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);      // (-0.0 + 0.0 == +0.0)
    return (b >> 63) ? ~b : b | (1ull << 63);
}

// a lane's running record: the extremes of the voxels of one label, and that label's weights
struct Rec {
    double w[3][3], mn[3], mx[3];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < 3; ++k) { mn[k] = __longlong_as_double(0x7FF0000000000000ll); mx[k] = __longlong_as_double((long long)0xFFF0000000000000ull); }
    }
};

__device__ void keys_merge_global(const ExtentArgs& A, uint32_t l, const unsigned long long (&lo)[3], const unsigned long long (&hi)[3]) {
    if (l > A.max_label) { atomicOr(&A.flags[EX_FLAG_RANGE], 1u); return; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        atomicMin(&A.lo[3 * (uint64_t)l + k], lo[k]);
        atomicMax(&A.hi[3 * (uint64_t)l + k], hi[k]);
    }
}

__device__ __forceinline__ void keys_merge_lds(ExtTable& S, const ExtentArgs& A, uint32_t l, const unsigned long long (&lo)[3],
                                               const unsigned long long (&hi)[3]) {
    uint32_t h = __umulhi(hash_u32(l), (uint32_t)EX_SLOTS);
    for (int probe = 0; probe < EX_PROBE; ++probe) {
        const uint32_t k = atomicCAS(&S.key[h], INVALID_LABEL, l);
        if (k == INVALID_LABEL || k == l) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { atomicMin(&S.lo[i][h], lo[i]); atomicMax(&S.hi[i][h], hi[i]); }
            return;
        }
        h = h + 1 == (uint32_t)EX_SLOTS ? 0u : h + 1;
    }
    atomicAdd(&A.flags[EX_FLAG_SPILL], 1u);
    keys_merge_global(A, l, lo, hi);
}

__device__ __forceinline__ void rec_merge_lds(ExtTable& S, const ExtentArgs& A, uint32_t l, const Rec& R) {
    const unsigned long long lo[3] = {key_of(R.mn[0]), key_of(R.mn[1]), key_of(R.mn[2])};
    const unsigned long long hi[3] = {key_of(R.mx[0]), key_of(R.mx[1]), key_of(R.mx[2])};
    keys_merge_lds(S, A, l, lo, hi);
}

// the strip of row r of plane p that starts at column c0: labels, INVALID_LABEL past the row's end.  VEC: every strip is whole or
// wholly outside the row (n2 % VPL == 0) and the buffer is aligned for the 16-byte load.
template <typename TL, int VPL, bool VEC>
__device__ __forceinline__ void load_strip(const ExtentArgs& A, int64_t p, int64_t r, int64_t c0, uint32_t (&l)[VPL]) {
    const int64_t base = (p * A.n1 + r) * A.n2 + c0;
    if (VEC) {
        if (c0 < A.n2) {
            const uint4 v = *reinterpret_cast<const uint4*>((const TL*)A.vol + base);
            uint32_t w[4];
            __builtin_memcpy(w, &v, 16);
#pragma unroll
            for (int j = 0; j < VPL; ++j) l[j] = sizeof(TL) == 4 ? w[j] : (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        } else {
#pragma unroll
            for (int j = 0; j < VPL; ++j) l[j] = INVALID_LABEL;
        }
    } else {
#pragma unroll
        for (int j = 0; j < VPL; ++j) l[j] = c0 + j < A.n2 ? (uint32_t)((const TL*)A.vol)[base + j] : INVALID_LABEL;
    }
}

template <typename TL, bool VEC>
__global__ __launch_bounds__(EX_THREADS) void extents_kernel(const ExtentArgs A) {
    constexpr int VPL = 16 / (int)sizeof(TL);
    __shared__ ExtTable S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < EX_SLOTS; i += EX_THREADS) {
        S.key[i] = INVALID_LABEL;
#pragma unroll
        for (int k = 0; k < 3; ++k) { S.lo[k][i] = EX_KEY_POS_INF; S.hi[k][i] = EX_KEY_NEG_INF; }
    }
    __syncthreads();

    const int64_t cols = 64 * VPL;
    const int64_t ncb = (A.n2 + cols - 1) / cols, nrb = (A.n1 + EX_WAVES - 1) / EX_WAVES;
    const int64_t npb = (A.n0 + EX_PLANES - 1) / EX_PLANES;
    const int64_t tiles = ncb * nrb * npb;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_group;
    const int64_t t1 = t0 + A.tiles_per_group < tiles ? t0 + A.tiles_per_group : tiles;

    uint32_t acc_l = INVALID_LABEL;                                // the label of the lane's running record
    Rec R;
    R.clear();
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) R.w[k][d] = 0.0;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t cb = t % ncb, rb = (t / ncb) % nrb, pb = t / (ncb * nrb);
        const int64_t r = rb * EX_WAVES + wave;
        if (r >= A.n1) continue;                                   // (wave-uniform)
        const int64_t c0 = cb * cols + (int64_t)lane * VPL;
        const int64_t pbeg = pb * EX_PLANES;
        const int64_t pend = pbeg + EX_PLANES < A.n0 ? pbeg + EX_PLANES : A.n0;
        const double x1 = (double)(int32_t)r;
        uint32_t cl[VPL];                                          // this plane
        load_strip<TL, VPL, VEC>(A, pbeg, r, c0, cl);
        for (int64_t p = pbeg; p < pend; ++p) {
            const bool more = p + 1 < pend;                        // (wave-uniform)
            uint32_t nl[VPL];                                      // the next plane, in flight while this one is worked on
            if (more) load_strip<TL, VPL, VEC>(A, p + 1, r, c0, nl);
            const double x0 = (double)(int32_t)p;
            double a[3];                                           // x0 w[k][0] + x1 w[k][1] of the running label
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] = x0 * R.w[k][0] + x1 * R.w[k][1];
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const uint32_t x = cl[j];
                if (x == INVALID_LABEL) continue;
                if (x != acc_l) {
                    if (acc_l != INVALID_LABEL) rec_merge_lds(S, A, acc_l, R);
                    R.clear();
                    acc_l = x;
                    // (a label above max_label reads the last row's weights; its record is dropped where the range flag is raised)
                    const double* w = A.weights + 9 * (uint64_t)(x < A.max_label ? x : A.max_label);
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
#pragma unroll
                        for (int d = 0; d < 3; ++d) R.w[k][d] = w[3 * k + d];
                        a[k] = x0 * R.w[k][0] + x1 * R.w[k][1];
                    }
                }
                const double x2 = (double)(int32_t)(c0 + j);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double pk = a[k] + x2 * R.w[k][2];
                    R.mn[k] = fmin(pk, R.mn[k]);                   // (no NaN can occur; the sign of a zero is settled by key_of)
                    R.mx[k] = fmax(pk, R.mx[k]);
                }
            }
            if (more) {
#pragma unroll
                for (int j = 0; j < VPL; ++j) cl[j] = nl[j];
            }
        }
    }

    // the lanes' last records: reduced across the wave one label at a time, the first lane of the label merges them into the table
    for (;;) {
        const uint64_t pending = __ballot(acc_l != INVALID_LABEL);
        if (!pending) break;
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const uint32_t L = (uint32_t)__shfl((int)acc_l, leader);
        const bool mine = acc_l == L;
        unsigned long long lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = mine ? key_of(R.mn[k]) : EX_KEY_POS_INF;
            hi[k] = mine ? key_of(R.mx[k]) : EX_KEY_NEG_INF;
        }
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned long long ol = __shfl_xor(lo[k], o), oh = __shfl_xor(hi[k], o);
                lo[k] = ol < lo[k] ? ol : lo[k];
                hi[k] = oh > hi[k] ? oh : hi[k];
            }
        }
        if (lane == leader) keys_merge_lds(S, A, L, lo, hi);
        if (mine) acc_l = INVALID_LABEL;
    }
    __syncthreads();
    for (int i = tid; i < EX_SLOTS; i += EX_THREADS) {
        const uint32_t l = S.key[i];
        if (l == INVALID_LABEL) continue;
        const unsigned long long lo[3] = {S.lo[0][i], S.lo[1][i], S.lo[2][i]};
        const unsigned long long hi[3] = {S.hi[0][i], S.hi[1][i], S.hi[2][i]};
        keys_merge_global(A, l, lo, hi);
    }
}

__global__ __launch_bounds__(256) void extents_fill_kernel(unsigned long long* lo, unsigned long long* hi, uint64_t count) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
        lo[i] = EX_KEY_POS_INF;
        hi[i] = EX_KEY_NEG_INF;
    }
}

template <typename TL>
void launch_type(hipStream_t s, const ExtentArgs& a, bool vec, uint32_t groups) {
    if (vec) hipLaunchKernelGGL((extents_kernel<TL, true>), dim3(groups), dim3(EX_THREADS), 0, s, a);
    else hipLaunchKernelGGL((extents_kernel<TL, false>), dim3(groups), dim3(EX_THREADS), 0, s, a);
}

}  // namespace

RangePlan extents_plan(const int64_t dims[3], int label_itemsize) {
    const RangeTiles t = range_tiles(dims[0], dims[1], dims[2], 0, label_itemsize, EX_RANGE);
    return plan_ranges(t.tiles, t.tile_voxels, EX_RANGE);
}

void launch_extents_fill(hipStream_t s, unsigned long long* lo, unsigned long long* hi, uint64_t count) {
    if (!count) return;
    const uint64_t blocks = (count + 255) / 256;
    hipLaunchKernelGGL(extents_fill_kernel, dim3((uint32_t)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, lo, hi, count);
}

void launch_extents(hipStream_t s, ExtentArgs a, int label_itemsize, const RangePlan& plan) {
    if (!plan.groups) return;
    a.tiles_per_group = plan.tiles_per_group;
    const bool vec = strips_vectorize(a.n2, label_itemsize, {{a.vol, label_itemsize}});
    if (label_itemsize == 2) launch_type<uint16_t>(s, a, vec, plan.groups);
    else launch_type<uint32_t>(s, a, vec, plan.groups);
}

}  // namespace ta
