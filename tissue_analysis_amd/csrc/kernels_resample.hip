// kernels_resample.hip -- a source volume S of any dims sampled through an affine map onto the grid of the resident label volume
// (include/tissue_scan_resample.h): nearest neighbour for labels, trilinear for signals, `fill` outside the source.
//
// Layout of the pass: output-stationary.  Every output voxel is written exactly once, by one store, and what is scattered is the
// READ side, which the caches serve: a gather.  (Source-stationary -- stream S, scatter into the output -- would leave holes under
// a zoom, write twice under a shrink and need atomics for neither.)  A tile is RS_WAVES rows x (64 lanes x VPL columns) x
// RS_PLANES planes of the target, VPL = 16 / sizeof(item): every wave owns one row of it and walks the planes, each lane producing
// one 16-byte strip of outputs along memory axis 2 a plane and writing it with one store.  A tile is a compact brick of the
// target -- 4 planes x 4 rows x one strip-row -- so under any rotation its footprint in S is a compact brick too (a slanted beam a
// few lines thick), not a sheet: the lines of S that the four rows and four planes share are fetched once and hit in L2 after
// that.  A workgroup takes a contiguous range of tiles (column blocks first, then row blocks, then plane blocks: ta_range_plan.h),
// so its next brick borders the last one.  Rows that are not whole strips, or an output that is not 16-byte aligned, take the
// scalar stores (strips_vectorize).  The loads of S are item-sized, from any address aligned to the item.
//
// The coordinate arithmetic IS the contract: s_x = ((A[x][0] * i0 + A[x][1] * i1) + A[x][2] * i2) + A[x][3] in IEEE double, every
// product and sum rounded on its own.  Device code is compiled with contraction on by default, under which a * b + c becomes one
// fused multiply-add of another rounding -- so contraction is OFF for this whole file (the pragma below, and -ffp-contract=off in
// build.py for good measure).  The products with the row's and plane's indices are the same for a whole strip and the compiler is
// free to hoist them: that does not change a rounding.  Nothing steps s along the strip: s + A[x][2] would round differently.
//
// outside: a lane counts the owned voxels it filled; one wave reduction and one 64-bit atomic a wave, at the end of its range.
#include "ta_resample.h"

#pragma clang fp contract(off)

namespace ta {
namespace {

constexpr int RS_WAVES = 4;                        // rows of a tile = waves of a workgroup
constexpr int RS_THREADS = RS_WAVES * 64;
constexpr int RS_PLANES = 4;                       // planes of a tile
constexpr int64_t RS_MAX_GROUPS = 4096;            // sixteen workgroups a CU: the gather wants many loads in flight
// a lane counts the voxels it filled in u32: fewer than 2^31 voxels a workgroup
constexpr RangeShape RS_RANGE = {RS_WAVES, RS_PLANES, RS_MAX_GROUPS, 31};

template <typename T>
__device__ __forceinline__ double src_at(const ResampleArgs& A, int64_t q0, int64_t q1, int64_t q2) {
    return (double)((const T*)A.src)[q0 * A.es[0] + q1 * A.es[1] + q2 * A.es[2]];
}

__device__ __forceinline__ int64_t clamp_index(int64_t q, int64_t m) { return q < 0 ? 0 : (q > m - 1 ? m - 1 : q); }

// the value of target voxel (i[0], i[1], i[2]) (array-axis order, as doubles); *filled: it received `fill`
template <typename T, int MODE>
__device__ __forceinline__ uint32_t sample(const ResampleArgs& A, const double (&i)[3], bool* filled) {
    double s[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const double t01 = A.A[4 * x + 0] * i[0] + A.A[4 * x + 1] * i[1];      // (no contraction in this file: see the top)
        const double t012 = t01 + A.A[4 * x + 2] * i[2];
        s[x] = t012 + A.A[4 * x + 3];
    }
    if (MODE == RS_NEAREST) {
        double q[3];
        bool in = true;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            q[x] = floor(s[x] + 0.5);
            in = in && q[x] >= 0.0 && q[x] < (double)A.m[x];                   // (false for a NaN)
        }
        *filled = !in;
        if (!in) return A.fill;
        // (0 <= q < m <= 2^30: the conversion is exact in 32 bits)
        return (uint32_t)((const T*)A.src)[(int64_t)(int32_t)q[0] * A.es[0] + (int64_t)(int32_t)q[1] * A.es[1] + (int64_t)(int32_t)q[2] * A.es[2]];
    } else {
        bool in = true;
#pragma unroll
        for (int x = 0; x < 3; ++x) in = in && s[x] >= -0.5 && s[x] < (double)A.m[x] - 0.5;
        *filled = !in;
        if (!in) return A.fill;
        int64_t lo[3], hi[3];
        double w[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const double f = floor(s[x]);
            w[x] = s[x] - f;
            lo[x] = clamp_index((int64_t)(int32_t)f, A.m[x]);              // (-1 <= f < m <= 2^30: exact in 32 bits)
            hi[x] = clamp_index((int64_t)(int32_t)f + 1, A.m[x]);
        }
        double v0[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int64_t q0 = a ? hi[0] : lo[0];
            double v1[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int64_t q1 = b ? hi[1] : lo[1];
                const double c0 = src_at<T>(A, q0, q1, lo[2]), c1 = src_at<T>(A, q0, q1, hi[2]);
                v1[b] = c0 + w[2] * (c1 - c0);
            }
            v0[a] = v1[0] + w[1] * (v1[1] - v1[0]);
        }
        const double v = v0[0] + w[0] * (v0[1] - v0[0]);
        return (uint32_t)rint(v);                                              // (half to even; inside the type's range)
    }
}

template <typename T, int MODE, bool VEC>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const ResampleArgs A) {
    constexpr int VPL = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cols = 64 * VPL;
    // (the halo plane is written like the others: the tiles cover the whole buffer)
    const int64_t ncb = (A.n2 + cols - 1) / cols, nrb = (A.n1 + RS_WAVES - 1) / RS_WAVES, npb = (A.n0 + RS_PLANES - 1) / RS_PLANES;
    const int64_t tiles = ncb * nrb * npb;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_group;
    const int64_t t1 = t0 + A.tiles_per_group < tiles ? t0 + A.tiles_per_group : tiles;
    uint32_t filled_owned = 0u;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t cb = t % ncb, rb = (t / ncb) % nrb, pb = t / (ncb * nrb);
        const int64_t r = rb * RS_WAVES + wave;
        if (r >= A.n1) continue;                                   // (wave-uniform)
        const int64_t c0 = cb * cols + (int64_t)lane * VPL;
        const int64_t left = A.n2 - c0;
        const int valid = left >= VPL ? VPL : (left > 0 ? (int)left : 0);
        if (!valid) continue;
        const int64_t pbeg = pb * RS_PLANES;
        const int64_t pend = pbeg + RS_PLANES < A.n0 ? pbeg + RS_PLANES : A.n0;
        for (int64_t p = pbeg; p < pend; ++p) {
            const bool owned = p >= A.first_owned;
            // memory-axis indices of the strip's first voxel, global along axis 0; then the same in array-axis order
            const double g[2] = {(double)(p - A.first_owned + A.a_origin), (double)(int32_t)r};
            T* const out = (T*)A.out + (p * A.n1 + r) * A.n2 + c0;
            uint32_t v[VPL];
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                v[j] = 0u;
                if (!VEC && j >= valid) continue;
                const double c = (double)(int32_t)(c0 + j);
                double i[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) i[a] = A.mem_of[a] == 0 ? g[0] : (A.mem_of[a] == 1 ? g[1] : c);
                bool filled;
                v[j] = sample<T, MODE>(A, i, &filled);
                filled_owned += filled && owned ? 1u : 0u;
            }
            if (VEC) {
                constexpr int IPW = 4 / (int)sizeof(T);            // items a 32-bit word
                constexpr uint32_t MASK = (uint32_t)(T)~(T)0;      // (`fill` is truncated to the type)
                uint32_t w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    w[k] = 0u;
#pragma unroll
                    for (int b = 0; b < IPW; ++b) w[k] |= (v[k * IPW + b] & MASK) << (8 * (int)sizeof(T) * b);
                }
                *reinterpret_cast<uint4*>(out) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int j = 0; j < VPL; ++j)
                    if (j < valid) out[j] = (T)v[j];
            }
        }
    }

    for (int o = 32; o > 0; o >>= 1) filled_owned += (uint32_t)__shfl_xor((int)filled_owned, o);
    if (lane == 0 && filled_owned) atomicAdd(A.outside, (unsigned long long)filled_owned);
}

template <typename T, int MODE>
void launch_vec(hipStream_t s, const ResampleArgs& a, bool vec, uint32_t groups) {
    if (vec) hipLaunchKernelGGL((resample_kernel<T, MODE, true>), dim3(groups), dim3(RS_THREADS), 0, s, a);
    else hipLaunchKernelGGL((resample_kernel<T, MODE, false>), dim3(groups), dim3(RS_THREADS), 0, s, a);
}

}  // namespace

RangePlan launch_resample(hipStream_t s, ResampleArgs a, int itemsize, int mode, bool* vec_out) {
    const RangeTiles t = range_tiles(a.n0, a.n1, a.n2, 0, itemsize, RS_RANGE);      // (first_owned 0: the halo plane is written too)
    const RangePlan plan = plan_ranges(t.tiles, t.tile_voxels, RS_RANGE);
    const bool vec = strips_vectorize(a.n2, itemsize, {{a.out, itemsize}});
    if (vec_out) *vec_out = vec;
    if (!plan.groups) return plan;
    a.tiles_per_group = plan.tiles_per_group;
    if (mode == RS_NEAREST) {
        if (itemsize == 1) launch_vec<uint8_t, RS_NEAREST>(s, a, vec, plan.groups);
        else if (itemsize == 2) launch_vec<uint16_t, RS_NEAREST>(s, a, vec, plan.groups);
        else launch_vec<uint32_t, RS_NEAREST>(s, a, vec, plan.groups);
    } else {
        if (itemsize == 1) launch_vec<uint8_t, RS_LINEAR>(s, a, vec, plan.groups);
        else launch_vec<uint16_t, RS_LINEAR>(s, a, vec, plan.groups);
    }
    return plan;
}

}  // namespace ta
