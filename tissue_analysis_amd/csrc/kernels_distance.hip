// kernels_distance.hip -- exact squared Euclidean distance maps of the label volume (include/tissue_scan_distance.h).
//
// Every voxel has its own site set (the voxels of another class than its own), and the transform still separates over the axes: along
// a line, inside a maximal run [lo, hi) of equal class, the voxel just outside either end is a site at distance 0 along the axes
// done so far, and it dominates everything behind it.  So the answer inside the run is the lower envelope of the run's own parabolas
// f(j) + w^2 (i - j)^2, a zero parabola at lo - 1 and a zero parabola at hi (an end outside the image exists with EDGE_IS_SITE only).
//   rows      memory axis 2: no envelope, f = (w * min(i - lo + 1, hi - i))^2
//   columns   memory axis 1, then 0: one lane per column, neighbouring lanes on neighbouring axis-2 positions, so that every step of
//             the walk is a coalesced access.  Forwards: the sequential lower envelope (Felzenszwalb-Huttenlocher) of the own parabolas
//             of every run, on a stack laid out [entry][column]; the zero parabola of the left end goes in place of f, which the stack
//             keeps where a later step still needs it.  Backwards: the envelope, the left end and the right end, whichever is lowest.
//   table     atomicMin / atomicMax on the bit patterns of the non-negative doubles per row, then atomicMin of the array-order index
//             where D2 equals the row's maximum; both compare with the row's current value before they send.
// All arithmetic is float64; the class of a voxel is its label (mode 0) or whether it is the site label (mode 1).
#include "ta_distance.h"

#include <cmath>

namespace ta {

namespace {

constexpr double DINF = __builtin_huge_val();

template <typename T>
__device__ __forceinline__ uint32_t voxel_class(const DistanceArgs& a, uint64_t idx) {
    const uint32_t l = (uint32_t)((const T*)a.vol)[idx];
    return a.mode ? (uint32_t)(a.has_site && l == a.site) : l;
}

__device__ __forceinline__ double sq(double x) { return x * x; }

// One wave per row.  The distance to the last change of class is carried from chunk to chunk: forwards the start of the run, then
// backwards its end (a run may be longer than the 64 voxels a wave holds at once).
template <typename T>
__global__ __launch_bounds__(256) void distance_row_kernel(DistanceArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * 4, rows = (uint64_t)a.n0 * (uint64_t)a.n1;
    const int64_t n2 = a.n2;
    const bool edge = a.flags & DIST_EDGE_IS_SITE;
    const double w = a.w[2];
    for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += nwaves) {
        const uint64_t at = row * (uint64_t)n2;
        // forwards: voxels to the site in front of the run's start, itself included; +inf when there is none
        int64_t start = 0;
        uint32_t carry = 0;
        for (int64_t b = 0; b < n2; b += 64) {
            const int64_t i = b + lane;
            const bool valid = i < n2;
            const uint32_t c = valid ? voxel_class<T>(a, at + (uint64_t)i) : 0u;
            uint32_t before = (uint32_t)__shfl_up((int)c, 1);
            if (lane == 0) before = carry;
            const uint64_t m = __ballot(valid && (i == 0 || c != before));
            const uint64_t mine = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
            const int64_t s = mine ? b + 63 - __builtin_clzll(mine) : start;
            if (valid) a.d2[at + (uint64_t)i] = (s > 0 || edge) ? (double)(i - s + 1) : DINF;
            if (m) start = b + 63 - __builtin_clzll(m);
            carry = (uint32_t)__shfl((int)c, 63);
        }
        // backwards: the same to the site behind the run's end, and the smaller of the two
        int64_t end = n2 - 1;
        const int64_t last = ((n2 - 1) / 64) * 64;
        for (int64_t b = last; b >= 0; b -= 64) {
            const int64_t i = b + lane;
            const bool valid = i < n2;
            const uint32_t c = valid ? voxel_class<T>(a, at + (uint64_t)i) : 0u;
            uint32_t after = (uint32_t)__shfl_down((int)c, 1);
            if (lane == 63) after = carry;
            const uint64_t m = __ballot(valid && (i == n2 - 1 || c != after));
            const uint64_t mine = m & (~0ull << lane);
            const int64_t e = mine ? b + __builtin_ctzll(mine) : end;
            if (valid) {
                const double left = a.d2[at + (uint64_t)i];
                const double right = (e < n2 - 1 || edge) ? (double)(e + 1 - i) : DINF;
                a.d2[at + (uint64_t)i] = (a.mode && c) ? 0.0 : sq(w * fmin(left, right));
            }
            if (m) end = b + __builtin_ctzll(m);
            carry = (uint32_t)__shfl((int)c, 0);
        }
    }
}

// One lane per column.  Entry k of a column's stack: position sv, f at that position sf, left boundary sz; the top entry is kept in
// registers too.  Every run opens with an entry of its own at lo - 1/2 (f may be +inf there: it is replaced by the run's first
// finite parabola, and never meets the intersection formula, where inf - inf would be a NaN), so a column of len voxels needs at
// most len entries, and the backward walk finds the end of a run's entries by the boundaries alone.
template <typename T>
__global__ __launch_bounds__(256) void distance_column_kernel(DistanceArgs a, int64_t len, uint64_t step, uint64_t inner, uint64_t outer_stride,
                                                              double w, uint64_t first, uint64_t columns, int32_t* sv, double* sf, double* sz,
                                                              uint64_t stride) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= columns) return;
    const uint64_t col = first + t;
    const uint64_t base = (col / inner) * outer_stride + (col % inner);
    const bool edge = a.flags & DIST_EDGE_IS_SITE;
    const double w2 = w * w;
    int64_t k = -1, run_base = 0, lo = 0;
    uint32_t cur = 0;
    int32_t tv = 0;
    double tf = DINF, tz = 0.0;
    for (int64_t i = 0; i < len; ++i) {
        const uint64_t idx = base + (uint64_t)i * step;
        const uint32_t c = voxel_class<T>(a, idx);
        const double f = a.d2[idx];
        if (i == 0 || c != cur) {
            cur = c; lo = i;
            ++k; run_base = k;
            tv = (int32_t)i; tf = f; tz = (double)i - 0.5;
            const uint64_t e = (uint64_t)k * stride + t;
            sv[e] = tv; sf[e] = tf; sz[e] = tz;
        } else if (f < DINF) {
            for (;;) {
                double s = 0.0;
                bool replace = !(tf < DINF);
                if (!replace) {
                    s = ((f + w2 * sq((double)i)) - (tf + w2 * sq((double)tv))) / (2.0 * w2 * (double)(i - tv));
                    replace = s <= tz && k == run_base;
                }
                if (replace) {                           // the run's first entry: it keeps its boundary at lo - 1/2
                    tv = (int32_t)i; tf = f;
                    const uint64_t e = (uint64_t)k * stride + t;
                    sv[e] = tv; sf[e] = tf;
                    break;
                }
                if (s <= tz) {
                    --k;
                    const uint64_t e = (uint64_t)k * stride + t;
                    tv = sv[e]; tf = sf[e]; tz = sz[e];
                } else {
                    ++k;
                    tv = (int32_t)i; tf = f; tz = s;
                    const uint64_t e = (uint64_t)k * stride + t;
                    sv[e] = tv; sf[e] = tf; sz[e] = tz;
                    break;
                }
            }
        }
        a.d2[idx] = (lo > 0 || edge) ? sq(w * (double)(i - lo + 1)) : DINF;
    }
    int64_t hi = len;
    for (int64_t i = len - 1; i >= 0; --i) {
        const uint64_t idx = base + (uint64_t)i * step;
        const uint32_t c = voxel_class<T>(a, idx);
        const double left = a.d2[idx];
        if (i == len - 1 || c != cur) { cur = c; hi = i + 1; }
        const double right = (hi < len || edge) ? sq(w * (double)(hi - i)) : DINF;
        while (tz > (double)i && k > 0) {
            --k;
            const uint64_t e = (uint64_t)k * stride + t;
            tv = sv[e]; tf = sf[e]; tz = sz[e];
        }
        const double own = tf < DINF ? tf + sq(w * (double)(i - tv)) : DINF;
        a.d2[idx] = fmin(fmin(own, left), right);
    }
}

__device__ __forceinline__ unsigned long long row_load(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void distance_table_init_kernel(DistanceTable t) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x, rows = (uint64_t)t.max_label + 1;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += nthreads) {
        t.min2[r] = (unsigned long long)__double_as_longlong(DINF);
        t.max2[r] = 0ull;
        t.pole[r] = DIST_NO_POLE;
    }
    if (blockIdx.x == 0 && threadIdx.x < DIST_NFLAGS) t.flags[threadIdx.x] = 0u;
}

template <typename T>
__global__ __launch_bounds__(256) void distance_extremes_kernel(DistanceArgs a, DistanceTable t, uint64_t nvox) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvox; v += nthreads) {
        const uint32_t l = (uint32_t)((const T*)a.vol)[v];
        if (l > t.max_label) { atomicOr(&t.flags[DIST_FLAG_RANGE], 1u); continue; }
        const unsigned long long bits = (unsigned long long)__double_as_longlong(a.d2[v]);
        if (bits < row_load(t.min2 + l)) (void)__hip_atomic_fetch_min(t.min2 + l, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (bits > row_load(t.max2 + l)) (void)__hip_atomic_fetch_max(t.max2 + l, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void distance_pole_kernel(DistanceArgs a, DistanceTable t, uint64_t nvox) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t plane = (uint64_t)a.n1 * (uint64_t)a.n2;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvox; v += nthreads) {
        const uint32_t l = (uint32_t)((const T*)a.vol)[v];
        if (l > t.max_label) continue;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(a.d2[v]);
        if (bits != row_load(t.max2 + l)) continue;
        const uint64_t q = v / plane, rest = v - q * plane, r = rest / (uint64_t)a.n2, c = rest - r * (uint64_t)a.n2;
        const unsigned long long key = q * t.key_stride[0] + r * t.key_stride[1] + c * t.key_stride[2];
        if (key < row_load(t.pole + l)) (void)__hip_atomic_fetch_min(t.pole + l, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

uint32_t launch_distance_rows(hipStream_t s, const DistanceArgs& a, int itemsize) {
    const uint64_t rows = (uint64_t)a.n0 * (uint64_t)a.n1;
    const uint32_t grid = blocks_for(rows * 64, DIST_ROW_MAX_GROUPS);
    if (itemsize == 2) hipLaunchKernelGGL(distance_row_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(distance_row_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, a);
    return grid;
}

void launch_distance_columns(hipStream_t s, const DistanceArgs& a, int itemsize, int axis, uint64_t first, uint64_t columns, void* work,
                             uint64_t stride) {
    const ColumnPass g = column_pass(a.n0, a.n1, a.n2, axis);
    double* sf = (double*)work;
    double* sz = sf + (uint64_t)g.len * stride;
    int32_t* sv = (int32_t*)(sz + (uint64_t)g.len * stride);
    const uint32_t grid = column_grid(columns);
    if (itemsize == 2)
        hipLaunchKernelGGL(distance_column_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, a, g.len, g.step, g.inner, g.outer_stride, a.w[axis],
                           first, columns, sv, sf, sz, stride);
    else
        hipLaunchKernelGGL(distance_column_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, a, g.len, g.step, g.inner, g.outer_stride, a.w[axis],
                           first, columns, sv, sf, sz, stride);
}

void launch_distance_table(hipStream_t s, const DistanceArgs& a, int itemsize, const DistanceTable& t, DistanceLaunch& launched) {
    const uint64_t nvox = (uint64_t)a.n0 * (uint64_t)a.n1 * (uint64_t)a.n2;
    const uint32_t grid = blocks_for(nvox, DIST_VOXEL_MAX_GROUPS), init = blocks_for((uint64_t)t.max_label + 1, DIST_INIT_MAX_GROUPS);
    launched.voxel_groups = grid;
    launched.init_groups = init;
    hipLaunchKernelGGL(distance_table_init_kernel, dim3(init), dim3(256), 0, s, t);
    if (itemsize == 2) {
        hipLaunchKernelGGL(distance_extremes_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, a, t, nvox);
        hipLaunchKernelGGL(distance_pole_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, a, t, nvox);
    } else {
        hipLaunchKernelGGL(distance_extremes_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, a, t, nvox);
        hipLaunchKernelGGL(distance_pole_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, a, t, nvox);
    }
}

}  // namespace ta
