// kernels_nearest.hip -- exact nearest-label maps of the label volume (include/tissue_scan_nearest.h).
//
// One global site set (every voxel that is neither empty nor of the excluded label), so the transform is the plain separable one, and
// every pass carries the label of the nearest site beside the squared distance.  Where several sites are equally near the smallest
// label wins, in every pass: the minimum over a union is the minimum of the minima, so the three passes together give the smallest
// label among all sites at the minimal distance in 3-D.
//   rows      memory axis 2: no envelope.  The site mask of 64 voxels is one ballot; clz and ctz give the nearest site to the left
//             and to the right; position and label of the last site are carried from chunk to chunk, forwards and then backwards.
//   columns   memory axis 1, then 0: one lane per column, neighbouring lanes on neighbouring axis-2 positions, so that every step of
//             the walk is a coalesced access.  Forwards: the sequential lower envelope (Felzenszwalb-Huttenlocher) of the parabolas
//             f(v) + w^2 (i - v)^2 on a stack laid out [entry][column].  An entry holds, beside position, f and left boundary z, its
//             label and a BOUNDARY label b: the smallest label of the parabolas that were popped because they met it exactly at z
//             (they are lowest at that one point only).  Backwards: the entry k with z(k) <= i < z(k + 1); where z(k) == i the
//             entries k and k - 1 and the parabolas behind b(k) all attain the value there.
//   counts    a streaming pass over the empty voxels: gained[N] += 1 where filled, and the two totals.
//   apply     a streaming pass: V = N where filled.
// All arithmetic is float64.  The boundary is the formula of kernels_distance.hip: exact numerator and denominator for power-of-two
// spacings and a correctly rounded quotient, which is what makes the == below mean what they say.
#include "ta_nearest.h"

#include <cmath>

namespace ta {

namespace {

constexpr double DINF = __builtin_huge_val();

template <typename T>
__device__ __forceinline__ uint32_t voxel_label(const NearestArgs& a, uint64_t idx) { return (uint32_t)((const T*)a.vol)[idx]; }
__device__ __forceinline__ bool is_empty(const NearestArgs& a, uint32_t l) { return a.has_empty && l == a.empty; }
__device__ __forceinline__ bool is_site(const NearestArgs& a, uint32_t l) { return !is_empty(a, l) && !(a.has_not_from && l == a.not_from); }
__device__ __forceinline__ bool is_filled(const NearestArgs& a, double f) { return f < DINF && f <= a.max_d2; }

__device__ __forceinline__ double sq(double x) { return x * x; }
__device__ __forceinline__ uint32_t umin(uint32_t x, uint32_t y) { return x < y ? x : y; }

// One wave per row.  Forwards f and lab hold the voxels to the nearest site at or in front of the voxel and its label; backwards they
// meet the same of the nearest site at or behind it.
template <typename T>
__global__ __launch_bounds__(256) void nearest_row_kernel(NearestArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * 4, rows = (uint64_t)a.n0 * (uint64_t)a.n1;
    const int64_t n2 = a.n2;
    const double w = a.w[2];
    for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += nwaves) {
        const uint64_t at = row * (uint64_t)n2;
        int64_t pos = -1;                                  // the last site of the chunks done so far, -1 = none
        uint32_t plab = NEAR_NONE;
        for (int64_t b = 0; b < n2; b += 64) {
            const int64_t i = b + lane;
            const bool valid = i < n2;
            const uint32_t c = valid ? voxel_label<T>(a, at + (uint64_t)i) : 0u;
            const uint64_t m = __ballot(valid && is_site(a, c));
            const uint64_t mine = m & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
            const int src = mine ? 63 - __builtin_clzll(mine) : 0;
            const uint32_t from = (uint32_t)__shfl((int)c, src);
            if (valid) {
                a.f[at + (uint64_t)i] = mine ? (double)(lane - src) : (pos >= 0 ? (double)(i - pos) : DINF);
                a.lab[at + (uint64_t)i] = mine ? from : plab;
            }
            if (m) {
                const int top = 63 - __builtin_clzll(m);
                pos = b + top;
                plab = (uint32_t)__shfl((int)c, top);
            }
        }
        pos = -1;
        plab = NEAR_NONE;
        for (int64_t b = ((n2 - 1) / 64) * 64; b >= 0; b -= 64) {
            const int64_t i = b + lane;
            const bool valid = i < n2;
            const uint32_t c = valid ? voxel_label<T>(a, at + (uint64_t)i) : 0u;
            const uint64_t m = __ballot(valid && is_site(a, c));
            const uint64_t mine = m & (~0ull << lane);
            const int src = mine ? __builtin_ctzll(mine) : 0;
            const uint32_t from = (uint32_t)__shfl((int)c, src);
            if (valid) {
                const double dl = a.f[at + (uint64_t)i];
                const uint32_t ll = a.lab[at + (uint64_t)i];
                const double dr = mine ? (double)(src - lane) : (pos >= 0 ? (double)(pos - i) : DINF);
                const uint32_t rl = mine ? from : plab;
                a.f[at + (uint64_t)i] = sq(w * fmin(dl, dr));
                a.lab[at + (uint64_t)i] = dl < dr ? ll : (dr < dl ? rl : umin(ll, rl));
            }
            if (m) {
                const int low = __builtin_ctzll(m);
                pos = b + low;
                plab = (uint32_t)__shfl((int)c, low);
            }
        }
    }
}

// One lane per column.  Entry k of a column's stack: position sv, f at that position sf, left boundary sz (-inf for entry 0), label
// sl, boundary label sb; the top entry is kept in registers too.  Voxels with f = +inf have no parabola, so the intersection formula
// never meets inf - inf; a column of len voxels needs at most len entries.
__global__ __launch_bounds__(256) void nearest_column_kernel(NearestArgs a, int64_t len, uint64_t step, uint64_t inner, uint64_t outer_stride,
                                                             double w, uint64_t first, uint64_t columns, double* sf, double* sz, int32_t* sv,
                                                             uint32_t* sl, uint32_t* sb, uint64_t stride) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= columns) return;
    const uint64_t col = first + t;
    const uint64_t base = (col / inner) * outer_stride + (col % inner);
    const double w2 = w * w;
    int64_t k = -1;
    int32_t tv = 0;
    double tf = DINF, tz = -DINF;
    uint32_t tl = NEAR_NONE, tb = NEAR_NONE;
    for (int64_t i = 0; i < len; ++i) {
        const uint64_t idx = base + (uint64_t)i * step;
        const double f = a.f[idx];
        if (!(f < DINF)) continue;
        const uint32_t l = a.lab[idx];
        uint32_t carried = NEAR_NONE;                      // the smallest label of the parabolas popped at exactly `carried_at`
        double carried_at = 0.0, s = -DINF;
        while (k >= 0) {
            s = ((f + w2 * sq((double)i)) - (tf + w2 * sq((double)tv))) / (2.0 * w2 * (double)(i - tv));
            if (s > tz) break;
            if (s == tz) { carried = umin(tl, tb); carried_at = s; }
            else carried = NEAR_NONE;
            --k;                                           // (entry 0 is never popped: its boundary is -inf)
            const uint64_t e = (uint64_t)k * stride + t;
            tv = sv[e]; tf = sf[e]; tz = sz[e]; tl = sl[e]; tb = sb[e];
        }
        ++k;
        tv = (int32_t)i; tf = f; tz = s; tl = l;
        tb = (carried != NEAR_NONE && carried_at == s) ? carried : NEAR_NONE;
        const uint64_t e = (uint64_t)k * stride + t;
        sv[e] = tv; sf[e] = tf; sz[e] = tz; sl[e] = tl; sb[e] = tb;
    }
    if (k < 0) return;                                     // no site along the axes done so far: +inf and NEAR_NONE stay
    for (int64_t i = len - 1; i >= 0; --i) {
        const uint64_t idx = base + (uint64_t)i * step;
        while (tz > (double)i) {
            --k;
            const uint64_t e = (uint64_t)k * stride + t;
            tv = sv[e]; tf = sf[e]; tz = sz[e]; tl = sl[e]; tb = sb[e];
        }
        uint32_t l = tl;
        if (tz == (double)i) l = umin(umin(tl, tb), sl[(uint64_t)(k - 1) * stride + t]);
        a.f[idx] = tf + sq(w * (double)(i - tv));
        a.lab[idx] = l;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void nearest_count_kernel(NearestArgs a, NearestTable t, uint64_t nvox) {
    const int lane = threadIdx.x & 63;
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    unsigned long long filled = 0ull, left = 0ull;         // of the wave
    // every lane of a wave makes the same trips: the ballots below take all of them
    for (uint64_t at = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); at < nvox; at += nthreads) {
        const uint64_t v = at + (uint64_t)lane;
        const bool valid = v < nvox;
        const uint32_t c = valid ? voxel_label<T>(a, v) : 0u;
        bool empty = valid && is_empty(a, c);
        uint32_t n = 0u;
        bool fill = false;
        if (empty) {
            fill = is_filled(a, a.f[v]);
            n = a.lab[v];
        }
        if (c > t.max_label || (fill && n > t.max_label)) {
            atomicOr(&t.flags[NEAR_FLAG_RANGE], 1u);
            empty = fill = false;
        }
        uint64_t pending = __ballot(fill);
        filled += (unsigned long long)__popcll(pending);
        left += (unsigned long long)__popcll(__ballot(empty && !fill));
        while (pending) {                                  // one add per label the wave's filled voxels take
            const int src = __builtin_ctzll(pending);
            const uint32_t label = (uint32_t)__shfl((int)n, src);
            const uint64_t same = __ballot(fill && n == label);
            if (lane == src) flush_add(t.gained + label, (unsigned long long)__popcll(same));
            pending &= ~same;
        }
    }
    if (lane == 0) {
        if (filled) flush_add(t.totals + 0, filled);
        if (left) flush_add(t.totals + 1, left);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void nearest_apply_kernel(NearestArgs a, uint64_t nvox, T* vol, T* ranks, const uint32_t* ids, uint32_t nids) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvox; v += nthreads) {
        if (!is_empty(a, voxel_label<T>(a, v)) || !is_filled(a, a.f[v])) continue;
        const uint32_t n = a.lab[v];
        if (!ranks) vol[v] = (T)n;
        else if (n < nids) { ranks[v] = (T)n; vol[v] = (T)ids[n]; }
    }
}

uint64_t voxels_of(const NearestArgs& a) { return (uint64_t)a.n0 * (uint64_t)a.n1 * (uint64_t)a.n2; }

}  // namespace

uint32_t launch_nearest_rows(hipStream_t s, const NearestArgs& a, int itemsize) {
    const uint64_t rows = (uint64_t)a.n0 * (uint64_t)a.n1;
    const uint32_t grid = blocks_for(rows * 64, NEAR_ROW_MAX_GROUPS);
    if (itemsize == 2) hipLaunchKernelGGL(nearest_row_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(nearest_row_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, a);
    return grid;
}

void launch_nearest_columns(hipStream_t s, const NearestArgs& a, int axis, uint64_t first, uint64_t columns, void* work, uint64_t stride) {
    const ColumnPass g = column_pass(a.n0, a.n1, a.n2, axis);
    static_assert(NEAR_STACK_ENTRY == 2 * sizeof(double) + sizeof(int32_t) + 2 * sizeof(uint32_t), "the five arrays below are what the host reserves");
    const uint64_t entries = (uint64_t)g.len * stride;
    double* sf = (double*)work;
    double* sz = sf + entries;
    int32_t* sv = (int32_t*)(sz + entries);
    uint32_t* sl = (uint32_t*)(sv + entries);
    uint32_t* sb = sl + entries;
    hipLaunchKernelGGL(nearest_column_kernel, dim3(column_grid(columns)), dim3(256), 0, s, a, g.len, g.step, g.inner, g.outer_stride, a.w[axis],
                       first, columns, sf, sz, sv, sl, sb, stride);
}

uint32_t nearest_voxel_groups(const NearestArgs& a) { return blocks_for(voxels_of(a), NEAR_VOXEL_MAX_GROUPS); }

uint32_t launch_nearest_count(hipStream_t s, const NearestArgs& a, int itemsize, const NearestTable& t) {
    const uint32_t grid = nearest_voxel_groups(a);
    if (itemsize == 2) hipLaunchKernelGGL(nearest_count_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, a, t, voxels_of(a));
    else hipLaunchKernelGGL(nearest_count_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, a, t, voxels_of(a));
    return grid;
}

uint32_t launch_nearest_apply(hipStream_t s, const NearestArgs& a, int itemsize, void* vol, void* ranks, const uint32_t* ids, uint32_t nids) {
    const uint32_t grid = nearest_voxel_groups(a);
    if (itemsize == 2)
        hipLaunchKernelGGL(nearest_apply_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, a, voxels_of(a), (uint16_t*)vol, (uint16_t*)ranks, ids, nids);
    else
        hipLaunchKernelGGL(nearest_apply_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, a, voxels_of(a), (uint32_t*)vol, (uint32_t*)ranks, ids, nids);
    return grid;
}

}  // namespace ta
