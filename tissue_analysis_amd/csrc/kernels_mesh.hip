// kernels_mesh.hip -- the exact surface mesh of every requested cell (include/tissue_scan_mesh.h): the voxel faces where the label
// changes, two triangles each, with a vertex set of its own per cell.
//
// Layout.  W = vol[::s, ::s, ::s] is read strided, never copied.  Two streams of records, each built as count -> scan -> emit:
//   faces    a wave walks 1024 consecutive voxels of W (memory order) 64 at a time; a lane looks at its voxel's six neighbours
//            and writes one record per boundary face of a requested cell -- voxel << 3 | direction, the neighbour's row, and the
//            cell's row as the sort key -- at the wave's offset (an exclusive scan of the per-wave counts) plus its rank among
//            the wave's faces (a wave scan): voxel order, then direction order, with no atomics at all;
//   corners  the same over the corner grid (m + 1 on each axis): a lane reads the eight voxels around its corner and writes
//            one (row, corner) record per requested cell that holds some but not all of them.
// Both streams are then grouped by cell with the stable radix sort of kernels_wallsort.hip (keys of label-bits width), so
// within a cell the records keep voxel / corner order.  The vertices of a cell are its corner records in that order; a face
// finds each of its four corners by binary search in its cell's vertex segment and writes its two triangles.
// The background -- whose faces are a large share of all faces -- costs no more than any cell: nothing here adds to a shared word.
#include "ta_mesh.h"
#include "ta_kernels.h"

namespace ta {
namespace {

constexpr int MESH_THREADS = 256;                     // four waves a workgroup

template <typename T>
__device__ __forceinline__ uint32_t mesh_at(const MeshArgs& a, int64_t i0, int64_t i1, int64_t i2) {
    return (uint32_t)((const T*)a.vol)[((i0 * a.s) * a.n1 + i1 * a.s) * a.n2 + i2 * a.s];
}

// a label read from W, or MESH_OUTSIDE beyond its border
template <typename T>
__device__ __forceinline__ uint32_t mesh_at_or_outside(const MeshArgs& a, int64_t i0, int64_t i1, int64_t i2) {
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= a.m0 || i1 >= a.m1 || i2 >= a.m2) return MESH_OUTSIDE;
    return mesh_at<T>(a, i0, i1, i2);
}

__device__ __forceinline__ bool mesh_wanted(const MeshArgs& a, uint32_t row) {
    if (row == MESH_OUTSIDE) return false;
    if (row >= a.rows) { a.flags[MESH_FLAG_RANGE] = 1u; return false; }
    return a.wanted[row] != 0;
}

// coordinates of item w of a grid of dims (d0, d1, d2), memory order
struct Coord { int64_t c0, c1, c2; };
__device__ __forceinline__ Coord mesh_coord(uint64_t w, int64_t d1, int64_t d2) {
    Coord c;
    const uint64_t row = w / (uint64_t)d2;
    c.c2 = (int64_t)(w - row * (uint64_t)d2);
    c.c0 = (int64_t)(row / (uint64_t)d1);
    c.c1 = (int64_t)(row - (uint64_t)c.c0 * (uint64_t)d1);
    return c;
}
// ... moved on by 64 items (a division only where a row wraps)
__device__ __forceinline__ void mesh_advance(Coord& c, int64_t d1, int64_t d2) {
    c.c2 += 64;
    if (c.c2 >= d2) {
        const int64_t q = c.c2 / d2;
        c.c2 -= q * d2;
        c.c1 += q;
        if (c.c1 >= d1) { const int64_t q1 = c.c1 / d1; c.c1 -= q1 * d1; c.c0 += q1; }
    }
}

__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// The boundary faces of voxel c of W: bit `dir` set for each of the six directions (dir = 2 a + (1 for +e_a), a an ARRAY axis)
// whose neighbour differs; nbr[dir] that neighbour.  0 for a voxel outside W or of a cell not requested.
template <typename T>
__device__ __forceinline__ uint32_t voxel_faces(const MeshArgs& a, const Coord& c, bool inside, uint32_t& row, uint32_t nbr[6]) {
    row = MESH_OUTSIDE;
    if (!inside) return 0u;
    row = mesh_at<T>(a, c.c0, c.c1, c.c2);
    if (!mesh_wanted(a, row)) return 0u;
    uint32_t bits = 0u;
#pragma unroll
    for (int dir = 0; dir < 6; ++dir) {
        const int k = a.inv[dir >> 1];
        const int64_t step = (dir & 1) ? 1 : -1;
        const uint32_t q = mesh_at_or_outside<T>(a, c.c0 + (k == 0 ? step : 0), c.c1 + (k == 1 ? step : 0), c.c2 + (k == 2 ? step : 0));
        nbr[dir] = q;
        if (q != row) bits |= 1u << dir;
    }
    return bits;
}

template <typename T, bool EMIT>
__global__ void __launch_bounds__(MESH_THREADS) mesh_face_kernel(const MeshArgs a, uint32_t* counts, const uint64_t* offsets, uint64_t cap,
                                                                 uint64_t* rec, uint32_t* nb, uint32_t* key, uint32_t* idx) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (MESH_THREADS / 64) + (threadIdx.x >> 6);
    const uint64_t total = (uint64_t)a.m0 * a.m1 * a.m2;
    const uint64_t base = wave * MESH_PER_WAVE;
    if (base >= total) return;
    Coord c = mesh_coord(base + lane, a.m1, a.m2);
    uint64_t at = EMIT ? offsets[wave] : 0;
    uint32_t sum = 0u;
    for (int k = 0; k < MESH_PER_WAVE / 64; ++k) {
        const uint64_t w = base + (uint64_t)k * 64 + lane;
        uint32_t row, nbr[6];
        const uint32_t bits = voxel_faces<T>(a, c, w < total, row, nbr);
        const uint32_t n = (uint32_t)__builtin_popcount(bits);
        if (EMIT) {
            const uint32_t incl = wave_inclusive(n, lane);
            uint64_t pos = at + incl - n;
#pragma unroll
            for (int dir = 0; dir < 6; ++dir) {
                if (!((bits >> dir) & 1u)) continue;
                if (pos < cap) {
                    rec[pos] = (w << 3) | (uint64_t)dir;
                    nb[pos] = nbr[dir];
                    key[pos] = row;
                    idx[pos] = (uint32_t)pos;
                } else {
                    a.flags[MESH_FLAG_OVERRUN] = 1u;
                }
                ++pos;
            }
            at += (uint32_t)__shfl((int)incl, 63, 64);
        } else {
            sum += n;
        }
        mesh_advance(c, a.m1, a.m2);
    }
    if (!EMIT) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += (uint32_t)__shfl_down((int)sum, o, 64);
        if (lane == 0) counts[wave] = sum;
    }
}

// The requested cells partially present around corner c (memory coordinates on the corner grid): bit d set when lab[d], the
// label of the d-th of the eight voxels around it, is such a cell and not one of lab[0 .. d) (first-occurrence order).
template <typename T>
__device__ __forceinline__ uint32_t corner_cells(const MeshArgs& a, const Coord& c, bool inside, uint32_t lab[8]) {
    if (!inside) return 0u;
#pragma unroll
    for (int d = 0; d < 8; ++d)
        lab[d] = mesh_at_or_outside<T>(a, c.c0 - 1 + ((d >> 2) & 1), c.c1 - 1 + ((d >> 1) & 1), c.c2 - 1 + (d & 1));
    bool uniform = true;
#pragma unroll
    for (int d = 1; d < 8; ++d) uniform = uniform && lab[d] == lab[0];
    if (uniform) return 0u;
    uint32_t bits = 0u;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        bool first = true;
#pragma unroll
        for (int e = 0; e < d; ++e) first = first && lab[e] != lab[d];
        if (first && mesh_wanted(a, lab[d])) bits |= 1u << d;
    }
    return bits;
}

template <typename T, bool EMIT>
__global__ void __launch_bounds__(MESH_THREADS) mesh_corner_kernel(const MeshArgs a, uint32_t* counts, const uint64_t* offsets, uint64_t cap,
                                                                   uint64_t* corner, uint32_t* key, uint32_t* idx) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (MESH_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t g1 = a.m1 + 1, g2 = a.m2 + 1;
    const uint64_t total = (uint64_t)(a.m0 + 1) * g1 * g2;
    const uint64_t base = wave * MESH_PER_WAVE;
    if (base >= total) return;
    Coord c = mesh_coord(base + lane, g1, g2);
    uint64_t at = EMIT ? offsets[wave] : 0;
    uint32_t sum = 0u;
    for (int k = 0; k < MESH_PER_WAVE / 64; ++k) {
        const uint64_t w = base + (uint64_t)k * 64 + lane;
        uint32_t lab[8];
        const uint32_t bits = corner_cells<T>(a, c, w < total, lab);
        const uint32_t n = (uint32_t)__builtin_popcount(bits);
        if (EMIT) {
            const uint32_t incl = wave_inclusive(n, lane);
            uint64_t pos = at + incl - n;
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                if (!((bits >> d) & 1u)) continue;
                if (pos < cap) {
                    corner[pos] = w;
                    key[pos] = lab[d];
                    idx[pos] = (uint32_t)pos;
                } else {
                    a.flags[MESH_FLAG_OVERRUN] = 1u;
                }
                ++pos;
            }
            at += (uint32_t)__shfl((int)incl, 63, 64);
        } else {
            sum += n;
        }
        mesh_advance(c, g1, g2);
    }
    if (!EMIT) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += (uint32_t)__shfl_down((int)sum, o, 64);
        if (lane == 0) counts[wave] = sum;
    }
}

__global__ void __launch_bounds__(256) mesh_bounds_kernel(const uint32_t* keys, uint64_t n, uint64_t* beg, uint64_t* end) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t k = keys[i];
        if (i == 0 || keys[i - 1] != k) beg[k] = i;
        if (i + 1 == n || keys[i + 1] != k) end[k] = i + 1;
    }
}

__global__ void __launch_bounds__(256) mesh_gather_kernel(const uint64_t* in, const uint32_t* perm, uint64_t n, uint64_t* out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = in[perm[i]];
}

// index of corner k in the ascending vcorner[lo .. hi), or MESH_OUTSIDE when it is not there
__device__ __forceinline__ uint32_t find_vertex(const uint64_t* vcorner, uint64_t lo, const uint64_t end, uint64_t k) {
    uint64_t hi = end;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (vcorner[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo < end && vcorner[lo] == k ? (uint32_t)lo : MESH_OUTSIDE;
}

__global__ void __launch_bounds__(256) mesh_resolve_kernel(const MeshArgs a, const uint32_t* fkey, const uint32_t* fperm, const uint64_t* rec,
                                                           const uint32_t* nb, uint64_t nfaces, const uint64_t* vcorner, const uint64_t* vbeg,
                                                           const uint64_t* vend, uint32_t* tri, uint32_t* tri_cell, uint32_t* tri_nb) {
    const uint64_t g1 = (uint64_t)a.m1 + 1, g2 = (uint64_t)a.m2 + 1;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nfaces; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t cell = fkey[j];
        const uint32_t r = fperm[j];
        const uint64_t vd = rec[r];
        const uint32_t q = nb[r];
        const int dir = (int)(vd & 7u), ax = dir >> 1;
        const Coord p = mesh_coord(vd >> 3, a.m1, a.m2);
        // the face's corner of smallest coordinates, and the memory axes of the array axes b = a + 1, d = a + 2 (mod 3)
        int64_t k[3] = {p.c0, p.c1, p.c2};
        k[a.inv[ax]] += dir & 1;
        const int kb = a.inv[(ax + 1) % 3], kd = a.inv[(ax + 2) % 3];
        const uint64_t v0 = ((uint64_t)k[0] * g1 + (uint64_t)k[1]) * g2 + (uint64_t)k[2];
        const uint64_t sb = kb == 0 ? g1 * g2 : (kb == 1 ? g2 : 1), sd = kd == 0 ? g1 * g2 : (kd == 1 ? g2 : 1);
        const uint64_t lo = vbeg[cell], hi = vend[cell];
        const uint32_t i0 = find_vertex(vcorner, lo, hi, v0), i1 = find_vertex(vcorner, lo, hi, v0 + sb);
        const uint32_t i2 = find_vertex(vcorner, lo, hi, v0 + sb + sd), i3 = find_vertex(vcorner, lo, hi, v0 + sd);
        if (i0 == MESH_OUTSIDE || i1 == MESH_OUTSIDE || i2 == MESH_OUTSIDE || i3 == MESH_OUTSIDE)
            a.flags[MESH_FLAG_MISS] = 1u;
        uint32_t* t = tri + 6 * j;
        if (dir & 1) { t[0] = i0; t[1] = i1; t[2] = i2; t[3] = i0; t[4] = i2; t[5] = i3; }
        else         { t[0] = i0; t[1] = i2; t[2] = i1; t[3] = i0; t[4] = i3; t[5] = i2; }
        tri_cell[2 * j] = cell; tri_cell[2 * j + 1] = cell;
        tri_nb[2 * j] = q; tri_nb[2 * j + 1] = q;
    }
}

unsigned grid_of_waves(uint64_t waves) { return (unsigned)((waves + MESH_THREADS / 64 - 1) / (MESH_THREADS / 64)); }
unsigned grid_stride(uint64_t n) { const uint64_t b = (n + 255) / 256; return (unsigned)(b < 16384 ? (b ? b : 1) : 16384); }

}  // namespace

void launch_mesh_face_count(hipStream_t s, const MeshArgs& a, int itemsize, uint32_t* counts) {
    const uint64_t waves = mesh_waves((uint64_t)a.m0 * a.m1 * a.m2);
    if (!waves) return;
    if (itemsize == 2) hipLaunchKernelGGL((mesh_face_kernel<uint16_t, false>), dim3(grid_of_waves(waves)), dim3(MESH_THREADS), 0, s, a, counts, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    else hipLaunchKernelGGL((mesh_face_kernel<uint32_t, false>), dim3(grid_of_waves(waves)), dim3(MESH_THREADS), 0, s, a, counts, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
}

void launch_mesh_face_emit(hipStream_t s, const MeshArgs& a, int itemsize, const uint64_t* offsets, uint64_t cap, uint64_t* rec,
                           uint32_t* nb, uint32_t* key, uint32_t* idx) {
    const uint64_t waves = mesh_waves((uint64_t)a.m0 * a.m1 * a.m2);
    if (!waves || !cap) return;
    if (itemsize == 2) hipLaunchKernelGGL((mesh_face_kernel<uint16_t, true>), dim3(grid_of_waves(waves)), dim3(MESH_THREADS), 0, s, a, nullptr, offsets, cap, rec, nb, key, idx);
    else hipLaunchKernelGGL((mesh_face_kernel<uint32_t, true>), dim3(grid_of_waves(waves)), dim3(MESH_THREADS), 0, s, a, nullptr, offsets, cap, rec, nb, key, idx);
}

void launch_mesh_corner_count(hipStream_t s, const MeshArgs& a, int itemsize, uint32_t* counts) {
    const uint64_t waves = mesh_waves((uint64_t)(a.m0 + 1) * (a.m1 + 1) * (a.m2 + 1));
    if (itemsize == 2) hipLaunchKernelGGL((mesh_corner_kernel<uint16_t, false>), dim3(grid_of_waves(waves)), dim3(MESH_THREADS), 0, s, a, counts, nullptr, 0, nullptr, nullptr, nullptr);
    else hipLaunchKernelGGL((mesh_corner_kernel<uint32_t, false>), dim3(grid_of_waves(waves)), dim3(MESH_THREADS), 0, s, a, counts, nullptr, 0, nullptr, nullptr, nullptr);
}

void launch_mesh_corner_emit(hipStream_t s, const MeshArgs& a, int itemsize, const uint64_t* offsets, uint64_t cap, uint64_t* corner,
                             uint32_t* key, uint32_t* idx) {
    const uint64_t waves = mesh_waves((uint64_t)(a.m0 + 1) * (a.m1 + 1) * (a.m2 + 1));
    if (!cap) return;
    if (itemsize == 2) hipLaunchKernelGGL((mesh_corner_kernel<uint16_t, true>), dim3(grid_of_waves(waves)), dim3(MESH_THREADS), 0, s, a, nullptr, offsets, cap, corner, key, idx);
    else hipLaunchKernelGGL((mesh_corner_kernel<uint32_t, true>), dim3(grid_of_waves(waves)), dim3(MESH_THREADS), 0, s, a, nullptr, offsets, cap, corner, key, idx);
}

void launch_mesh_bounds(hipStream_t s, const uint32_t* keys, uint64_t n, uint64_t* beg, uint64_t* end) {
    if (!n) return;
    hipLaunchKernelGGL(mesh_bounds_kernel, dim3(grid_stride(n)), dim3(256), 0, s, keys, n, beg, end);
}

void launch_mesh_gather(hipStream_t s, const uint64_t* in, const uint32_t* perm, uint64_t n, uint64_t* out) {
    if (!n) return;
    hipLaunchKernelGGL(mesh_gather_kernel, dim3(grid_stride(n)), dim3(256), 0, s, in, perm, n, out);
}

void launch_mesh_resolve(hipStream_t s, const MeshArgs& a, const uint32_t* fkey, const uint32_t* fperm, const uint64_t* rec,
                         const uint32_t* nb, uint64_t nfaces, const uint64_t* vcorner, const uint64_t* vbeg, const uint64_t* vend,
                         uint32_t* tri, uint32_t* tri_cell, uint32_t* tri_nb) {
    if (!nfaces) return;
    hipLaunchKernelGGL(mesh_resolve_kernel, dim3(grid_stride(nfaces)), dim3(256), 0, s, a, fkey, fperm, rec, nb, nfaces, vcorner, vbeg,
                       vend, tri, tri_cell, tri_nb);
}

}  // namespace ta
