// ta_mesh.h -- launchers of kernels_mesh.hip: the exact voxel-face surface mesh of every requested cell of the resident label
// volume (include/tissue_scan_mesh.h).
#pragma once
#include "ta_device.h"

namespace ta {

// flag words of the mesh pass (device u32[MESH_NFLAGS], zeroed before every pass)
enum { MESH_FLAG_RANGE = 0, MESH_FLAG_MISS = 1, MESH_FLAG_OVERRUN = 2, MESH_NFLAGS = 4 };
constexpr uint32_t MESH_OUTSIDE = 0xFFFFFFFFu;        // the neighbour across the stack border
constexpr int MESH_PER_WAVE = 1024;                   // voxels (corners) one wave of the count and emit kernels walks

struct MeshArgs {
    const void* vol;             // labels, dense C-ordered [n0][n1][n2] (u16 or u32; the rank copy of a compacted context)
    int64_t n0, n1, n2;          // buffer dims (memory order)
    int64_t s;                   // sub_factor: the meshed image is vol[::s, ::s, ::s]
    int64_t m0, m1, m2;          // its dims, ceil(n / s)
    int32_t inv[3];              // inv[a] = memory axis of array axis a
    const uint8_t* wanted;       // [rows] 1 = mesh this row
    uint32_t rows;               // max_label + 1 of the extraction
    uint32_t* flags;             // [MESH_NFLAGS]
};

// waves of the count / emit kernels over n items
inline uint64_t mesh_waves(uint64_t n) { return (n + MESH_PER_WAVE - 1) / MESH_PER_WAVE; }

// boundary faces of requested cells per wave (counts[mesh_waves(m0 m1 m2)])
void launch_mesh_face_count(hipStream_t s, const MeshArgs& a, int itemsize, uint32_t* counts);
// the face records in voxel order, then direction order (-0, +0, -1, +1, -2, +2 in array axes): rec = voxel << 3 | direction,
// nb = neighbour row (MESH_OUTSIDE at the border), key = cell row, idx = record index.  offsets: the exclusive scan of counts.
void launch_mesh_face_emit(hipStream_t s, const MeshArgs& a, int itemsize, const uint64_t* offsets, uint64_t cap, uint64_t* rec,
                           uint32_t* nb, uint32_t* key, uint32_t* idx);
// (cell, corner) records of the (m0+1)(m1+1)(m2+1) corner grid: a requested cell that holds some but not all of the eight voxels
// around the corner (the outside counts as a label of its own)
void launch_mesh_corner_count(hipStream_t s, const MeshArgs& a, int itemsize, uint32_t* counts);
void launch_mesh_corner_emit(hipStream_t s, const MeshArgs& a, int itemsize, const uint64_t* offsets, uint64_t cap, uint64_t* corner,
                             uint32_t* key, uint32_t* idx);
// beg[k] / end[k] of the run of key k in keys[0 .. n) (sorted); rows without a run are left alone
void launch_mesh_bounds(hipStream_t s, const uint32_t* keys, uint64_t n, uint64_t* beg, uint64_t* end);
// out[i] = in[perm[i]]
void launch_mesh_gather(hipStream_t s, const uint64_t* in, const uint32_t* perm, uint64_t n, uint64_t* out);
// two triangles per face (face j -> triangles 2j, 2j + 1), vertex indices found in the cell's vertex segment
// vcorner[vbeg[c] .. vend[c]) (ascending corner indices)
void launch_mesh_resolve(hipStream_t s, const MeshArgs& a, const uint32_t* fkey, const uint32_t* fperm, const uint64_t* rec,
                         const uint32_t* nb, uint64_t nfaces, const uint64_t* vcorner, const uint64_t* vbeg, const uint64_t* vend,
                         uint32_t* tri, uint32_t* tri_cell, uint32_t* tri_nb);

}  // namespace ta
