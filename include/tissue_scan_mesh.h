/* tissue_scan_mesh.h -- the exact triangle surface mesh of every requested cell of the resident label volume
 * (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its conventions).
 *
 * The reference meshes cells through VTK (marching cubes + smoothing) on an image subsampled by 4 or 6.  This is the exact
 * voxel-face surface instead, with no smoothing; subsampling is strided, as `image[::s, ::s, ::s]`.
 *
 * Definitions.  V is the label volume of the context, in array axes 0, 1, 2 with dims n; s >= 1 the sub_factor.  The meshed image
 * is W = V[::s, ::s, ::s], of dims m = ceil(n / s).  Rows are those of the last ta_extract (0 .. max_label, or ranks in a
 * compacted context): every label below is a ROW, and the host maps rows to ids.
 *  cells      the requested rows that have a voxel in W, ascending.
 *  faces      for a voxel p with W[p] = c, c requested, and a direction +-e_a: when q = p +- e_a is outside W or W[q] != c, the face
 *             between them is a boundary face of c; its neighbour is W[q], or TA_MESH_OUTSIDE at the stack border.
 *  corners    K in 0 .. m on each axis; reported as the C-order index of K on the corner grid of dims m + 1 (array axes).
 *             Voxel p spans the corners p .. p + 1, so corner K sits at (K - 1/2) * voxelsize * s.
 *  triangles  two per face, oriented so that the normal (right-hand rule) points from p to q.  With b = (a + 1) % 3,
 *             d = (a + 2) % 3 and K0 the face's corner of smallest coordinates: v0 = K0, v1 = K0 + e_b, v2 = K0 + e_b + e_d,
 *             v3 = K0 + e_d; +e_a: (v0, v1, v2), (v0, v2, v3); -e_a: (v0, v2, v1), (v0, v3, v2).  Triangles 2k, 2k + 1 of a cell
 *             are one face.
 *  vertices   per cell, the distinct corners of its faces (a corner shared by two cells is a vertex of each).
 *  order      cells ascending; within a cell, vertices by ascending corner index, faces by ascending C-order index of p and, for
 *             one voxel, in the order -0, +0, -1, +1, -2, +2.  For a volume stored in another axis permutation the vertex
 *             order still holds, and the faces come in memory order: only their set is specified.
 * Counts are uint64; more than 2^32 - 1 vertices, or as many faces, is TA_ERANGE before anything is emitted.
 */
#ifndef TISSUE_SCAN_MESH_H
#define TISSUE_SCAN_MESH_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the neighbour of a face on the stack border */
#define TA_MESH_OUTSIDE 0xFFFFFFFFu

/* Count, size exactly, then emit the meshes of the rows with wanted_rows[row] != 0 (one byte per row of the last extraction;
 * NULL = every row present, background included).  Needs a finished ta_extract of the current volume, else TA_EINVAL;
 * TA_EINVAL on a slab adopted with a halo.  One read-back of the totals synchronises, the rest is enqueued on the context's
 * stream.  TA_ENOMEM when the output does not fit: no result is then held.  A new volume, ta_volume_relabel, compaction or its
 * end, or a new ta_extract invalidates the results: the getters then answer TA_EINVAL. */
TA_API int ta_mesh_extract(ta_ctx* ctx, int sub_factor, const uint8_t* wanted_rows);
/* Cells, vertices and triangles of the last ta_mesh_extract; any pointer may be NULL.  Synchronises. */
TA_API int ta_mesh_size(ta_ctx* ctx, uint64_t* n_cells, uint64_t* n_vertices, uint64_t* n_triangles);
/* The mesh; any pointer may be NULL.  cells u32[C] (rows); vertex_offsets, triangle_offsets u64[C + 1] (CSR over the cells);
 * corners u64[V] (corner indices, see above); triangles u32[T][3] (global vertex indices); triangle_cell u32[T] (rows);
 * triangle_neighbor u32[T] (rows, TA_MESH_OUTSIDE at the border).  Synchronises. */
TA_API int ta_mesh_get(ta_ctx* ctx, uint32_t* cells, uint64_t* vertex_offsets, uint64_t* triangle_offsets, uint64_t* corners,
                       uint32_t* triangles, uint32_t* triangle_cell, uint32_t* triangle_neighbor);
/* Milliseconds of device time of the last ta_mesh_extract: the count kernels and the emit / sort / resolve kernels, each span
 * between two HIP events (the read-back between them is not counted). */
TA_API int ta_mesh_timing(ta_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_MESH_H */
