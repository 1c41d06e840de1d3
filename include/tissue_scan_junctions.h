/* tissue_scan_junctions.h -- cell junctions of the resident label volume: the lines where three cells meet and the points where
 * four cells meet (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its conventions).
 *
 * What it is for: the two lowest levels of the tissue's cell complex, as landmarks for junction lengths and for growth and strain
 * between two frames that share a lineage.  The reference takes its topology from a library outside its tree: there is no
 * function to mirror here, and the semantics below are this library's own.
 *
 * Definitions.  V is the label volume of the context (uint16 or uint32), dims (n0, n1, n2) in array-axis order.
 *  - Block.  A block at origin o = (i, j, k) is the set of voxels o + d with d_x in {0, 1} for the axes with n_x >= 2 and d_x = 0
 *    for the axes with n_x = 1; o_x ranges over 0 .. n_x - 2 (over 0 alone when n_x = 1).  Only blocks wholly inside the volume
 *    exist: a 2-D image (n, m, 1) has 2 x 2 blocks.
 *  - Order.  The order of a block is the number of distinct labels among its voxels.
 *  - No label is special: 0 and the background count like any cell, and any 32-bit value is a label.  The caller filters.
 *  - Position.  The position of a block is its centre in doubled voxel-centre coordinates, c_x = 2 o_x + 1 (0 when n_x = 1):
 *    exact integers, and c / 2 is the centre in voxel units, the frame of the barycentres in voxel units.
 *  - Edge table (order 3).  Rows (a < b < c, n, s0, s1, s2): n is the number of blocks of order 3 whose label set is {a, b, c},
 *    s_x the sum of their c_x (uint64).  Sorted ascending by (a, b, c), each triple once, n > 0.
 *  - Vertex table (order 4).  The same with (a < b < c < d).
 *  - Degenerate blocks (order >= 5) are counted in one uint64 and enter no row.
 *  - All outputs are exact integers, bit-identical whatever the order of the device's operations.  The labels of the rows are
 *    the ids as stored, never ranks: a compacted context answers in ids too (the pass reads the ids, not the rank copy).
 *  - Slabs.  In a slab adopted with has_low_halo a block belongs to the slab that owns its UPPER plane along axis 0: the halo
 *    plane only ever serves as a lower plane, and positions use the global a0_origin.  The tables of the slabs of a volume, merged
 *    by summing n and s over equal keys (and summing the degenerate counts), equal the whole volume's tables.
 *  - The pass needs a volume, not a finished ta_extract.
 *  - The number of junction blocks is not known beforehand: the pass counts them, the records and the tables are then allocated
 *    at exactly that size (count, scan, emit).  Never a silently short table; TA_ENOMEM comes before anything is written to
 *    caller memory.
 */
#ifndef TISSUE_SCAN_JUNCTIONS_H
#define TISSUE_SCAN_JUNCTIONS_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The counting walk over the 2 x 2 x 2 blocks of the label volume, asynchronous on the context's stream.  Needs a label volume
 * (else TA_EINVAL), no ta_extract.  A new label volume, ta_volume_relabel or ta_volume_rerank (the caller edited the labels in
 * place) invalidates the tables: the functions below then answer TA_EINVAL. */
TA_API int ta_junctions_extract(ta_ctx* ctx);
/* Rows of the edge table, rows of the vertex table, blocks of order >= 5; any pointer may be NULL.  Synchronises and settles:
 * the emitting walk, the sort of the records and their reduction into the tables.  TA_ENOMEM when the records or the tables
 * cannot be allocated. */
TA_API int ta_junctions_size(ta_ctx* ctx, uint64_t* nedges, uint64_t* nvertices, uint64_t* degenerate);
/* The edge table: labels [nedges][3] ascending in a row, n [nedges], sums [nedges][3] in array-axis order; any pointer may be
 * NULL.  Synchronises (and settles, as above, before anything is written to caller memory). */
TA_API int ta_junctions_get_edges(ta_ctx* ctx, uint32_t* labels, uint64_t* n, uint64_t* sums);
/* The vertex table: labels [nvertices][4], n [nvertices], sums [nvertices][3]. */
TA_API int ta_junctions_get_vertices(ta_ctx* ctx, uint32_t* labels, uint64_t* n, uint64_t* sums);
/* Diagnostics for tests: what the last pass launched.  out[0] the tasks of a walk (one wave each), out[1] and out[2] the
 * workgroups of the kernel that writes the sort keys of the edge and of the vertex records (0 without records; fewer than
 * records / 256 means that it strode over them), out[3] 0.  Synchronises and settles; TA_EINVAL as the getters above. */
TA_API int ta_junctions_debug(ta_ctx* ctx, uint32_t out[4]);
/* Milliseconds between HIP events.  ms_pass: the two walks over the volume (counting and emitting).  ms_after: everything else
 * on the device, from the scans of the counts to the finished tables (it spans the host's read of the row counts).  Settled
 * tables only (ask ta_junctions_size first), else TA_EINVAL; either pointer may be NULL. */
TA_API int ta_junctions_timing(ta_ctx* ctx, double* ms_pass, double* ms_after);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_JUNCTIONS_H */
