/* tissue_scan_wallgeo.h -- per-wall geometry of the resident label volume: signed face counts and the first and second sums of
 * the face centres of every wall (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its
 * conventions).
 *
 * What it is for: the wall level of the tissue's cell complex.  From fifteen exact integers a wall the host derives a wall
 * area that a tilted wall's voxel staircase does not inflate, a wall normal, a wall centroid and a plane fit with its flatness.
 * The reference's users fit the wall-voxel point cloud in Python; there is no function to mirror here, and the semantics below
 * are this library's own.
 *
 * Definitions.  V is the label volume the last ta_extract swept (the rank copy in a compacted context), dims (n0, n1, n2) in
 * array-axis order; rows speak the language of ta_adjacency_get, exactly as ta_signal_get_walls does.
 *  - Face.  A pair of voxels p and q = p + e_d, both inside the volume, with V[p] != V[q]: exactly the faces TA_F_ADJACENCY
 *    counts.  Its pair is lo = min, hi = max of the two labels, its row that pair's row in the sorted list of ta_adjacency_get
 *    (which must be LOCAL, as for TA_SIG_WALLS).  No label is special: background pairs are included.
 *  - Position.  c = p + q in doubled voxel-centre coordinates: an odd integer along d, even along the other two axes; in
 *    array-axis order and global (axis 0 carries the slab's a0_origin).  This is the frame of the junction tables, and c / 2 is
 *    the frame of the barycentres in voxel units.
 *  - Per pair row, all uint64, all exact:
 *      fwd[3]    faces of axis d with V[p] == lo: lo on the low-coordinate side, +e_d points from lo to hi
 *      rev[3]    faces of axis d with V[p] == hi
 *      sum1[3]   sum of c over all faces of the pair (every face once, whatever its axis)
 *      sum2[6]   sum of c_x c_y for xx, xy, xz, yy, yz, zz
 *  - fwd + rev equals the `faces` column of ta_adjacency_get, row by row.
 *  - Slabs.  In a slab adopted with has_low_halo a face belongs to the slab of its higher voxel, as for the adjacency and the
 *    signal walls: the halo plane contributes only its faces with plane 1.  Summed over slabs every field equals the whole
 *    volume's.
 *  - Range.  ta_wallgeo_extract answers TA_ERANGE before the pass when 3 nvox (2 E)^2 >= 2^64, E the largest global extent
 *    (a0_origin + owned planes, n1, n2): no sum can wrap, and 2048^3 is far inside.  Never a silently wrapped sum.
 *  - A face whose pair the list does not hold cannot happen; if the pass flags one (the volume changed behind the library's
 *    back) the getters fail with TA_ERANGE.  Never short sums.  The one exception: an extraction without any pair has no row
 *    to add to and launches no pass, so its getters answer TA_OK with no rows whatever the volume holds by then.
 */
#ifndef TISSUE_SCAN_WALLGEO_H
#define TISSUE_SCAN_WALLGEO_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One pass over the labels, asynchronous on the context's stream.  Needs a finished ta_extract of the current volume with
 * TA_F_ADJACENCY and a LOCAL pair list, else TA_EINVAL.  A new volume, ta_volume_relabel or ta_volume_rerank, compaction or its
 * end, or a new ta_extract invalidates the rows: the getters then answer TA_EINVAL. */
TA_API int ta_wallgeo_extract(ta_ctx* ctx);
/* The rows, one per pair of ta_adjacency_get (ta_adjacency_size of them): fwd [P][3], rev [P][3], sum1 [P][3], sum2 [P][6]; any
 * pointer may be NULL.  Synchronises. */
TA_API int ta_wallgeo_get(ta_ctx* ctx, uint64_t* fwd, uint64_t* rev, uint64_t* sum1, uint64_t* sum2);
/* Diagnostics of the last pass: records that found no slot in a workgroup's LDS table and went to the global rows directly
 * (the results are the same).  Synchronises. */
TA_API int ta_wallgeo_spills(ta_ctx* ctx, uint32_t* spills);
/* The same and the launch plan, for tests: out[0] the spills, out[1] 0, out[2] the tiles a workgroup took, out[3] the
 * workgroups (0 and 0 when the extraction has no pair: the pass is then not launched at all).  Synchronises. */
TA_API int ta_wallgeo_debug(ta_ctx* ctx, uint32_t out[4]);
/* Milliseconds between two HIP events around the pass kernel of the last ta_wallgeo_extract (the pair table is built before). */
TA_API int ta_wallgeo_timing(ta_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_WALLGEO_H */
