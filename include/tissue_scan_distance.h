/* tissue_scan_distance.h -- exact Euclidean distance maps of the resident label volume: for every voxel the squared distance to
 * the nearest voxel of another label (or of one chosen label), and per label the smallest and the largest of them and where the
 * largest sits (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its conventions).
 *
 * What it is for: "how far" is the one question the stencils and the keyed reductions of this library do not answer.  The largest
 * distance of a cell's voxels to its own wall is the radius of its largest inscribed sphere, and the voxel where it is reached (the
 * pole) is a centre that stays inside a curved or fragmented cell, where the barycentre does not.  The smallest distance of a cell's
 * voxels to the background is its depth below the tissue surface.  Users of the reference run scipy.ndimage.distance_transform_edt
 * themselves, once per label crop; here all labels are done at once, in three passes over the volume.
 *
 * Definitions.  V is the label volume of the context (uint16 or uint32, any dense layout), dims (n0, n1, n2) in array-axis order.
 * spacing[3] holds positive finite doubles in array-axis order.
 *  - D2(p) = min over the sites q of p of  sum_a (spacing[a] * (p_a - q_a))^2,  a float64; +inf when p has no site.  Distances run
 *    between voxel centres.
 *  - TA_DIST_OWN_WALL (mode 0).  The sites of p are the voxels whose label differs from V(p): D2(p) >= min spacing^2, and sqrt(D2)
 *    equals scipy's distance_transform_edt(V == V(p), sampling=spacing) at p.  No label is special.
 *  - TA_DIST_FROM_LABEL (mode 1, with site_label).  The sites are the voxels with V == site_label; those voxels themselves read 0.
 *    A site label that the volume does not hold gives +inf everywhere and no error.  In a compacted context site_label is an id.
 *  - TA_DIST_EDGE_IS_SITE (flag).  The layer of voxels just outside the image counts as sites of every voxel: the result equals the
 *    same transform of the image padded by one voxel of a label it does not hold (mode 1: of site_label).  Off by default, so a
 *    cell cut by the stack margin is not bounded by the margin.
 *  - Table.  One row per row of the last ta_extract (0 .. max_label, or the ranks of a compacted context: the convention of
 *    tissue_scan_signal.h):
 *      min2  f64      the minimum of D2 over the label's voxels
 *      max2  f64      the maximum of D2 over the label's voxels
 *      pole  i32[3]   the voxel where D2 == max2, in array axes; among several the first in C order of the ARRAY axes (as `first`
 *                     of the components), hence the same for every memory layout
 *    A label without voxels reads +inf, +inf, (-1, -1, -1).  There are no sums of distances: float sums depend on the order.
 *  - Exactness.  Where every spacing is a power of two (1 included) every product and sum of the passes is exact, and the image and
 *    the table are bit-identical to the definition for every memory layout -- as long as every squared distance, in units of the
 *    smallest spacing squared, stays below 2^53.  The boundary between two parabolas of the lower envelope is
 *        ((f(q) + w^2 q^2) - (f(v) + w^2 v^2)) / (2 w^2 (q - v))
 *    in float64: for such spacings numerator and denominator are exact and the division is correctly rounded, so ties and near-ties
 *    resolve as in exact arithmetic.  For other spacings the results agree with the definition to 1e-12 relative: the passes follow
 *    the MEMORY axes, so the order of the three additions differs between layouts, which costs a few ulp of 2^-53.
 *  - Slabs are out of scope (an exact transform needs halos of unbounded depth): a volume adopted with a halo plane or a non-zero
 *    origin answers TA_EINVAL.
 *  - Limits.  The buffer holds fewer than 2^63 bytes; coordinates are int32 (an axis holds at most 2^30 voxels, ta_volume_set).
 *  - Size.  One float64 per voxel stays on the context as the image until the results are invalidated, and a work buffer of at most
 *    1 GiB (or one batch of 64 columns, if that is more) holds the envelopes of a batch of columns.
 */
#ifndef TISSUE_SCAN_DISTANCE_H
#define TISSUE_SCAN_DISTANCE_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TA_DIST_OWN_WALL     0   /* mode: the sites of a voxel are the voxels of every other label */
#define TA_DIST_FROM_LABEL   1   /* mode: the sites are the voxels of site_label */
#define TA_DIST_EDGE_IS_SITE 1u  /* flag: the voxels just outside the image are sites too */

/* The three passes and the table, asynchronous on the context's stream.  Needs a finished ta_extract of the current volume (any
 * feature mask: the table takes its rows), else TA_EINVAL; TA_EINVAL for a bad mode, unknown flags, a spacing that is not positive
 * and finite, and for a slab.  site_label is read in mode 1 only.  A new label volume, ta_volume_relabel, ta_components_relabel,
 * ta_volume_rerank, compaction or its end, and a new ta_extract invalidate the results: the getters then answer TA_EINVAL. */
TA_API int ta_distance_extract(ta_ctx* ctx, int mode, uint32_t site_label, const double spacing[3], uint32_t flags);
/* The table: min2 [R], max2 [R], pole [R][3], R = max_label + 1 of the extraction; any pointer may be NULL.  Synchronises.
 * TA_ERANGE when the pass met a label above max_label (the volume changed since ta_extract). */
TA_API int ta_distance_get(ta_ctx* ctx, double* min2, double* max2, int32_t* pole);
/* D2 of the buffer planes first_plane .. first_plane + nplanes - 1 along memory axis 0, in memory order: d2 [nplanes * m1 * m2]
 * on the host.  Synchronises.  TA_EINVAL for planes outside the buffer. */
TA_API int ta_distance_image(ta_ctx* ctx, int64_t first_plane, int64_t nplanes, double* d2);
/* Milliseconds between HIP events.  ms_pass: the row pass and the two column passes.  ms_after: the two table passes.  Either
 * pointer may be NULL. */
TA_API int ta_distance_timing(ta_ctx* ctx, double* ms_pass, double* ms_after);
/* Diagnostics for tests: what the last ta_distance_extract launched.  out[0] the workgroups of the row pass (four rows each at a
 * time), out[1] those of the extremes and of the pole kernel (256 voxels each at a time), out[2] those of the table initialisation
 * (256 rows each at a time), out[3] the launches of the column kernel, both axes together.  Fewer workgroups than work means that
 * the kernel strode over it.  TA_EINVAL as the getters above. */
TA_API int ta_distance_debug(ta_ctx* ctx, uint32_t out[4]);
/* Columns a launch of a column pass takes (tuning and tests): 0 = automatic (what fits the work buffer's cap), else rounded up to
 * whole waves of 64.  The results do not depend on it. */
TA_API int ta_distance_set_batch(ta_ctx* ctx, int64_t columns);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_DISTANCE_H */
