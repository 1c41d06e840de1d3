/* tissue_scan_nearest.h -- exact nearest-label maps of the resident label volume: for every voxel the squared distance to the nearest
 * site voxel and the label of that site, the count of the empty voxels every label would gain, and the volume with its empty voxels
 * given to the label they lie nearest to (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its
 * conventions).
 *
 * What it is for: every method that repairs a segmentation ends by writing a hole into the image (voxels set to an erase value), and
 * this is the complement: "give every erased voxel to the cell it lies nearest to".  Users know it as
 * scipy.ndimage.distance_transform_edt(..., return_indices=True) followed by a gather, or as skimage.segmentation.expand_labels, which
 * is also how nuclei are grown into cell territories.  The result is the exact Voronoi tessellation of the sites, with a stated rule
 * for the voxels that lie equally near to several labels, so that it is the same for every memory layout.
 *
 * Definitions.  V is the label volume of the context (uint16 or uint32, any dense layout), dims (n0, n1, n2) in array-axis order.
 * spacing[3] holds positive finite doubles in array-axis order.
 *  - Empty voxels are the voxels with V == empty_label.
 *  - Sites are all other voxels.  With TA_NEAREST_NOT_FROM the voxels of not_from_label are not sites either: they are neither sites
 *    nor filled and stay as they are (a hole next to the background then goes to a cell and not to the background).
 *  - D2(p) = min over the sites q of  sum_a (spacing[a] * (p_a - q_a))^2,  a float64; +inf when there is no site, 0 at a site.
 *    Distances run between voxel centres.
 *  - N(p) = the SMALLEST label among the sites at distance exactly D2(p); at a site N(p) = V(p).  It is defined for every voxel (the
 *    voxels of not_from_label get their nearest site too); TA_NEAREST_NONE where there is no site.
 *  - A voxel is FILLED when it is empty and D2(p) <= max_d2.  max_d2 is a float64 >= 0, +inf = no limit; the bound is inclusive.
 *    Where there is no site nothing is filled.
 *  - Exactness.  Where every spacing is a power of two (1 included) and every squared distance, in units of the smallest spacing
 *    squared, stays below 2^53, D2 and N are bit-identical to the definition for every memory layout: every product and sum of the
 *    passes is exact, and the boundary between two parabolas of the lower envelope,
 *        ((f(q) + w^2 q^2) - (f(v) + w^2 v^2)) / (2 w^2 (q - v)),
 *    has an exact numerator and denominator and a correctly rounded quotient, so that "equally near" is decided as in exact arithmetic.
 *    A pass along one axis that resolves ties to the smallest label composes over the three axes, because the minimum over a union is
 *    the minimum of the minima.  For other spacings D2 agrees with the definition to 1e-12 relative, and N is a label with a site
 *    within D2 * (1 + 1e-12).
 *  - Compacted context (sparse ids).  The passes read ranks; empty_label and not_from_label are ids that are looked up.  An id the
 *    volume does not hold means "no voxel is empty" or "nothing excluded" and is no error.  The images answer in ids, the table has one
 *    row per row of the extraction (ranks).  Ranks preserve order: the smallest rank is the smallest id.
 *  - Slabs are out of scope (an exact transform needs halos of unbounded depth): a volume adopted with a halo plane or a non-zero
 *    origin answers TA_EINVAL.
 *  - Limits.  The buffer holds fewer than 2^63 bytes; coordinates are int32 (an axis holds at most 2^30 voxels, ta_volume_set).
 *  - Size.  One float64 and one uint32 per voxel stay on the context until the results are invalidated, and a work buffer of at most
 *    1 GiB (or one batch of 64 columns, if that is more) holds the envelopes of a batch of columns.  Nothing is shared with the
 *    distance maps of tissue_scan_distance.h: a distance map and a nearest map can both be current.
 */
#ifndef TISSUE_SCAN_NEAREST_H
#define TISSUE_SCAN_NEAREST_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TA_NEAREST_NOT_FROM 1u           /* flag: the voxels of not_from_label are no sites (and are not filled) */
#define TA_NEAREST_NONE     0xFFFFFFFFu  /* N of a voxel of a volume without a site */

/* The three passes and the counts, asynchronous on the context's stream.  Needs a finished ta_extract of the current volume (any
 * feature mask: the counts take its rows), else TA_EINVAL; TA_EINVAL for unknown flags, a spacing that is not positive and finite,
 * max_d2 negative or NaN, and for a slab.  not_from_label is read with TA_NEAREST_NOT_FROM only.  A new label volume,
 * ta_volume_relabel, ta_components_relabel, ta_nearest_apply, ta_volume_rerank, compaction or its end, and a new ta_extract
 * invalidate the results: the functions below then answer TA_EINVAL. */
TA_API int ta_nearest_extract(ta_ctx* ctx, uint32_t empty_label, uint32_t not_from_label, const double spacing[3], double max_d2, uint32_t flags);
/* gained [R], R = max_label + 1 of the extraction: the filled voxels by the label they take; totals = {filled voxels, empty voxels
 * left unfilled}; either pointer may be NULL.  Synchronises.  TA_ERANGE when the pass met a label above max_label (the volume changed
 * since ta_extract). */
TA_API int ta_nearest_get(ta_ctx* ctx, uint64_t* gained, uint64_t totals[2]);
/* N and D2 of the buffer planes first_plane .. first_plane + nplanes - 1 along memory axis 0, in memory order: nearest and d2
 * [nplanes * m1 * m2] on the host; either pointer may be NULL.  Ids in a compacted context.  Synchronises.  TA_EINVAL for planes
 * outside the buffer. */
TA_API int ta_nearest_image(ta_ctx* ctx, int64_t first_plane, int64_t nplanes, uint32_t* nearest, double* d2);
/* Writes N(p) into every filled voxel of the resident volume (the caller's own buffer, if it was adopted), and into the rank copy of
 * a compacted context.  Then as ta_components_relabel: every table, this one included, is stale, and the caller sweeps again (no
 * new id can appear, but an id may have lost its last voxel). */
TA_API int ta_nearest_apply(ta_ctx* ctx);
/* Milliseconds between HIP events.  ms_pass: the row pass and the two column passes.  ms_after: the counting pass.  Either pointer may
 * be NULL. */
TA_API int ta_nearest_timing(ta_ctx* ctx, double* ms_pass, double* ms_after);
/* Diagnostics for tests: what the last ta_nearest_extract launched.  out[0] the workgroups of the row pass (four rows each at a
 * time), out[1] those of the counting pass (256 voxels each at a time), out[2] those ta_nearest_apply launches for this volume (256
 * voxels each at a time), out[3] the launches of the column kernel, both axes together.  Fewer workgroups than work means that the
 * kernel strode over it.  TA_EINVAL as the getters above. */
TA_API int ta_nearest_debug(ta_ctx* ctx, uint32_t out[4]);
/* Columns a launch of a column pass takes (tuning and tests): 0 = automatic (what fits the work buffer's cap), else rounded up to
 * whole waves of 64.  The results do not depend on it. */
TA_API int ta_nearest_set_batch(ta_ctx* ctx, int64_t columns);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_NEAREST_H */
