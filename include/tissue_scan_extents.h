/* tissue_scan_extents.h -- oriented extents per cell: how far every cell reaches along three directions of its own
 * (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its conventions).
 *
 * What it is for: the sweep's second moments give the principal axes of a cell (inertia_axis) and the variances along them, not
 * how long, wide and thick the cell is along those axes, how large it is along a chosen direction such as the organ axis, or how
 * much of its oriented box it fills.  The answer is a minimum and a maximum of a projection per cell: one more pass over the
 * labels, instead of pulling voxel coordinates back per label.
 *
 * Definitions.  V is the label volume of the context.  Rows as those of the last ta_extract: 0 .. max_label, or the ranks of a
 * compacted context; R of them.  Every row r brings three directions as a host table weights[r][k][d] of float64, k = 0 .. 2 the
 * direction and d = 0 .. 2 the MEMORY axis: a weight is the unit direction times the voxel size, already permuted to memory order
 * by the host.  The projection of the voxel at memory indices (x0, x1, x2) -- plane, row, column -- onto direction k is
 *
 *     p = (x0 * w[k][0] + x1 * w[k][1]) + x2 * w[k][2]
 *
 * every product and every sum rounded to float64 on its own, in this order: no fused multiply-add.  Per row and direction,
 * over the voxels with V == r:
 *    lo[r][k] = min p        hi[r][k] = max p        +inf and -inf for a row without voxels
 * A zero result is +0.0, whichever zero a voxel gave.
 *
 * Exactness.  A minimum and a maximum do not depend on the order in which the voxels are visited, and the arithmetic of one
 * projection is pinned above: the results are bit-identical to a restatement in any IEEE-754 float64 arithmetic that rounds each
 * operation on its own (tests/extent_reference.py).  The pass merges order-preserving 64-bit keys of the values with integer
 * atomic minima and maxima.
 *
 * Out of scope: slabs (ta_extents_extract answers TA_EINVAL for a context with a halo plane or an axis-0 origin; an extent over
 * ranks is a minimum of minima the caller can take), the voxels that attain the extremes, extents over many directions at once
 * (Feret diameters), convex hulls.
 */
#ifndef TISSUE_SCAN_EXTENTS_H
#define TISSUE_SCAN_EXTENTS_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One pass over the labels, asynchronous on the context's stream; the table is copied before the call returns.  TA_EINVAL
 * without a finished ta_extract of the current volume, for a slab, when `rows` is not the R of that extraction, when a weight
 * is not finite, or so large that a projection could overflow (|w| * largest dim * 4 > DBL_MAX).  A new volume,
 * ta_volume_relabel, ta_components_relabel, ta_nearest_apply, compaction or its end, or a new ta_extract invalidates the
 * results: the getters then answer TA_EINVAL. */
TA_API int ta_extents_extract(ta_ctx* ctx, const double* weights /* host, [rows][3][3] */, uint32_t rows);
/* The rows, decoded to float64; either pointer may be NULL.  Synchronises.  TA_ERANGE when the pass met a label above
 * max_label (the volume changed since ta_extract). */
TA_API int ta_extents_get(ta_ctx* ctx, double* lo /* [rows][3] */, double* hi /* [rows][3] */);
/* Diagnostics of the last pass, for tests: out[0] the records that found no slot in a workgroup's LDS table and went to the global
 * rows directly (the results are the same), out[1] 0, out[2] the tiles a workgroup took, out[3] the workgroups.  Valid when the
 * getter is; TA_ERANGE as it answers it.  Synchronises. */
TA_API int ta_extents_debug(ta_ctx* ctx, uint32_t out[4]);
/* Milliseconds between two HIP events around the pass kernel of the last ta_extents_extract. */
TA_API int ta_extents_timing(ta_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_EXTENTS_H */
