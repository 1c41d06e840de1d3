/* tissue_scan_signal.h -- per-cell and per-wall statistics of an intensity image over the resident label volume
 * (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its conventions).
 *
 * The reference has nothing here: its users call scipy.ndimage.mean(signal, labels, index) and walk the faces in Python.
 *
 * Definitions.  V is the label volume of the context, S the signal image: same dims, same layout, uint8 or uint16.
 *  per label, rows as those of the last ta_extract (0 .. max_label, or ranks in a compacted context):
 *    n[l]         voxels of label l (equals ta_get_labels' count)
 *    sum[l]       sum of S over those voxels                                 u64
 *    sumsq[l][2]  sum of S^2: 128 bits, low word first                       u64[2]
 *    min[l], max[l]  extremes of S; UINT32_MAX / 0 for an absent row         u32
 *  per wall, rows as those of ta_adjacency_get (pairs lo < hi of the last extraction, background pairs included): for every
 *  voxel face the pair's `faces` counts (6-connectivity, all three axes),
 *    side_lo[i] += S[p] where V[p] == lo,   side_hi[i] += S[q] where V[q] == hi     u64
 *  so the wall mean is (side_lo + side_hi) / (2 * sum of faces): FACE-weighted, like the wall areas (a voxel that touches a
 *  wall through two faces counts twice).
 *  In a slab adopted with has_low_halo the signal buffer holds the halo plane too: that plane adds nothing to the per-label
 *  rows, the faces between it and plane 1 belong to this slab.  Summed over slabs every number equals the whole volume's.
 *  All outputs are exact integers; mean / std / min / max in float64 are the host's work.
 */
#ifndef TISSUE_SCAN_SIGNAL_H
#define TISSUE_SCAN_SIGNAL_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what ta_signal_extract computes */
#define TA_SIG_LABELS 1u
#define TA_SIG_WALLS  2u

/* Upload a host signal image: itemsize 1 (uint8) or 2 (uint16); dims and strides as for ta_volume_set, and they must name the
 * SAME dims and the SAME dense layout (axis permutation) as the label volume of the context, else TA_EINVAL.  The host
 * buffer may be freed after return.  A new label volume of other dims drops the signal. */
TA_API int ta_signal_set(ta_ctx* ctx, const void* host_ptr, int itemsize, const int64_t dims[3], const int64_t strides_bytes[3]);
/* Adopt a signal resident in this GPU's HBM: dense C order with the buf_dims of the label volume (halo plane included),
 * not copied, not owned. */
TA_API int ta_signal_set_device(ta_ctx* ctx, const void* dev_ptr, int itemsize);
/* One pass over labels + signal, asynchronous on the context's stream.  Needs a finished ta_extract of the current volume
 * (with TA_F_ADJACENCY, and a LOCAL pair list, for TA_SIG_WALLS), else TA_EINVAL.  A new volume, ta_volume_relabel,
 * compaction or its end, a new ta_extract or a new signal invalidates the results: the getters then answer TA_EINVAL. */
TA_API int ta_signal_extract(ta_ctx* ctx, uint32_t what);
/* Per-label rows (max_label + 1 of them, as ta_get_labels); any pointer may be NULL.  Synchronises. */
TA_API int ta_signal_get_labels(ta_ctx* ctx, uint64_t* n, uint64_t* sum, uint64_t* sumsq /* [L+1][2] */, uint32_t* min,
                                uint32_t* max);
/* Per-wall sums, one per pair of ta_adjacency_get (ta_adjacency_size of them); either pointer may be NULL.  Synchronises. */
TA_API int ta_signal_get_walls(ta_ctx* ctx, uint64_t* side_lo, uint64_t* side_hi);
/* Diagnostics of the last pass, for tests: out[0] per-label records and out[1] per-wall records that found no slot in a
 * workgroup's LDS tables and went to the global rows directly (the results are the same); out[2] the tiles a workgroup took,
 * out[3] the workgroups.  Valid when either getter above is; TA_ERANGE as they answer it.  Synchronises. */
TA_API int ta_signal_debug(ta_ctx* ctx, uint32_t out[4]);
/* Milliseconds between two HIP events around the pass kernel of the last ta_signal_extract (the pair table is built before). */
TA_API int ta_signal_timing(ta_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_SIGNAL_H */
