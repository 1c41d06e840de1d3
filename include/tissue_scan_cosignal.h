/* tissue_scan_cosignal.h -- two-channel statistics per cell: ratio, correlation, colocalisation (libtissue_scan.so; the entry
 * points live in the same library as tissue_scan.h and follow its conventions).
 *
 * What it is for: ratiometric reporters are read as the per-cell ratio of two channels, the colocalisation of a marker with a
 * compartment channel as Pearson's r and Manders' M1 / M2 per cell.  The signal pass (tissue_scan_signal.h) gives sum A and
 * sum B in two runs; it cannot give sum A B, so neither a correlation nor a thresholded overlap.  Users of the reference loop
 * over the labels with scipy.ndimage.
 *
 * Definitions.  V is the label volume of the context.  Channel A is its signal (ta_signal_set / ta_signal_set_device), channel B
 * the companion set here: the same dims and layout, uint8 or uint16 each, chosen independently; B may be the very buffer of A.
 * Rows as those of the last ta_extract: 0 .. max_label, or the ranks of a compacted context; R of them.  Per row, over the owned
 * voxels p with V(p) == r (the halo plane of a has_low_halo slab adds nothing), with the thresholds thr_a, thr_b of the pass:
 *    n                   voxels (equals ta_get_labels' count)                                  u64
 *    sum_a, sum_b        sum of A, of B                                                        u64
 *    sq_aa, sq_bb, sq_ab sum of A^2, of B^2, of A B: 128 bits, low word first                  u64[2]
 *    n_a, n_b, n_ab      voxels with A > thr_a; with B > thr_b; with both                      u64
 *    sum_a_over          sum of A over the voxels with B > thr_b (the numerator of Manders' M1) u64
 *    sum_b_over          sum of B over the voxels with A > thr_a (the numerator of Manders' M2) u64
 *  The comparison is strict: a threshold at or above a channel's largest value leaves zeros.  Every number is an exact integer,
 *  bit-identical whatever the order of the atomics; summed over the slabs of a volume every column equals the whole volume's.
 *  Ratio sum_a / sum_b, covariance (n sq_ab - sum_a sum_b) / n^2, Pearson's r, M1 = sum_a_over / sum_a, M2 = sum_b_over / sum_b
 *  are the host's work, in float64 from exact integers.
 *
 * Both channels lie on the label grid.  A channel on another grid goes through the resample pass (tissue_scan_resample.h) first;
 * that pass owns ONE result buffer, so at most one of the two channels can be adopted from it at a time.
 */
#ifndef TISSUE_SCAN_COSIGNAL_H
#define TISSUE_SCAN_COSIGNAL_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upload channel B from the host: itemsize 1 (uint8) or 2 (uint16); dims and strides as for ta_signal_set (the SAME dims and the
 * SAME dense layout as the label volume of the context, else TA_EINVAL).  The host buffer may be freed after return.  A new label
 * volume of other dims drops B. */
TA_API int ta_cosignal_set(ta_ctx* ctx, const void* host_ptr, int itemsize, const int64_t dims[3], const int64_t strides_bytes[3]);
/* Adopt a B resident in this GPU's HBM: dense C order with the buf_dims of the label volume (halo plane included), not copied,
 * not owned. */
TA_API int ta_cosignal_set_device(ta_ctx* ctx, const void* dev_ptr, int itemsize);
/* One pass over labels + A + B, asynchronous on the context's stream.  TA_EINVAL without a finished ta_extract of the current
 * volume, without an A or without a B of the volume's dims.  A new volume, ta_volume_relabel, ta_components_relabel,
 * ta_nearest_apply, compaction or its end, a new ta_extract, a new A (ta_signal_set, ta_signal_set_device, the resample pass
 * rewriting an adopted A) or a new B invalidates the results: the getters then answer TA_EINVAL. */
TA_API int ta_cosignal_extract(ta_ctx* ctx, uint32_t thr_a, uint32_t thr_b);
/* The rows; any pointer may be NULL.  Synchronises.  TA_ERANGE when the pass met a label above max_label (the volume changed
 * since ta_extract); the pass never writes outside the rows. */
TA_API int ta_cosignal_get(ta_ctx* ctx, uint64_t* n /* [R] */, uint64_t* sum_a /* [R] */, uint64_t* sum_b /* [R] */,
                           uint64_t* sq_aa /* [R][2] */, uint64_t* sq_bb /* [R][2] */, uint64_t* sq_ab /* [R][2] */,
                           uint64_t* n_a /* [R] */, uint64_t* n_b /* [R] */, uint64_t* n_ab /* [R] */,
                           uint64_t* sum_a_over /* [R] */, uint64_t* sum_b_over /* [R] */);
/* Diagnostics of the last pass, for tests: out[0] the label records that found no slot in a workgroup's LDS table and went to the
 * global rows directly (the results are the same), out[1] 0, out[2] the tiles a workgroup took, out[3] the workgroups.  Valid when
 * the getter is; TA_ERANGE as it answers it.  Synchronises. */
TA_API int ta_cosignal_debug(ta_ctx* ctx, uint32_t out[4]);
/* Milliseconds between two HIP events around the pass kernel of the last ta_cosignal_extract. */
TA_API int ta_cosignal_timing(ta_ctx* ctx, double* ms);
/* The thresholds of the last ta_cosignal_extract; valid when the getter is. */
TA_API int ta_cosignal_thresholds(ta_ctx* ctx, uint32_t* thr_a, uint32_t* thr_b);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_COSIGNAL_H */
