/* tissue_scan_profile.h -- distance-shell profiles: per label and per shell of squared distance, the voxels and the statistics of
 * the signal image (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its conventions).
 *
 * What it is for: the distance table (tissue_scan_distance.h) says how far a cell's voxels lie from their sites at the two extremes;
 * the signal table (tissue_scan_signal.h) says how much signal a cell holds.  WHERE in the cell the signal sits -- how much of it
 * within 1 um of the wall, the volume of the cortical shell or of the cell eroded by a ball of radius r, how the signal falls off
 * with depth below the tissue surface -- is one keyed reduction over (label, distance shell) of the two images the context already
 * holds.  Users of the reference download the distance image and loop over label crops.
 *
 * Definitions.  V is the label volume of the context, D2 the image of squared distances it currently holds (the last
 * ta_distance_extract, whichever mode and flags it ran with), S the signal of the context (optional).
 *  - edges2[0 .. K] is a strictly ascending array of K + 1 float64, edges2[0] >= 0, no NaN, 1 <= K <= 64; the last may be +inf.
 *  - A voxel p with  edges2[k] <= D2(p) < edges2[k + 1]  belongs to shell k of row V(p): in float64,
 *    numpy.searchsorted(edges2, d2, side='right') - 1 where that lies in 0 .. K - 1.  A voxel below edges2[0], at or above
 *    edges2[K], or with D2 = +inf is counted nowhere (+inf also when edges2[K] is +inf: inf < inf is false).
 *  - Table.  Rows as those of the last ta_extract (0 .. max_label, or the ranks of a compacted context), K shells a row:
 *      n[r][k]         voxels                                                      u64
 *    and with a signal
 *      sum[r][k]       sum of S over those voxels                                  u64
 *      sumsq[r][k][2]  sum of S^2: 128 bits, low word first (as the signal table)  u64[2]
 *      min, max        extremes of S; UINT32_MAX / 0 where n == 0                  u32
 *  - Exactness.  Every output is an integer and the float comparisons are exact: for a given D2 image the table is defined bit for
 *    bit, whatever the order of the atomics.  (D2 itself is bit-identical to its definition for power-of-two spacings.)
 *  - Limits.  rows x K <= 2^31: the key of a record is row * K + shell in 32 bits, 0xFFFFFFFF being "no record", and the table
 *    holds 40 bytes per (row, shell) with a signal, 8 without.  More answers TA_EINVAL, as a pair list too large for the index of the
 *    signal and wall-geometry passes does.  A workgroup counts its voxels in 32 bits, as those passes do.
 *  - Slabs: the distance map refuses them, so there is never a D2 image of a slab to profile.
 */
#ifndef TISSUE_SCAN_PROFILE_H
#define TISSUE_SCAN_PROFILE_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TA_PROF_SIGNAL   1u   /* what: also sum, sumsq, min and max of the signal image */
#define TA_PROF_MAX_BINS 64

/* One pass over labels + D2 (+ signal), asynchronous on the context's stream.  edges2: nbins + 1 doubles on the host, read before
 * the call returns.  TA_EINVAL without valid distance results (ta_distance_extract of the current extraction), without a signal
 * of the volume's dims while TA_PROF_SIGNAL is set, for nbins outside 1 .. TA_PROF_MAX_BINS, for edges that do not ascend strictly
 * or are negative or NaN, for unknown bits in `what`, and for rows x nbins > 2^31.  Everything that invalidates the distance
 * results, a new ta_distance_extract, and a new signal when the pass used one invalidate the table: the getters then answer
 * TA_EINVAL. */
TA_API int ta_profile_extract(ta_ctx* ctx, int nbins, const double* edges2, uint32_t what);
/* The table: arrays [R][K], row-major (sumsq [R][K][2]), R = max_label + 1 of the extraction; any pointer may be NULL.
 * Synchronises.  TA_ERANGE when the pass met a label above max_label (the volume changed since ta_extract); TA_EINVAL for a signal
 * column of a pass that ran without TA_PROF_SIGNAL. */
TA_API int ta_profile_get(ta_ctx* ctx, uint64_t* n, uint64_t* sum, uint64_t* sumsq, uint32_t* min, uint32_t* max);
/* Diagnostics of the last pass, for tests: out[0] the records that found no slot in a workgroup's LDS table and went to the global
 * rows directly (the results are the same), out[1] 0, out[2] the tiles a workgroup took, out[3] the workgroups.  TA_ERANGE as
 * ta_profile_get answers it.  Synchronises. */
TA_API int ta_profile_debug(ta_ctx* ctx, uint32_t out[4]);
/* Milliseconds between two HIP events around the pass kernel of the last ta_profile_extract. */
TA_API int ta_profile_timing(ta_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_PROFILE_H */
