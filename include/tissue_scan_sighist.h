/* tissue_scan_sighist.h -- exact per-cell histograms and order statistics (median, quantiles) of the signal image over the
 * resident label volume (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its conventions).
 *
 * What it is for: the signal table (tissue_scan_signal.h) and the shell profiles (tissue_scan_profile.h) are moments.  A reporter
 * quantified per cell is skewed by a few saturated voxels, by a bright neighbour's wall bleeding in and by the dark vacuole; the
 * median and the quartiles are robust against all three, and the share of a cell's voxels above a threshold is a histogram.  Users
 * of the reference call scipy.ndimage.median / histogram(signal, ..., labels, index), a Python loop over label crops.
 *
 * Definitions.  V is the label volume of the context, S its signal (ta_signal_set / ta_signal_set_device): uint8 or uint16,
 * bits = 8 or 16.  Rows as those of the signal table: 0 .. max_label of the last ta_extract, or the ranks of a compacted context;
 * R of them.
 *  - Histogram.  The bin of a voxel p is b(p) = S(p) >> log2_width; B = 2^(bits - log2_width) bins, 1 <= B <= 256: log2_width
 *    0 .. 8 for uint8, 8 .. 16 for uint16.
 *      counts[r][b]    voxels with V == r in bin b                                  u64
 *    The sum of a row is n[r] of the signal table and `count` of the extraction.  In a slab adopted with has_low_halo the halo
 *    plane adds nothing; summed over the slabs the table equals the whole volume's.
 *  - Order statistics.  ranks[r][0 .. nranks) are 0-based ranks, 1 <= nranks <= 8:
 *      value[r][j]     the ranks[r][j]-th smallest of the multiset {S(p) : V(p) == r}   u32
 *    UINT32_MAX where ranks[r][j] >= n[r]; UINT64_MAX is the conventional rank for "none".
 *  - Exactness.  A histogram is a keyed integer reduction, bit-exact whatever the order of the atomics.  An order statistic of an
 *    8- or 16-bit image is an exact integer, found on the device by a radix select: one histogram of the 256 values (uint8), or
 *    one of the high bytes, the choice of each rank's high byte and its remainder, and one of the low bytes under the chosen
 *    high bytes (uint16).  No float leaves the device; medians and interpolated quantiles in float64 are the host's work.
 *  - Limits.  R x 256 <= 2^31 for a histogram (whatever B is) and R x nranks x 256 <= 2^31 for order statistics, else TA_EINVAL:
 *    the tables hold 8 bytes a counter.  A workgroup counts its voxels in 32 bits, as the other passes do.  Order statistics of
 *    a slab (a halo plane or a non-zero origin) answer TA_EINVAL: a local select is not the global one.  Signals wider than 16
 *    bits, quantiles per wall or per distance shell are not offered.
 */
#ifndef TISSUE_SCAN_SIGHIST_H
#define TISSUE_SCAN_SIGHIST_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TA_SIGRANK_MAX_RANKS 8

/* One pass over labels + signal, asynchronous on the context's stream.  TA_EINVAL without a finished ta_extract of the current
 * volume, without a signal of the volume's dims, for log2_width outside the range above, and for R x 256 > 2^31.  A new volume,
 * ta_volume_relabel, ta_components_relabel, ta_volume_rerank, compaction or its end, a new ta_extract or a new signal invalidates
 * the results of both passes of this header: the getters then answer TA_EINVAL. */
TA_API int ta_sighist_extract(ta_ctx* ctx, int log2_width);
/* The table, [R][B] row-major; counts may be NULL.  Synchronises.  TA_ERANGE when the pass met a label above max_label (the
 * volume changed since ta_extract). */
TA_API int ta_sighist_get(ta_ctx* ctx, uint64_t* counts /* [R][B] */);
/* The radix select, asynchronous on the context's stream; nothing goes through the host between its passes.  ranks: R x nranks
 * values on the host, read before the call returns.  TA_EINVAL as ta_sighist_extract, for nranks outside 1 .. TA_SIGRANK_MAX_RANKS,
 * for R x nranks x 256 > 2^31, and on a slab. */
TA_API int ta_sigrank_extract(ta_ctx* ctx, int nranks, const uint64_t* ranks /* host, [R][nranks] */);
/* The order statistics, [R][nranks] row-major; values may be NULL.  Synchronises.  TA_ERANGE as ta_sighist_get. */
TA_API int ta_sigrank_get(ta_ctx* ctx, uint32_t* values /* [R][nranks] */);
/* Diagnostics of the last launch of the digit kernel by either pass (of a uint16 select: its second), for tests: out[0] the counts
 * that found no slot in a workgroup's LDS table and went to the global table directly (the results are the same), out[1] 0, out[2]
 * the tiles a workgroup took, out[3] the workgroups.  TA_ERANGE as the getters answer it.  Synchronises. */
TA_API int ta_sighist_debug(ta_ctx* ctx, uint32_t out[4]);
/* Milliseconds between two HIP events: ms_hist around the kernel of the last ta_sighist_extract, ms_rank around all the kernels
 * of the last ta_sigrank_extract (their sum).  Either pointer may be NULL; NaN for a pass whose results are not valid; TA_EINVAL
 * when neither's are. */
TA_API int ta_sighist_timing(ta_ctx* ctx, double* ms_hist, double* ms_rank);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_SIGHIST_H */
