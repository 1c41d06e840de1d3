/* tissue_scan_overlap.h -- the label-overlap table between the resident label volume and a second label volume of the same
 * grid (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its conventions).
 *
 * What it is for: frame t against frame t+1 resampled onto it (which cell became which: lineage), or two segmentations of one
 * image (Jaccard index, over- and under-segmentation).  The reference has nothing here.
 *
 * Definitions.  A is the label volume of the context (uint16 or uint32).  B is a second label volume, uint16 or uint32
 * independently of A's type, with the SAME dims and the SAME dense layout as A.  The table is the list of rows (a, b, n) with
 *     n = #{ p : A[p] == a and B[p] == b } > 0,
 * sorted ascending by (a, b), each pair once.
 *  - a and b are the labels as the caller stored them, never ranks: a compacted context answers in original ids too.  Any
 *    value up to 2^32 - 1 is legal on either side, and no label is special: 0 and the background are rows like the others.
 *  - The pass needs a volume, not a finished ta_extract.
 *  - In a slab adopted with has_low_halo, B's buffer holds the halo plane too and that plane adds nothing: the tables of the
 *    slabs of a volume, merged by summing n over equal (a, b), equal the whole volume's table.
 *  - All outputs are exact integers: the results are bit-identical whatever the order of the atomics.
 *  - The number of distinct pairs is not known beforehand.  The pass folds into a device hash table of an automatic capacity
 *    (or the one ta_overlap_set_capacity names); a table that fills up raises a flag on the device, and the pass is then run
 *    again into a larger table when the size is first asked for.  Never a silently short table.
 */
#ifndef TISSUE_SCAN_OVERLAP_H
#define TISSUE_SCAN_OVERLAP_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Upload a host label volume B: itemsize 2 (uint16) or 4 (uint32); dims and strides as for ta_volume_set, and they must name
 * the SAME dims and the SAME dense layout (axis permutation) as the label volume of the context, else TA_EINVAL.  The host
 * buffer may be freed after return.  A new label volume of other dims drops B. */
TA_API int ta_overlap_set(ta_ctx* ctx, const void* host_ptr, int itemsize, const int64_t dims[3], const int64_t strides_bytes[3]);
/* Adopt a B resident in this GPU's HBM: dense C order with the buf_dims of the label volume (halo plane included), not
 * copied, not owned. */
TA_API int ta_overlap_set_device(ta_ctx* ctx, const void* dev_ptr, int itemsize);
/* log2 of the slots of the device hash table the next passes start with: 0 = automatic (by the size of the volume), else
 * 4 .. 31.  A table that proves too small is grown and the pass repeated, whatever was asked for. */
TA_API int ta_overlap_set_capacity(ta_ctx* ctx, int log2_slots);
/* One pass over A and B, asynchronous on the context's stream.  Needs a label volume and a B (else TA_EINVAL), no ta_extract.
 * A new label volume, ta_volume_relabel or a new B invalidates the table: the getters then answer TA_EINVAL. */
TA_API int ta_overlap_extract(ta_ctx* ctx);
/* The number of rows.  Synchronises; settles a capacity re-run, compacts the table and sorts it.  TA_ENOMEM when a table or
 * the sorted rows cannot be allocated. */
TA_API int ta_overlap_size(ta_ctx* ctx, uint64_t* npairs);
/* The rows, ta_overlap_size of them, sorted by (a, b); any pointer may be NULL.  Synchronises (and settles, as above, before
 * anything is written to caller memory). */
TA_API int ta_overlap_get(ta_ctx* ctx, uint32_t* a, uint32_t* b, uint64_t* n);
/* Diagnostics of the last run of the pass kernel, for tests: out[0] records that found no slot in a workgroup's LDS table and
 * went to the device table directly (the results are the same); out[1] the runs of the pass kernel (as
 * ta_overlap_timing_compaction); out[2] the tiles a workgroup took, out[3] the workgroups.  Synchronises and settles, as
 * ta_overlap_size. */
TA_API int ta_overlap_debug(ta_ctx* ctx, uint32_t out[4]);
/* Milliseconds between two HIP events around the pass kernel of the last ta_overlap_extract (the last run of it, when the
 * table had to grow). */
TA_API int ta_overlap_timing(ta_ctx* ctx, double* ms);
/* Milliseconds of what follows the pass of a settled table: counting and scanning the occupied slots, emitting them, the
 * sort by (a, b) and the unpacking of the rows (HIP events).  passes: how many times the pass kernel ran (1 = the first
 * table was large enough); may be NULL. */
TA_API int ta_overlap_timing_compaction(ta_ctx* ctx, double* ms, int* passes);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_OVERLAP_H */
