/* tissue_scan_sigmoments.h -- signal-weighted moments per cell: where in the cell the signal sits (libtissue_scan.so; the entry
 * points live in the same library as tissue_scan.h and follow its conventions).
 *
 * What it is for: the signal table (tissue_scan_signal.h), the histograms (tissue_scan_sighist.h) and the shell profiles
 * (tissue_scan_profile.h) say how much signal a cell holds.  The signal's centroid, its displacement from the cell's barycentre
 * (polarity) and the axes along which it is spread follow from eleven exact integers per cell.  Users of the reference call
 * scipy.ndimage.center_of_mass(signal, labels, index) and loop over bounding boxes in Python for the rest.
 *
 * Definitions.  V is the label volume of the context, S its signal (ta_signal_set / ta_signal_set_device; there is no second
 * upload slot): uint8 or uint16.  Rows as those of the last ta_extract: 0 .. max_label, or the ranks of a compacted context; R of
 * them.  Coordinates are in MEMORY-axis order, k = 0, 1, 2:
 *    x0   the plane index counted from the first owned plane of this context's buffer: LOCAL, a_origin is not added
 *    x1   the row
 *    x2   the column
 *  per row, over the owned voxels p with V(p) == r (the halo plane of a has_low_halo slab adds nothing):
 *    n        voxels (equals ta_get_labels' count)                                   u64
 *    w        sum of S                                                               u64
 *    m1[3]    sum of S x_k                                                           u64[3]
 *    m2[6][2] sum of S x_j x_k for (j, k) = 00, 01, 02, 11, 12, 22: 128 bits, low word first   u64[6][2]
 *  Shifting to global axis-0 coordinates, x0 -> x0 + o with o = a_origin, is exact integer work of the host -- in this order,
 *  every right-hand side being the local value:
 *    m2_00 += 2 o m1_0 + o^2 w
 *    m2_0k += o m1_k            (k = 1, 2)
 *    m1_0  += o w
 *  (m1_0 then needs more than 64 bits when (a_origin + planes) n_vox smax does).  Summed over the slabs of a volume after that
 *  shift, every number equals the whole volume's.  The coordinates are local so that the bounds below depend on the buffer dims
 *  only.  Centroid m1 / w, covariance (w m2_jk - m1_j m1_k) / w^2, the axis permutation of a volume that is not C-ordered and
 *  the voxel size are the host's work, in float64 from exact integers.
 *
 * Exactness.  Every number is an exact integer, bit-identical whatever the order of the atomics; nothing wraps silently at any
 * size the pass accepts.  With gmax the largest buffer dim, g = max(gmax - 1, 1), nvox the voxels of the buffer and smax = 255
 * (uint8) or 65535 (uint16):
 *  - n, w and m1 are u64: ta_sigmom_extract answers TA_EINVAL when nvox g smax >= 2^64.
 *  - m2 is 128-bit in global memory: the add to the low word returns the old value, and an add that wraps it carries one into
 *    the high word.
 *  - a workgroup's LDS rows and a lane's running record are 64-bit; a workgroup therefore takes at most
 *        most = floor( floor(2^64 / (g^2 smax)) / tile_voxels )
 *    tiles (tile_voxels = 4 rows x 64 lanes x 16 / sizeof(label) columns x 16 planes), beside the 2^31-voxel cap that keeps its
 *    u32 n.  most == 0 answers TA_EINVAL: the dims are too large for the pass.  At 2048^3 with a uint16 signal the bound is
 *    6.7e7 voxels a workgroup, far above what the launch plan asks for.
 */
#ifndef TISSUE_SCAN_SIGMOMENTS_H
#define TISSUE_SCAN_SIGMOMENTS_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One pass over labels + signal, asynchronous on the context's stream.  TA_EINVAL without a finished ta_extract of the current
 * volume, without a signal of the volume's dims (as ta_signal_extract answers), and for dims beyond the exactness bounds above.
 * A new volume, ta_volume_relabel, ta_components_relabel, ta_nearest_apply, compaction or its end, a new ta_extract or a new
 * signal invalidates the results: the getters then answer TA_EINVAL. */
TA_API int ta_sigmom_extract(ta_ctx* ctx);
/* The rows; any pointer may be NULL.  Synchronises.  TA_ERANGE when the pass met a label above max_label (the volume changed
 * since ta_extract). */
TA_API int ta_sigmom_get(ta_ctx* ctx, uint64_t* n /* [R] */, uint64_t* w /* [R] */, uint64_t* m1 /* [R][3] */,
                         uint64_t* m2 /* [R][6][2] */);
/* Diagnostics of the last pass, for tests: out[0] the records that found no slot in a workgroup's LDS table and went to the global
 * rows directly (the results are the same), out[1] 0, out[2] the tiles a workgroup took, out[3] the workgroups.  Valid when the
 * getter is; TA_ERANGE as it answers it.  Synchronises. */
TA_API int ta_sigmom_debug(ta_ctx* ctx, uint32_t out[4]);
/* Milliseconds between two HIP events around the pass kernel of the last ta_sigmom_extract. */
TA_API int ta_sigmom_timing(ta_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_SIGMOMENTS_H */
