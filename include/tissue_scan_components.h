/* tissue_scan_components.h -- connected components of the labels of the resident label volume, and the means to split or erase
 * the fragments of a label (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its
 * conventions).
 *
 * What it is for: every table of this library is keyed by label VALUE and so assumes that a label is one cell.  A label whose
 * voxels form several separate blobs (watershed leaks, resampling, fused labels, an erased label that leaves the background in
 * pieces) gets one volume, one barycentre between the blobs and walls that are really several walls.  This pass finds such
 * labels and can give every fragment a label of its own.  The reference has no such function (its per-label crops silently
 * include all fragments): the semantics below are this library's own.
 *
 * Definitions.  V is the label volume of the context (uint16 or uint32), dims (n0, n1, n2) in array-axis order.
 *  - Component.  A maximal set of voxels of equal label value joined through shared faces: the 6-connectivity of the adjacency and
 *    of the walls.  Voxels that touch only along an edge or at a corner are not joined.
 *  - No label is special: 0, the background and any 32-bit value are labels like the rest.  The pass reads the ids as stored, never
 *    ranks: a compacted context answers in ids too.
 *  - The pass needs a volume, not a finished ta_extract.
 *  - Component table.  One row per component, all exact integers:
 *      label  u32      the label of its voxels
 *      n      u64      its voxels
 *      first  i32[3]   its lexicographically smallest voxel (x0, x1, x2) in array axes; global along the slab axis
 *      bbox   i32[6]   min and max + 1 per array axis
 *      sum1   u64[3]   the sum of its voxels' coordinates in array axes
 *    Rows are sorted ascending by (label, first).
 *  - The table is bit-identical whatever the order of the device's operations, and whatever the memory layout of the image
 *    (C, Fortran, transposed).
 *  - Row image.  For any range of buffer planes along memory axis 0 the pass returns the row index of every voxel as u32.
 *  - Slabs.  In a slab adopted with has_low_halo connectivity is taken over the whole buffer, halo plane included; n, first, bbox
 *    and sum1 are taken over the owned voxels only.  A component with no owned voxel gets no row, and its voxels read
 *    TA_COMPONENT_NONE in the row image.  The tables of a volume's slabs merge into the whole volume's table: two rows of
 *    neighbouring slabs are one component where the row image of the lower slab's top owned plane and that of the upper slab's
 *    halo plane (the same voxels) name rows at the same voxel.  The merged row sums n and sum1, merges bbox and takes the
 *    lexicographic minimum of first.
 *  - The number of rows is not known beforehand: the pass counts the components of the buffer, the tables are then allocated at
 *    that number (count, scan, emit).  In a slab that count includes the components that lie in the halo plane only: they take a
 *    slot and are dropped when the rows are sorted, so the allocation exceeds the rows by at most one plane's voxels.  Never a
 *    silently short table; TA_ENOMEM comes before anything is written to caller memory.
 *  - Coordinates are int32.  An axis of a volume holds at most 2^30 voxels (ta_volume_set), and the global coordinates of a slab
 *    must stay below 2139062143: a0_origin + planes beyond that answers TA_ERANGE from ta_components_extract.
 *  - Size.  One u32 per voxel of the buffer stays on the context as the parent / row image until the tables are invalidated.  A
 *    word of it holds a voxel index or a flagged table slot, so a buffer (halo plane included) may hold at most 2^31 voxels:
 *    n0 * n1 * n2 <= 2147483648.  A larger one answers TA_ERANGE from ta_components_extract and must be cut into slabs.
 */
#ifndef TISSUE_SCAN_COMPONENTS_H
#define TISSUE_SCAN_COMPONENTS_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TA_COMPONENT_NONE 0xFFFFFFFFu  /* row image: a voxel of a component that has no owned voxel */

/* The union-find over the label volume up to the count of its components, asynchronous on the context's stream.  Needs a label
 * volume (else TA_EINVAL), no ta_extract; TA_ERANGE for a buffer of more than 2^31 voxels or global coordinates beyond the
 * int32 bound above.  A new label volume, ta_volume_relabel, ta_volume_rerank (the caller edited the labels in place) and
 * ta_components_relabel invalidate the tables: the functions below then answer TA_EINVAL. */
TA_API int ta_components_extract(ta_ctx* ctx);
/* Rows of the component table.  Synchronises and settles: the slots of the components, their statistics, the sort and the table.
 * TA_ENOMEM when those cannot be allocated. */
TA_API int ta_components_size(ta_ctx* ctx, uint64_t* nrows);
/* The table: label [R], n [R], first [R][3], bbox [R][6], sum1 [R][3]; any pointer may be NULL.  Synchronises (and settles, as
 * above, before anything is written to caller memory). */
TA_API int ta_components_get(ta_ctx* ctx, uint32_t* label, uint64_t* n, int32_t* first, int32_t* bbox, uint64_t* sum1);
/* The row of every voxel of the buffer planes first_plane .. first_plane + nplanes - 1 along memory axis 0 (the halo plane of a
 * slab is plane 0), in memory order: rows [nplanes * m1 * m2] on the host.  TA_EINVAL for planes outside the buffer. */
TA_API int ta_components_image(ta_ctx* ctx, int64_t first_plane, int64_t nplanes, uint32_t* rows);
/* Every voxel of row r becomes new_label[r], in place on the resident volume; voxels without a row stay as they are.  Like
 * ta_volume_relabel for everything downstream: it ends the compacted state and invalidates the extraction, the feature tables and
 * these tables.  TA_EINVAL when nrows is not the table's row count, TA_ERANGE when a value does not fit the volume's item size:
 * both before the volume is touched. */
TA_API int ta_components_relabel(ta_ctx* ctx, const uint32_t* new_label, uint64_t nrows);
/* Diagnostics for tests: what the last pass launched.  out[0] the tiles (= workgroups) of the local pass, out[1] the workgroups
 * of the seam pass, out[2] the workgroups of the last ta_components_image or ta_components_relabel launch since the extract (0 if
 * none), out[3] the workgroups of the kernel that writes the sort keys.  Fewer workgroups than rows (seam pass) or than 256-item
 * chunks (the others) means that the kernel strode over its work.  Synchronises and settles; TA_EINVAL as the getters above. */
TA_API int ta_components_debug(ta_ctx* ctx, uint32_t out[4]);
/* Milliseconds between HIP events.  ms_pass: the kernels that walk the volume (local pass, seams, flatten and count, emit,
 * statistics).  ms_after: everything else on the device, from the scan of the counts to the sorted table (it spans the host's
 * read of the slot count).  Settled tables only (ask ta_components_size first), else TA_EINVAL; either pointer may be NULL. */
TA_API int ta_components_timing(ta_ctx* ctx, double* ms_pass, double* ms_after);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_COMPONENTS_H */
