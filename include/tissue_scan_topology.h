/* tissue_scan_topology.h -- exact per-cell Euler numbers: tunnels and cavities (libtissue_scan.so; the entry points live in the
 * same library as tissue_scan.h and follow its conventions).
 *
 * What it is for: a cell should be a topological ball.  Segmentations hold labels with a tunnel through them (a watershed leak
 * around a neighbour), labels that enclose a cavity (a speck of another label swallowed whole) and labels that hang together
 * only across a voxel edge or corner.  The Euler number of every label, for 6- and for 26-connectivity, follows from twelve exact
 * integers per label, all counted in one pass over the 2 x 2 x 2 blocks of the resident volume.  With the blob count b0 of the
 * component pass (tissue_scan_components.h), b0 - chi = tunnels - cavities: chi != b0 flags every label that is not a union of
 * balls.  The same integers give the intrinsic volumes of the voxel solid: mean breadth, and half its surface.  Users of the
 * reference crop every label and call skimage.measure.euler_number per bounding box in Python.
 *
 * Definitions.  The volume has dims N0 x N1 x N2 in MEMORY-axis order; voxels outside it hold no label.  A block has origin
 * o in [-1, N0-1] x [-1, N1-1] x [-1, N2-1] and holds the eight voxels o + {0,1}^3; its voxels are indexed by bit 4a + 2b + c,
 * (a, b, c) the offset along memory axes 0, 1, 2.  The upper half along axis 0 is bits {4,5,6,7}, along axis 1 {2,3,6,7}, along
 * axis 2 {1,3,5,7}.  Every lattice vertex is the centre of exactly one block, the vertices on the faces of the volume included;
 * every lattice edge is the + edge of exactly one vertex; every 2 x 2 square and every face-adjacent pair is found in exactly
 * one block.  Per row l (rows as those of the last ta_extract: 0 .. max_label, or the ranks of a compacted context; R of them),
 * all u64 -- what a block adds for l:
 *    n0      1 if voxel 7 is l (equals ta_get_labels' count)
 *    n1[a]   1 if voxel 7 and its lower neighbour along axis a (bits 3, 5 and 6 for a = 0, 1, 2) are both l: same-label face pairs
 *    n2[a]   1 if all four voxels of the upper half along a are l: 2 x 2 squares normal to a
 *    n3      1 if all eight are l
 *    v       1 if any of the eight is l: lattice vertices the label touches
 *    e[a]    1 if any of the four voxels of the upper half along a is l: lattice edges along a the label touches
 *  The host derives the rest, in exact integers:
 *    faces normal to a      F_a   = 2 n0 - n1[a]
 *    6-connectivity         chi6  = n0 - sum n1 + sum n2 - n3           (the label's voxels joined across faces only)
 *    26-connectivity        chi26 = v - sum e + sum F_a - n0            (the closed voxel solid: faces, edges and corners join)
 *  and with the voxel size s per memory axis, A_a the product of the other two sizes:
 *    V1 = sum_a s_a (e[a] - sum_{b != a} F_b + n0)      mean breadth is V1 / 2; a box of a x b x c voxels: a s0 + b s1 + c s2
 *    V2 = sum_a A_a (F_a - n0)                          half the surface of the solid, the faces on the image border included
 *  A ball gives (chi6, chi26) = (1, 1), a hollow shell (2, 2), a solid torus (0, 0); two voxels that share only an edge or only
 *  a corner give (2, 1).  Each label of a multi-label image gives the numbers of its binary mask on its own.
 *
 * Exactness and widths.  Every number is an exact integer, bit-identical whatever the order of the atomics.  Every column is at
 * most the number of blocks, (N0 + 1)(N1 + 1)(N2 + 1), far below 2^64.  A workgroup's LDS counters are u32: it walks at most
 * 2^31 voxel positions (the cap of the other range passes) and at most one block more per row and plane of a tile, fewer than
 * 2^32 blocks in all.
 *
 * Slabs are out of scope, as for the distance and nearest-label passes: a block at a seam belongs to two buffers.
 */
#ifndef TISSUE_SCAN_TOPOLOGY_H
#define TISSUE_SCAN_TOPOLOGY_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One pass over the blocks of the resident volume, asynchronous on the context's stream.  TA_EINVAL without a finished ta_extract
 * of the current volume, and on a slab context (a_origin != 0 or a low halo).  A new volume, ta_volume_relabel,
 * ta_components_relabel, ta_nearest_apply, compaction or its end or a new ta_extract invalidates the results -- the events that
 * invalidate ta_sigmom_extract's, less the new signal this pass does not read: the getters then answer TA_EINVAL. */
TA_API int ta_topology_extract(ta_ctx* ctx);
/* The rows; any pointer may be NULL.  Synchronises.  TA_ERANGE when the pass met a label above max_label (the volume changed
 * since ta_extract). */
TA_API int ta_topology_get(ta_ctx* ctx, uint64_t* n0 /* [R] */, uint64_t* n1 /* [R][3] */, uint64_t* n2 /* [R][3] */,
                           uint64_t* n3 /* [R] */, uint64_t* v /* [R] */, uint64_t* e /* [R][3] */);
/* Diagnostics of the last pass, for tests: out[0] the records that found no slot in a workgroup's LDS table and went to the global
 * rows directly (the results are the same), out[1] the blocks that held more than one label (saturating at 2^32 - 1), out[2] the
 * tiles a workgroup took, out[3] the workgroups.  Valid when the getter is; TA_ERANGE as it answers it.  Synchronises. */
TA_API int ta_topology_debug(ta_ctx* ctx, uint32_t out[4]);
/* Milliseconds between two HIP events around the pass kernel of the last ta_topology_extract. */
TA_API int ta_topology_timing(ta_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_TOPOLOGY_H */
