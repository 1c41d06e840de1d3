/* tissue_scan_resample.h -- resample a second volume of any dims through an affine map onto the grid of the resident label
 * volume (libtissue_scan.so; the entry points live in the same library as tissue_scan.h and follow its conventions).
 *
 * What it is for: frame t+1 of a time lapse, or a signal channel acquired on another grid, brought onto the grid of frame t by a
 * rigid or affine registration the caller already has -- so that ta_overlap_* and ta_signal_* (which take a second volume of the
 * label volume's dims only) can read it, without the image leaving the device.  The reference has nothing here.
 *
 * Definitions.
 *  - Target grid: the grid of the label volume of the context, dims (n0, n1, n2) in array-axis order.
 *  - Target index: output voxel p = (i0, i1, i2) is the GLOBAL voxel index in array-axis order: axis 0 carries the slab's
 *    a0_origin, and the low halo plane of a slab is plane a0_origin - 1.  The output buffer has the label volume's buf_dims
 *    (halo plane included) and its memory layout: what ta_overlap_set_device and ta_signal_set_device expect.
 *  - Source: a dense volume S of dims (m0, m1, m2), independent of the target's; itemsize 1, 2 or 4 (uint8, uint16, uint32).
 *  - Map: twelve doubles A[3][4], row-major, give the continuous source index of a target voxel,
 *        s_x = ((A[x][0] * i0 + A[x][1] * i1) + A[x][2] * i2) + A[x][3]        x = 0, 1, 2
 *    evaluated in IEEE double IN EXACTLY THIS ORDER: every product and every sum is rounded on its own, nothing is fused into a
 *    multiply-add.  This order is part of the ABI: it is what makes the pass bit-identical to a restatement of it anywhere.  A is
 *    in voxel-index units.  A non-finite entry answers TA_EINVAL.
 *  - TA_RS_NEAREST: q_x = floor(s_x + 0.5) (the sum rounded to double first).  Output S[q] when 0 <= q_x < m_x on all three axes,
 *    else `fill`.  The output itemsize equals the source's.
 *  - TA_RS_LINEAR (itemsize 1 or 2 only, else TA_EINVAL): output `fill` unless -0.5 <= s_x < m_x - 0.5 on all three axes.
 *    Otherwise f_x = floor(s_x), w_x = s_x - f_x, the corner indices f_x and f_x + 1 are clamped to [0, m_x - 1], and the value is
 *    three nested lerp(a, b, w) = a + w * (b - a) in double, along axis 2, then axis 1, then axis 0 (again nothing fused), rounded
 *    half to even.  It cannot leave the type's range.
 *  - `fill` is truncated to the output type.
 *  - outside: the number of OWNED target voxels that received `fill` by the rules above; an exact uint64, bit-identical whatever
 *    the order of the atomics.  (A transform that throws the whole frame away is a user error worth seeing.)
 *  - Slabs: every rank holds the whole source.  The outputs of a volume's slabs, laid end to end, equal the whole volume's
 *    output.  The halo plane is written (the adopted buffer is complete) but not counted in `outside`.
 */
#ifndef TISSUE_SCAN_RESAMPLE_H
#define TISSUE_SCAN_RESAMPLE_H

#include "tissue_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TA_RS_NEAREST 0
#define TA_RS_LINEAR 1

/* Upload a host source volume: itemsize 1, 2 or 4; dims in array-axis order and strides as for ta_volume_set (any dense axis
 * permutation).  Needs no label volume.  The host buffer may be freed after return.  Drops the result of an earlier pass. */
TA_API int ta_resample_set_source(ta_ctx* ctx, const void* host_ptr, int itemsize, const int64_t dims[3], const int64_t strides_bytes[3]);
/* Adopt a source resident in this GPU's HBM: dense C order with `dims`, aligned to its type; not copied, not owned. */
TA_API int ta_resample_set_source_device(ta_ctx* ctx, const void* dev_ptr, int itemsize, const int64_t dims[3]);
/* One pass, asynchronous on the context's stream.  Needs a source and a label volume (for its grid only; no ta_extract).
 * mode: TA_RS_NEAREST or TA_RS_LINEAR.  A table that an adopter below handed the old result to is invalidated. */
TA_API int ta_resample_extract(ta_ctx* ctx, const double A[12], int mode, uint32_t fill);
/* Copy `nplanes` buffer planes of the result from `first_plane` (along memory axis 0, halo plane included) to the host.
 * Synchronises. */
TA_API int ta_resample_get(ta_ctx* ctx, void* host_out, int64_t first_plane, int64_t nplanes);
/* The device pointer and the itemsize of the result; owned by the context, valid until the next pass or volume of other dims. */
TA_API int ta_resample_device(ta_ctx* ctx, void** dev_ptr, int* itemsize);
/* `outside` of the last pass.  Synchronises. */
TA_API int ta_resample_outside(ta_ctx* ctx, uint64_t* outside);
/* Milliseconds between two HIP events around the kernel of the last pass. */
TA_API int ta_resample_timing(ta_ctx* ctx, double* ms);
/* Diagnostics of the last pass, for tests: out[0] 1 when it wrote whole 16-byte strips, 0 on the scalar path; out[1] the mode;
 * out[2] the tiles a workgroup took, out[3] the workgroups. */
TA_API int ta_resample_debug(ta_ctx* ctx, uint32_t out[4]);
/* Hand the result to the overlap pass as its B, exactly as ta_overlap_set_device would: a TA_RS_NEAREST result of itemsize 2 or
 * 4, else TA_EINVAL.  The context keeps ownership of the buffer. */
TA_API int ta_resample_as_overlap(ta_ctx* ctx);
/* Hand the result to the signal passes, exactly as ta_signal_set_device would: itemsize 1 or 2, else TA_EINVAL. */
TA_API int ta_resample_as_signal(ta_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* TISSUE_SCAN_RESAMPLE_H */
