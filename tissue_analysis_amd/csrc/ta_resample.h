// ta_resample.h -- launcher of kernels_resample.hip: a source volume sampled through an affine map onto the grid of the resident
// label volume (include/tissue_scan_resample.h).
#pragma once
#include "ta_device.h"

namespace ta {

enum { RS_NEAREST = 0, RS_LINEAR = 1 };

struct ResampleArgs {
    const void* src;             // source S (u8, u16 or u32)
    void* out;                   // output, dense C-ordered [n0][n1][n2] of the source's type
    int64_t n0, n1, n2;          // output buffer dims in MEMORY-axis order; n0 counts the halo plane when first_owned == 1
    int64_t a_origin;            // global coordinate along memory axis 0 of buffer plane `first_owned`
    int32_t first_owned;         // 0, or 1 when plane 0 is the low halo of a slab
    int32_t mem_of[3];           // mem_of[a] = the memory axis of the target's array axis a
    int64_t m[3];                // source dims, array-axis order
    int64_t es[3];               // source element strides, array-axis order
    double A[12];                // the map, array-axis order (rows: source axis, columns: target axis | offset)
    uint32_t fill;
    unsigned long long* outside; // owned voxels that received `fill` (zeroed before the pass)
    uint32_t tiles_per_group;    // (set by launch_resample)
};

// One gather pass.  Returns the plan it launched; *vec (may be NULL): it wrote whole 16-byte strips.
RangePlan launch_resample(hipStream_t s, ResampleArgs a, int itemsize, int mode, bool* vec);

}  // namespace ta
