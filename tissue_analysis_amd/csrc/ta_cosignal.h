// ta_cosignal.h -- launcher of kernels_cosignal.hip: the joint sums per label of two intensity images A and B (uint8 / uint16 each)
// over the resident label volume (include/tissue_scan_cosignal.h).
#pragma once
#include "ta_device.h"

namespace ta {

// flag words of the pass (device u32[COSIG_NFLAGS], zeroed before every pass)
enum { COSIG_FLAG_RANGE = 0, COSIG_FLAG_SPILL = 1, COSIG_NFLAGS = 4 };
constexpr int COSIG_SLOTS = 512;                    // rows of a workgroup's LDS table (_capi.COSIG_SLOTS): 76 bytes each, four workgroups a CU
constexpr int64_t COSIG_MAX_GROUPS = 1024;          // workgroups of the pass at most (_capi.COSIG_MAX_GROUPS): four a CU, all resident at once

struct CoSigArgs {
    const void* vol;             // labels, dense C-ordered [n0][n1][n2] (u16 or u32; the rank copy of a compacted context)
    const void* a;               // channel A, same buffer dims (u8 or u16)
    const void* b;               // channel B, same buffer dims (u8 or u16); may be the buffer of A
    int64_t n0, n1, n2;          // buffer dims; n0 counts the halo plane when first_owned == 1
    int32_t first_owned;         // 0, or 1 when plane 0 is the low halo of a slab
    uint32_t max_label;          // rows 0 .. max_label
    uint32_t thr_a, thr_b;       // a voxel is "over" in a channel when its value is > the threshold
    unsigned long long* n;       // [max_label + 1] voxels
    unsigned long long* sum_a;   // [max_label + 1] sum of A
    unsigned long long* sum_b;   // [max_label + 1] sum of B
    unsigned long long* sq_aa;   // [max_label + 1][2] sum of A^2: lo, hi words
    unsigned long long* sq_bb;   // [max_label + 1][2] sum of B^2
    unsigned long long* sq_ab;   // [max_label + 1][2] sum of A B
    unsigned long long* n_a;     // [max_label + 1] voxels with A > thr_a
    unsigned long long* n_b;     // [max_label + 1] voxels with B > thr_b
    unsigned long long* n_ab;    // [max_label + 1] voxels with both
    unsigned long long* over_a;  // [max_label + 1] sum of A over the voxels with B > thr_b
    unsigned long long* over_b;  // [max_label + 1] sum of B over the voxels with A > thr_a
    uint32_t* flags;             // [COSIG_NFLAGS]
    uint32_t tiles_per_group;    // (set by launch_cosignal)
};

// one streaming pass over labels + A + B.  The rows and the flags must be zero.  Returns the plan it launched.
RangePlan launch_cosignal(hipStream_t s, CoSigArgs a, int label_itemsize, int a_itemsize, int b_itemsize);

}  // namespace ta
