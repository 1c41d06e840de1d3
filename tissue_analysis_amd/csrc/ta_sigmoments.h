// ta_sigmoments.h -- launcher of kernels_sigmoments.hip: signal-weighted moments per label of the signal image (uint8 / uint16)
// over the resident label volume (include/tissue_scan_sigmoments.h).
#pragma once
#include "ta_device.h"

namespace ta {

// flag words of the pass (device u32[SM_NFLAGS], zeroed before every pass)
enum { SM_FLAG_RANGE = 0, SM_FLAG_SPILL = 1, SM_NFLAGS = 4 };
constexpr int SM_SLOTS = 448;                       // rows of a workgroup's LDS table (_capi.SIGMOM_SLOTS): 88 bytes each, four workgroups a CU
constexpr int64_t SM_MAX_GROUPS = 1024;             // workgroups of the pass at most: four a CU, all resident at once

struct SigMomArgs {
    const void* vol;             // labels, dense C-ordered [n0][n1][n2] (u16 or u32; the rank copy of a compacted context)
    const void* sig;             // signal, same buffer dims (u8 or u16)
    int64_t n0, n1, n2;          // buffer dims; n0 counts the halo plane when first_owned == 1
    int32_t first_owned;         // 0, or 1 when plane 0 is the low halo of a slab
    uint32_t max_label;          // rows 0 .. max_label
    unsigned long long* n;       // [max_label + 1] voxels
    unsigned long long* w;       // [max_label + 1] sum of S
    unsigned long long* m1;      // [max_label + 1][3] sum of S x_k
    unsigned long long* m2;      // [max_label + 1][6][2] sum of S x_j x_k: lo, hi words
    uint32_t* flags;             // [SM_NFLAGS]
    uint32_t tiles_per_group;    // (set by launch_sigmoments)
};

// What the exactness contract of the public header leaves of the launch plan for these buffer dims.  Returns 0 and the plan, 1 when
// the u64 first moments could wrap (nvox g smax >= 2^64), 2 when not even one tile fits the 64-bit rows of a workgroup (most == 0).
int sigmoments_plan(const int64_t dims[3], int first_owned, int label_itemsize, int signal_itemsize, RangePlan* plan);
// one streaming pass over labels + signal, by a plan sigmoments_plan accepted.  The rows and the flags must be zero.
void launch_sigmoments(hipStream_t s, SigMomArgs a, int label_itemsize, int signal_itemsize, const RangePlan& plan);

}  // namespace ta
