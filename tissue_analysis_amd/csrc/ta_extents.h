// ta_extents.h -- launcher of kernels_extents.hip: per label the minimum and the maximum of three float64 projections of its
// voxels over the resident label volume (include/tissue_scan_extents.h).
#pragma once
#include "ta_device.h"

namespace ta {

// flag words of the pass (device u32[EX_NFLAGS], zeroed before every pass)
enum { EX_FLAG_RANGE = 0, EX_FLAG_SPILL = 1, EX_NFLAGS = 4 };
constexpr int EX_SLOTS = 768;                       // rows of a workgroup's LDS table (_capi.EXTENT_SLOTS): 52 bytes each, four workgroups a CU
constexpr int64_t EX_MAX_GROUPS = 1024;             // workgroups of the pass at most: four a CU, all resident at once

// The order-preserving key of a float64: a < b as numbers <=> key(a) < key(b) as u64 (v + 0.0 first: -0.0 and +0.0 share a key).
// Negative values have all bits flipped, the others the top bit set.
constexpr uint64_t EX_KEY_POS_INF = 0xFFF0000000000000ull;     // key(+inf): where a minimum starts
constexpr uint64_t EX_KEY_NEG_INF = 0x000FFFFFFFFFFFFFull;     // key(-inf): where a maximum starts
inline double extent_of_key(uint64_t k) {
    const uint64_t bits = (k >> 63) ? k ^ (1ull << 63) : ~k;
    double v;
    __builtin_memcpy(&v, &bits, 8);
    return v;
}

struct ExtentArgs {
    const void* vol;             // labels, dense C-ordered [n0][n1][n2] (u16 or u32; the rank copy of a compacted context)
    int64_t n0, n1, n2;          // buffer dims (no halo plane: the pass does not take a slab)
    uint32_t max_label;          // rows 0 .. max_label
    const double* weights;       // [max_label + 1][3][3]: direction k, memory axis d
    unsigned long long* lo;      // [max_label + 1][3] keys of the minima, EX_KEY_POS_INF before the pass
    unsigned long long* hi;      // [max_label + 1][3] keys of the maxima, EX_KEY_NEG_INF before the pass
    uint32_t* flags;             // [EX_NFLAGS]
    uint32_t tiles_per_group;    // (set by launch_extents)
};

// the launch plan for these buffer dims; 0, 0 for an empty volume
RangePlan extents_plan(const int64_t dims[3], int label_itemsize);
// the key rows of a pass: `count` words of `value` each (on the stream, before launch_extents)
void launch_extents_fill(hipStream_t s, unsigned long long* lo, unsigned long long* hi, uint64_t count);
// one streaming pass over the labels, by extents_plan's plan.  The rows must hold the start keys and the flags zero.
void launch_extents(hipStream_t s, ExtentArgs a, int label_itemsize, const RangePlan& plan);

}  // namespace ta
