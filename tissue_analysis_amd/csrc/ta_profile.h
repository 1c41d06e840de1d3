// ta_profile.h -- launcher of kernels_profile.hip: per (label, shell of squared distance) the voxels and the statistics of the signal
// image over the resident label volume and its distance image (include/tissue_scan_profile.h).
#pragma once
#include "ta_device.h"

namespace ta {

// flag words of the profile pass (device u32[PROF_NFLAGS], zeroed before every pass)
enum { PROF_FLAG_RANGE = 0, PROF_FLAG_SPILL = 1, PROF_NFLAGS = 4 };
constexpr int PROF_MAX_BINS = 64;                   // TA_PROF_MAX_BINS of the public header
constexpr int PROF_SLOTS = 1024;                    // slots of a workgroup's LDS table (_capi.PROFILE_SLOTS)

struct ProfileArgs {
    const void* vol;             // labels, dense C-ordered [n0][n1][n2] (u16 or u32; the rank copy of a compacted context)
    const double* d2;            // squared distances, same dims
    const void* sig;             // signal, same dims (u8 or u16); not read by a pass without signal
    int64_t n0, n1, n2;          // buffer dims
    uint32_t max_label;          // rows 0 .. max_label
    uint32_t bins;               // K shells a row; (max_label + 1) * K <= 2^31
    unsigned long long* n;       // [R][K] voxels
    unsigned long long* sum;     // [R][K] sum of S                          (the four signal columns: a pass with signal only)
    unsigned long long* sumsq;   // [R][K][2] sum of S^2: lo, hi words
    uint32_t* vmin;              // [R][K] (UINT32_MAX when empty)
    uint32_t* vmax;              // [R][K] (0 when empty)
    uint32_t* flags;             // [PROF_NFLAGS]
    const double* edges;         // [PROF_MAX_BINS + 1] on the device: edges2[0 .. K], +inf behind them
    uint32_t tiles_per_group;    // (set by launch_profile)
};

// one streaming pass over labels + d2 (+ signal: signal_itemsize 1 or 2, 0 = none).  The rows must be initialised by the caller
// (n, sum, sumsq, vmax: 0; vmin: 0xff bytes; flags: 0) and the edges be in place.  Returns the plan it launched.
RangePlan launch_profile(hipStream_t s, ProfileArgs a, int label_itemsize, int signal_itemsize);

}  // namespace ta
