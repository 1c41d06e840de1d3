// ta_signal.h -- launchers of kernels_signal.hip: per-label and per-wall statistics of an intensity image (uint8 / uint16)
// over the resident label volume (include/tissue_scan_signal.h).
#pragma once
#include "ta_device.h"

namespace ta {

// flag words of the signal pass (device u32[SIG_NFLAGS], zeroed before every pass)
enum { SIG_FLAG_RANGE = 0, SIG_FLAG_PAIR_MISS = 1, SIG_FLAG_LABEL_SPILL = 2, SIG_FLAG_PAIR_SPILL = 3, SIG_NFLAGS = 4 };
// what the pass computes (TA_SIG_LABELS / TA_SIG_WALLS of the public header)
constexpr uint32_t SIG_LABELS = 1u, SIG_WALLS = 2u;

struct SignalArgs {
    const void* vol;             // labels, dense C-ordered [n0][n1][n2] (u16 or u32; the rank copy of a compacted context)
    const void* sig;             // signal, same buffer dims (u8 or u16)
    int64_t n0, n1, n2;          // buffer dims; n0 counts the halo plane when first_owned == 1
    int32_t first_owned;         // 0, or 1 when plane 0 is the low halo of a slab
    uint32_t max_label;          // rows 0 .. max_label
    unsigned long long* n;       // [max_label + 1] voxels
    unsigned long long* sum;     // [max_label + 1] sum of S
    unsigned long long* sumsq;   // [max_label + 1][2] sum of S^2: lo, hi words
    uint32_t* vmin;              // [max_label + 1] (UINT32_MAX when absent)
    uint32_t* vmax;              // [max_label + 1] (0 when absent)
    const uint64_t* hkeys;       // pair -> row hash of the sorted pair list: keys lo << 32 | hi, EMPTY_KEY when free
    const uint32_t* hrows;       // ... and the row of each key
    uint32_t hmask;              // capacity - 1
    unsigned long long* side_lo; // [npairs] sum of S on the lo side of every face of the pair
    unsigned long long* side_hi; // [npairs] ... on the hi side
    uint32_t* flags;             // [SIG_NFLAGS]
    uint32_t tiles_per_group;    // (set by launch_signal)
};

// open-addressed pair -> row table of keys[0 .. n) (unique); hkeys must hold EMPTY_KEY everywhere (memset 0xff) before
void launch_signal_hash(hipStream_t s, const uint64_t* keys, uint64_t n, uint64_t* hkeys, uint32_t* hrows, uint32_t hmask);
// one streaming pass over labels + signal; `what` = SIG_LABELS | SIG_WALLS.  The rows must be initialised by the caller
// (n, sum, sumsq, vmax: 0; vmin: 0xff bytes; side_lo / side_hi: 0; flags: 0).
// Returns the plan it launched.
RangePlan launch_signal(hipStream_t s, SignalArgs a, int label_itemsize, int signal_itemsize, uint32_t what);

}  // namespace ta
