// ta_wallgeo.h -- launcher of kernels_wallgeo.hip: per-wall face geometry (signed face counts, first and second sums of the
// doubled face centres) over the resident label volume (include/tissue_scan_wallgeo.h).
#pragma once
#include "ta_device.h"

namespace ta {

// flag words of the wall-geometry pass (device u32[WG_NFLAGS], zeroed before every pass)
enum { WG_FLAG_PAIR_MISS = 0, WG_FLAG_SPILL = 1, WG_NFLAGS = 4 };
// words of a global row: fwd[3] | rev[3] | sum1[3] | sum2[6] (00 01 02 11 12 22), all in MEMORY-axis order
constexpr int WG_ROW = 15;

struct WallGeoArgs {
    const void* vol;             // labels, dense C-ordered [n0][n1][n2] (u16 or u32; the rank copy of a compacted context)
    int64_t n0, n1, n2;          // buffer dims; n0 counts the halo plane when first_owned == 1
    int32_t first_owned;         // 0, or 1 when plane 0 is the low halo of a slab
    int64_t origin0;             // global coordinate of buffer plane 0 along memory axis 0 (a0_origin - first_owned)
    const uint64_t* hkeys;       // pair -> row hash of the sorted pair list: keys lo << 32 | hi, EMPTY_KEY when free
    const uint32_t* hrows;       // ... and the row of each key
    uint32_t hmask;              // capacity - 1
    unsigned long long* rows;    // [npairs][WG_ROW], zeroed by the caller
    uint32_t* flags;             // [WG_NFLAGS], zeroed by the caller
    uint32_t tiles_per_group;    // (set by launch_wallgeo)
};

// one streaming pass over the labels; the pair -> row table is launch_signal_hash's (ta_signal.h)
// Returns the plan it launched.
RangePlan launch_wallgeo(hipStream_t s, WallGeoArgs a, int label_itemsize);

}  // namespace ta
