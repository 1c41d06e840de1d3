// ta_overlap.h -- launchers of kernels_overlap.hip: the label-overlap table between the resident label volume A and a second
// label volume B of the same grid (include/tissue_scan_overlap.h).
#pragma once
#include "ta_device.h"

namespace ta {

// flag words of the overlap pass (device u32[OV_NFLAGS], zeroed before every pass)
enum { OV_FLAG_OVERFLOW = 0, OV_FLAG_LDS_SPILL = 1, OV_NFLAGS = 4 };

struct OverlapArgs {
    const void* a;               // labels A, dense C-ordered [n0][n1][n2] (u16 or u32), the ids as the caller stored them
    const void* b;               // labels B, same buffer dims (u16 or u32)
    int64_t n0, n1, n2;          // buffer dims; n0 counts the halo plane when first_owned == 1
    int32_t first_owned;         // 0, or 1 when plane 0 is the low halo of a slab
    unsigned long long* keys;    // [mask + 1] device-global open-addressed table: a << 32 | b, EMPTY_KEY when free
    unsigned long long* counts;  // [mask + 1] voxels of the slot's pair
    uint32_t mask;               // slots - 1 (a power of two)
    uint32_t* flags;             // [OV_NFLAGS]
    unsigned long long* top;     // voxels of the pair (2^32 - 1, 2^32 - 1): its key IS EMPTY_KEY, so it has a counter of its own
    uint32_t tiles_per_group;    // (set by launch_overlap)
};

// one streaming pass over A and B.  keys must hold EMPTY_KEY everywhere (memset 0xff); counts, flags and *top zero.
// Returns the plan it launched.
RangePlan launch_overlap(hipStream_t s, OverlapArgs a, int itemsize_a, int itemsize_b);

// compaction of the occupied slots: count per block of OV_COMPACT_BLOCK slots, (the caller scans the counts,) emit.
constexpr uint32_t OV_COMPACT_BLOCK = 1024;
inline uint64_t overlap_compact_blocks(uint64_t slots) { return (slots + OV_COMPACT_BLOCK - 1) / OV_COMPACT_BLOCK; }
void launch_overlap_count(hipStream_t s, const unsigned long long* keys, uint64_t slots, uint32_t* block_counts);
// sort_keys[i] = a << shift_b | b of the i-th occupied slot (any order inside a block), slot_of[i] = its slot
void launch_overlap_emit(hipStream_t s, const unsigned long long* keys, uint64_t slots, const uint64_t* block_offsets, int shift_b,
                         uint64_t* sort_keys, uint32_t* slot_of);
// the sorted rows: a, b from the sort key, n through the slot; when top != 0 one more row (2^32 - 1, 2^32 - 1, top) behind them
void launch_overlap_rows(hipStream_t s, const uint64_t* sorted_keys, const uint32_t* slot_of, uint64_t n, const unsigned long long* counts,
                         int shift_b, uint64_t top, uint32_t* a_out, uint32_t* b_out, uint64_t* n_out);

}  // namespace ta
