// ta_sighist.h -- launchers of kernels_sighist.hip: per-label histograms of the signal image and the radix select of order
// statistics over them (include/tissue_scan_sighist.h).
#pragma once
#include "ta_device.h"

namespace ta {

// flag words of one digit pass (device u32[SH_NFLAGS], zeroed before the pass)
enum { SH_FLAG_RANGE = 0, SH_FLAG_SPILL = 1, SH_NFLAGS = 4 };
// (macros so that scripts/build_variant.py can build other tables and plans with -D: DESIGN.md 4.14 has what was measured)
#ifndef TA_SH_SLOTS
#define TA_SH_SLOTS 39
#endif
#ifndef TA_SH_MAX_GROUPS
#define TA_SH_MAX_GROUPS 65536
#endif
constexpr int SH_SLOTS = TA_SH_SLOTS;               // rows of 256 counters in a workgroup's LDS table (_capi.SIGHIST_SLOTS)
constexpr int64_t SH_MAX_GROUPS = TA_SH_MAX_GROUPS; // workgroups of the digit pass at most (_capi.SIGHIST_MAX_GROUPS)
constexpr int SH_MAX_RANKS = 8;                     // ranks a row of one ta_sigrank_extract
constexpr uint32_t SH_NONE = 0xffffffffu;           // no selector / no value

struct DigitArgs {
    const void* vol;             // labels, dense C-ordered [n0][n1][n2] (u16 or u32; the rank copy of a compacted context)
    const void* sig;             // signal, same buffer dims (u8 or u16)
    int64_t n0, n1, n2;          // buffer dims; n0 counts the halo plane when first_owned == 1
    int32_t first_owned;         // 0, or 1 when plane 0 is the low halo of a slab
    uint32_t max_label;          // rows 0 .. max_label
    uint32_t shift;              // digit = (S >> shift) & 255
    uint32_t stride;             // counters of a key in `counts`: the bins of a histogram, 256 for a select
    uint32_t nsel;               // 0: every voxel counts, key = row.  Else key = row * nsel + j for the j with S >> (shift + 8) == sel[key]
    const uint32_t* sel;         // [rows][nsel] selectors (SH_NONE: none), written by the select kernel before
    unsigned long long* counts;  // [keys][stride]
    uint32_t* flags;             // [SH_NFLAGS]
    uint32_t tiles_per_group;    // (set by launch_sighist_digits)
};

// one streaming pass over labels + signal.  counts and flags must be zero.  Returns the plan it launched.
RangePlan launch_sighist_digits(hipStream_t s, DigitArgs a, int label_itemsize, int signal_itemsize);

struct SelectArgs {
    uint32_t rows, nranks;
    const unsigned long long* ranks;    // [rows][nranks] wanted 0-based ranks
    const unsigned long long* counts1;  // [rows][256] digits of the first pass (the only one of a uint8 signal)
    const unsigned long long* counts2;  // [rows][nranks][256] low digits under each selector (uint16)
    unsigned long long* rem;            // [rows][nranks] the rank inside the chosen high byte
    uint32_t* hi;                       // [rows][nranks] the chosen high byte, SH_NONE: rank >= n
    uint32_t* sel;                      // [rows][nranks] the distinct high bytes of a row, each at its first j; SH_NONE elsewhere
    uint32_t* map;                      // [rows][nranks] the j whose selector holds rank j's high byte
    uint32_t* values;                   // [rows][nranks] the order statistics
};

// one wave a row.  first: from counts1 and ranks; final = the digit is the value (uint8), else hi, rem, sel and map are written.
void launch_sighist_select_first(hipStream_t s, const SelectArgs& a, bool final);
// from counts2, rem, hi and map: values = hi << 8 | low digit
void launch_sighist_select_second(hipStream_t s, const SelectArgs& a);

}  // namespace ta
