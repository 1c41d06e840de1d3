// ta_topology.h -- launcher of kernels_topology.hip: the twelve block counts per label behind the Euler numbers of the resident
// label volume (include/tissue_scan_topology.h).
#pragma once
#include "ta_device.h"

namespace ta {

// flag words of the pass (device u32[TP_NFLAGS], zeroed before every pass)
enum { TP_FLAG_RANGE = 0, TP_FLAG_SPILL = 1, TP_NFLAGS = 4 };
constexpr int TP_SLOTS = 768;                       // rows of a workgroup's LDS table (_capi.TOPOLOGY_SLOTS): 52 bytes each, four workgroups a CU
constexpr int64_t TP_MAX_GROUPS = 1024;             // workgroups of the pass at most: four a CU, all resident at once

struct TopologyArgs {
    const void* vol;             // labels, dense C-ordered [n0][n1][n2] (u16 or u32; the rank copy of a compacted context)
    int64_t n0, n1, n2;          // buffer dims
    uint32_t max_label;          // rows 0 .. max_label
    unsigned long long* n0c;     // [max_label + 1]
    unsigned long long* n1c;     // [max_label + 1][3]
    unsigned long long* n2c;     // [max_label + 1][3]
    unsigned long long* n3c;     // [max_label + 1]
    unsigned long long* vc;      // [max_label + 1]
    unsigned long long* ec;      // [max_label + 1][3]
    unsigned long long* mixed;   // blocks that held more than one label
    uint32_t* flags;             // [TP_NFLAGS]
    uint32_t tiles_per_group;    // (set by launch_topology)
};

// The launch plan for these buffer dims: tiles over the block positions [0, n0] x [0, n1] x [0, n2) (kernels_topology.hip).
RangePlan topology_plan(const int64_t dims[3], int label_itemsize);
// one pass over the blocks of the volume.  The rows, the mixed word and the flags must be zero.
void launch_topology(hipStream_t s, TopologyArgs a, int label_itemsize, const RangePlan& plan);

}  // namespace ta
