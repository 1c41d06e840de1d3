// ta_nearest.h -- launchers of kernels_nearest.hip: for every voxel of the resident label volume the exact squared Euclidean distance
// to the nearest site and the smallest label among the sites at that distance (include/tissue_scan_nearest.h), one pass per memory
// axis, then the counts of the empty voxels every label gains and the pass that writes them into the volume.
#pragma once
#include "ta_device.h"
#include "ta_separable.h"

namespace ta {

constexpr uint32_t NEAR_NONE = 0xFFFFFFFFu;         // no label: of a voxel without a site, and of an envelope entry without a boundary label
enum { NEAR_FLAG_RANGE = 0, NEAR_NFLAGS = 4 };
constexpr uint64_t NEAR_WORK_CAP = 1ull << 30;      // bytes of the column passes' envelope stacks, unless one wave of columns needs more
constexpr uint64_t NEAR_STACK_ENTRY = 28;           // bytes of an envelope entry: f f64 | left boundary f64 | position i32 | label u32 | boundary label u32
// workgroups at most of the kernels that stride over their items: the row pass (four rows a workgroup at a time), the counting and
// the apply pass (256 voxels)
constexpr uint32_t NEAR_ROW_MAX_GROUPS = 1u << 16, NEAR_VOXEL_MAX_GROUPS = 1u << 14;

struct NearestArgs {
    const void* vol;             // labels (ranks in a compacted context), dense C-ordered [n0][n1][n2] (u16 or u32)
    int64_t n0, n1, n2;          // buffer dims, memory axes
    double* f;                   // [n0 * n1 * n2] D2
    uint32_t* lab;               // [n0 * n1 * n2] N, as the volume stores labels
    double w[3];                 // spacing of memory axis k
    double max_d2;               // an empty voxel is filled when D2 <= max_d2 (and there is a site)
    uint32_t empty, has_empty;   // the empty label as the volume stores it; has_empty = 0: no voxel is empty
    uint32_t not_from, has_not_from;     // likewise the label whose voxels are neither sites nor filled
};

// Row pass along memory axis 2: f = (w2 * distance to the nearest site of the row)^2 and lab = its label, the smaller one where the
// site to the left and the site to the right are equally far; +inf and NEAR_NONE in a row without a site.  One wave per row, 64
// voxels at a time, forwards and then backwards.  Returns its workgroups.
uint32_t launch_nearest_rows(hipStream_t s, const NearestArgs& a, int itemsize);

// Column pass along memory axis `axis` (1 or 0), in place on f and lab: the lower envelope of the parabolas f(v) + w^2 (i - v)^2 of
// the column, with the smallest label where several parabolas are lowest.  One lane per column; `columns` of them from `first` per
// launch.  The stack of a column lies in `work`: f f64[len][stride] | boundaries f64[len][stride] | positions i32[len][stride] |
// labels u32[len][stride] | boundary labels u32[len][stride], len = the axis' length, stride = the columns of a batch
// (NEAR_STACK_ENTRY bytes per entry and column).  Geometry and batches: ta_separable.h.
void launch_nearest_columns(hipStream_t s, const NearestArgs& a, int axis, uint64_t first, uint64_t columns, void* work, uint64_t stride);

struct NearestTable {
    unsigned long long* gained;  // [R] filled voxels by the label they take; starts at 0
    unsigned long long* totals;  // [2] filled voxels | empty voxels left unfilled
    uint32_t* flags;             // [NEAR_NFLAGS]
    uint32_t max_label;
};
// workgroups of the two kernels that stream over the voxels
uint32_t nearest_voxel_groups(const NearestArgs& a);
// one streaming pass over labels, f and lab: the counts of the (zeroed) table.  Returns its workgroups.
uint32_t launch_nearest_count(hipStream_t s, const NearestArgs& a, int itemsize, const NearestTable& t);
// one streaming pass: vol[p] = lab[p] where p is filled.  In a compacted context `ranks` is the rank copy (it gets lab[p]) and `vol`
// gets ids[lab[p]] (nids of them); else ranks and ids are NULL.  Returns its workgroups.
uint32_t launch_nearest_apply(hipStream_t s, const NearestArgs& a, int itemsize, void* vol, void* ranks, const uint32_t* ids, uint32_t nids);

}  // namespace ta
