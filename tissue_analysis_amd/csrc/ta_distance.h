// ta_distance.h -- launchers of kernels_distance.hip: the exact squared Euclidean distance of every voxel of the resident label
// volume to its nearest site (include/tissue_scan_distance.h), one pass per memory axis, and the per-label table of it.
#pragma once
#include "ta_device.h"
#include "ta_separable.h"

namespace ta {

constexpr uint32_t DIST_EDGE_IS_SITE = 1u;
enum { DIST_FLAG_RANGE = 0, DIST_NFLAGS = 4 };
constexpr uint64_t DIST_WORK_CAP = 1ull << 30;      // bytes of the column passes' envelope stacks, unless one wave of columns needs more
constexpr uint64_t DIST_STACK_ENTRY = 20;           // bytes of an envelope entry: position i32 | f f64 | left boundary f64
constexpr uint64_t DIST_NO_POLE = ~0ull;
// workgroups at most of the kernels that stride over their items: the row pass (four rows a workgroup at a time), the extremes
// and pole kernels (256 voxels), the table initialisation (256 rows)
constexpr uint32_t DIST_ROW_MAX_GROUPS = 1u << 16, DIST_VOXEL_MAX_GROUPS = 1u << 14, DIST_INIT_MAX_GROUPS = 1u << 12;

struct DistanceArgs {
    const void* vol;             // labels (ranks in a compacted context), dense C-ordered [n0][n1][n2] (u16 or u32)
    int64_t n0, n1, n2;          // buffer dims, memory axes
    double* d2;                  // [n0 * n1 * n2]
    double w[3];                 // spacing of memory axis k
    int32_t mode;                // 0: a voxel's class is its label; 1: its class is (label == site)
    uint32_t site, has_site;     // mode 1: the site label as the volume stores it; has_site = 0: no voxel is a site
    uint32_t flags;              // DIST_EDGE_IS_SITE
};

// Row pass along memory axis 2: d2 = (w2 * distance to the nearest end of the voxel's run)^2, +inf where neither end has a site
// behind it; 0 on the site voxels of mode 1.  One wave per row, 64 voxels at a time, forwards and then backwards.  Returns its
// workgroups.
uint32_t launch_distance_rows(hipStream_t s, const DistanceArgs& a, int itemsize);

// Column pass along memory axis `axis` (1 or 0), in place on d2: per run of equal class the lower envelope of the run's own
// parabolas and of a zero parabola on the voxel behind either end.  One lane per column; `columns` of them from `first` per launch.
// The stack of a column lies in `work`: f f64[len][stride] | boundaries f64[len][stride] | positions i32[len][stride], len = the
// axis' length, stride = the columns of a batch (DIST_STACK_ENTRY bytes per entry and column).  Geometry and batches: ta_separable.h.
void launch_distance_columns(hipStream_t s, const DistanceArgs& a, int itemsize, int axis, uint64_t first, uint64_t columns, void* work,
                             uint64_t stride);

struct DistanceTable {
    unsigned long long* min2;    // [R] bit patterns of non-negative doubles; starts at +inf
    unsigned long long* max2;    // [R] starts at 0
    unsigned long long* pole;    // [R] the smallest array-order index among the voxels at max2; DIST_NO_POLE for a label without voxels
    uint32_t* flags;             // [DIST_NFLAGS]
    uint32_t max_label;
    uint64_t key_stride[3];      // of memory axis k in the C order of the ARRAY axes
};
// the rows set to their starting values, then two streaming passes over labels and d2: the extremes, then the pole; their
// workgroups go to launched.init_groups and launched.voxel_groups
void launch_distance_table(hipStream_t s, const DistanceArgs& a, int itemsize, const DistanceTable& t, DistanceLaunch& launched);

}  // namespace ta
