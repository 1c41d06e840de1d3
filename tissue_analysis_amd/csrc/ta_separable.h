// ta_separable.h -- what the two separable transforms (kernels_distance.hip, kernels_nearest.hip) and their host layers share around
// their column passes: the geometry of a pass along memory axis 1 or 0, and the columns of a launch.  Host only, private to csrc/.
#pragma once
#include <algorithm>
#include <cstdint>

namespace ta {

// A column pass along memory axis `axis` (1 or 0) of a dense [n0][n1][n2] volume: column `col` starts at voxel
// (col / inner) * outer_stride + col % inner and walks `len` voxels, `step` apart.
struct ColumnPass {
    int64_t len;
    uint64_t step;
    uint64_t inner;              // columns that lie side by side in memory
    uint64_t outer_stride;       // axis 1: one group of them per plane; axis 0: one group
    uint64_t columns;
};
inline ColumnPass column_pass(int64_t n0, int64_t n1, int64_t n2, int axis) {
    const uint64_t plane = (uint64_t)n1 * (uint64_t)n2;
    if (axis == 1) return {n1, (uint64_t)n2, (uint64_t)n2, plane, (uint64_t)n2 * (uint64_t)n0};
    return {n0, plane, plane, plane, plane};
}
inline uint32_t column_grid(uint64_t columns) { return (uint32_t)((columns + 255) / 256); }      // one lane per column

// workgroups of 256 for a kernel that strides over its items: one at least, `cap` at most
inline uint32_t blocks_for(uint64_t threads, uint32_t cap) {
    const uint64_t b = (threads + 255) / 256;
    return (uint32_t)(b < 1 ? 1 : (b > cap ? cap : b));
}

// columns of a launch of pass g, at entry_bytes of envelope stack per voxel of a column: whole waves; what the option says
// (opt_batch > 0), else what fits work_cap
inline uint64_t batch_columns(const ColumnPass& g, int64_t opt_batch, uint64_t entry_bytes, uint64_t work_cap) {
    const uint64_t b = opt_batch > 0 ? ((uint64_t)opt_batch + 63) / 64 * 64
                                     : std::max<uint64_t>(64, work_cap / ((uint64_t)g.len * entry_bytes) / 64 * 64);
    return std::min(b, (g.columns + 63) / 64 * 64);
}

// ... of both column passes ([0]: along memory axis 1, [1]: along memory axis 0), and the bytes of the stacks of the larger batch
struct BatchPlan { uint64_t batch[2], work; };
inline BatchPlan plan_batches(const int64_t mdims[3], int64_t opt_batch, uint64_t entry_bytes, uint64_t work_cap) {
    BatchPlan p = {{0, 0}, 0};
    for (int k = 0; k < 2; ++k) {
        const ColumnPass g = column_pass(mdims[0], mdims[1], mdims[2], 1 - k);
        p.batch[k] = batch_columns(g, opt_batch, entry_bytes, work_cap);
        p.work = std::max(p.work, (uint64_t)g.len * p.batch[k] * entry_bytes);
    }
    return p;
}

}  // namespace ta
