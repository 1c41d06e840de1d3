// ta_range_plan.h -- the launch plan of the range passes: kernels_signal, _overlap, _wallgeo, _profile, _sighist, _sigmoments, _extents.hip
// and, over block positions, kernels_topology.hip (plain host C++, no HIP).  A tile is `waves` rows x (64 lanes x VPL columns) x `planes` planes, VPL = 16 / sizeof(label) voxels a
// lane; a workgroup takes `tiles_per_group` consecutive tiles (column blocks first, then row blocks, then plane blocks) and keeps
// its LDS tables for the whole range.  Each kernel file states its RangeShape; tests/range_tiles.py restates the arithmetic, once.
#pragma once
#include <stdint.h>

#include <initializer_list>

namespace ta {

// What a range pass launched: every workgroup takes `tiles_per_group` consecutive tiles (the last one what is left); 0, 0 when there
// was nothing to launch.  The host layer keeps it for the ta_*_debug getters.
struct RangePlan { uint32_t tiles_per_group = 0, groups = 0; };
// voxel_cap_log2: a workgroup walks at most 2^cap voxels (its LDS counters are u32)
struct RangeShape { int waves, planes; int64_t max_groups; int voxel_cap_log2; };
// column, row and plane blocks of the owned planes of a buffer, their product, the voxels of a tile; all 0 for an empty volume
struct RangeTiles { int64_t ncb = 0, nrb = 0, npb = 0, tiles = 0, tile_voxels = 0; };

inline RangeTiles range_tiles(int64_t n0, int64_t n1, int64_t n2, int64_t first_owned, int label_itemsize, const RangeShape& shape) {
    const int64_t cols = 64 * (16 / label_itemsize), owned = n0 - first_owned;
    RangeTiles t;
    if (owned <= 0 || n1 <= 0 || n2 <= 0) return t;
    t.ncb = (n2 + cols - 1) / cols;
    t.nrb = (n1 + shape.waves - 1) / shape.waves;
    t.npb = (owned + shape.planes - 1) / shape.planes;
    t.tiles = t.ncb * t.nrb * t.npb;
    t.tile_voxels = shape.waves * cols * shape.planes;
    return t;
}

// per = min(ceil(tiles / max_groups), 2^cap / tile_voxels, extra_most); 0, 0 without tiles, or when not even one tile is allowed
inline RangePlan plan_ranges(int64_t tiles, int64_t tile_voxels, const RangeShape& shape, int64_t extra_most = INT64_MAX) {
    RangePlan plan;
    int64_t most = tiles > 0 ? ((int64_t)1 << shape.voxel_cap_log2) / tile_voxels : 0;
    if (extra_most < most) most = extra_most;
    if (most <= 0) return plan;
    int64_t per = (tiles + shape.max_groups - 1) / shape.max_groups;
    if (per > most) per = most;
    plan.tiles_per_group = (uint32_t)per;
    plan.groups = (uint32_t)((tiles + per - 1) / per);
    return plan;
}

// The vector loads: rows are whole strips of VPL items, and every buffer is aligned to its strip, or to 16 bytes (one load) where
// the strip is longer.  itemsize 0: a buffer the pass does not read.
struct StripBuffer { const void* p; int itemsize; };
inline bool strips_vectorize(int64_t n2, int label_itemsize, std::initializer_list<StripBuffer> buffers) {
    const int vpl = 16 / label_itemsize;
    for (const StripBuffer& b : buffers) {
        const int strip = vpl * b.itemsize;
        if (strip && (uintptr_t)b.p % (uintptr_t)(strip < 16 ? strip : 16)) return false;
    }
    return n2 % vpl == 0;
}

}  // namespace ta
