// ta_components.h -- launchers of kernels_components.hip: the face-connected components of equal label of the resident label
// volume (include/tissue_scan_components.h) by a block-based union-find, their statistics, and the row image.
#pragma once
#include "ta_device.h"

namespace ta {

// the tile of the local pass, in voxels per memory axis (planes x rows x columns): one workgroup resolves one tile in LDS
constexpr int CC_TILE_PLANES = 4, CC_TILE_ROWS = 4, CC_TILE_COLS = 256;
constexpr uint32_t CC_SLOT_FLAG = 0x80000000u;      // parent[root] = CC_SLOT_FLAG | slot once the slots are handed out
constexpr uint32_t CC_NO_ROW = 0xFFFFFFFFu;         // row image: a voxel of a component without an owned voxel
constexpr uint64_t CC_MAX_VOXELS = 1ull << 31;      // buffer voxels (halo included): an index and a flagged slot share a word
constexpr uint32_t CC_SEAM_MAX_GROUPS = 1u << 18;   // workgroups of the seam pass at most: one takes every CC_SEAM_MAX_GROUPS-th row
constexpr uint32_t CC_STREAM_MAX_GROUPS = 65536;    // ... of the key, row, image and relabel kernels, which stride over their items

struct ComponentArgs {
    const void* vol;             // labels, dense C-ordered [n0][n1][n2] (u16 or u32), the ids as the caller stored them
    int64_t n0, n1, n2;          // buffer dims (connectivity runs over all of them, the halo plane included)
    uint32_t* parent;            // [n0 * n1 * n2] buffer-linear index of a voxel of the same component, never a larger one
};

// tiles of the local pass (= its workgroups)
uint64_t component_tiles(const ComponentArgs& a);
// local pass: every tile's components in LDS; parent[v] = the smallest voxel of v's component INSIDE its tile
void launch_component_local(hipStream_t s, const ComponentArgs& a, int itemsize);
// seam pass: the pairs of equal label across tile faces, united in `parent` by agent-scope atomics.  Returns its workgroups.
uint32_t launch_component_seams(hipStream_t s, const ComponentArgs& a, int itemsize);

// a wave of the flatten / emit kernels holds 256 consecutive voxels
inline uint64_t component_waves(uint64_t nvox) { return ((nvox + 1023) / 1024) * 4; }
// parent[v] = root of v (the voxels the seam pass linked out of their tile first: two launches); wave_counts[w] = roots among
// the wave's voxels.  n1, n2: rows and columns of the buffer
void launch_component_flatten(hipStream_t s, uint32_t* parent, uint64_t nvox, int64_t n1, int64_t n2, uint32_t* wave_counts);
// the roots take the slots wave_offsets[w] .. in voxel order: parent[root] = CC_SLOT_FLAG | slot, root_of_slot[slot] = root
void launch_component_emit(hipStream_t s, uint32_t* parent, uint64_t nvox, const uint64_t* wave_offsets, uint32_t* root_of_slot);

// per slot, over the OWNED voxels, in memory axes and buffer coordinates
struct ComponentStats {
    unsigned long long* n;       // [S]     zeroed by the caller
    unsigned long long* sum1;    // [S][3]  zeroed by the caller
    unsigned long long* first;   // [S]     all bits set by the caller; the smallest array-order index (see key_stride)
    int32_t* box;                // [S][6]  every byte 0x7F by the caller; min0, min1, min2, -max0, -max1, -max2
};
struct ComponentGeometry {
    uint64_t nvox, own_begin;    // voxels of the buffer; the first owned one (the halo plane lies in front of it)
    uint32_t n1, n2;
    uint64_t key_stride[3];      // of memory axis k in the C order of the ARRAY axes: the key of (q, r, c) is their weighted sum
};
void launch_component_stats(hipStream_t s, const uint32_t* parent, const ComponentGeometry& g, const ComponentStats& t);

// sort keys of the slots: label << 32 | first for a slot with owned voxels (counted in *nonempty, zeroed by the caller), all
// bits set for the others, which therefore sort behind every row; index_out[i] = i.  Returns its workgroups.
uint32_t launch_component_keys(hipStream_t s, const void* vol, int itemsize, const uint32_t* root_of_slot, const ComponentStats& t, uint64_t nslots,
                               uint64_t* keys_out, uint32_t* index_out, unsigned long long* nonempty);

struct ComponentRows {
    uint32_t* label;             // [R]
    unsigned long long* n;       // [R]
    int32_t* first;              // [R][3] array axes
    int32_t* bbox;               // [R][6] array axes: min, max + 1
    unsigned long long* sum1;    // [R][3] array axes
    int64_t dims[3];             // of the ARRAY axes, to take the key of `first` apart
    int64_t origin0;             // global coordinate of buffer plane 0 along memory axis 0
    int32_t axis[3];             // array axis of memory axis k
};
// order[i]: the slot at sorted position i; the first *nonempty positions become rows, and row_of_slot the inverse (CC_NO_ROW
// for the slots behind them)
void launch_component_rows(hipStream_t s, const void* vol, int itemsize, const uint32_t* root_of_slot, const ComponentStats& t,
                           const uint32_t* order, uint64_t nslots, const unsigned long long* nonempty, uint32_t* row_of_slot,
                           const ComponentRows& rows);

// rows_out[i] = row of voxel first + i.  This one and the next return their workgroups.
uint32_t launch_component_image(hipStream_t s, const uint32_t* parent, const uint32_t* row_of_slot, uint64_t first, uint64_t count, uint32_t* rows_out);
// vol[v] = new_label[row of v] for every voxel that has a row
uint32_t launch_component_relabel(hipStream_t s, const uint32_t* parent, const uint32_t* row_of_slot, uint64_t nvox, const uint32_t* new_label,
                                  void* vol, int itemsize);

}  // namespace ta
