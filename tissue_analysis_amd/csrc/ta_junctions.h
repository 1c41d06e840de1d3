// ta_junctions.h -- launchers of kernels_junctions.hip: the 2 x 2 x 2 blocks of the resident label volume that hold three or four
// distinct labels (include/tissue_scan_junctions.h), as records, and the reduction of the sorted records into the tables.
#pragma once
#include "ta_device.h"

namespace ta {

struct JunctionArgs {
    const void* vol;             // labels, dense C-ordered [n0][n1][n2] (u16 or u32), the ids as the caller stored them
    int64_t n0, n1, n2;          // buffer dims (a halo plane is a plane like the others: it only ever is a block's lower plane)
    int64_t b0, b1, b2;          // block origins per memory axis: max(n - 1, 1)            (set by junction_plan)
    int64_t ncb, nrb, npb;       // tasks per memory axis: one wave walks one task          (set by junction_plan)
    // counting walk: out
    uint32_t* wave_counts3;      // [waves] blocks of order 3 of the wave's task
    uint32_t* wave_counts4;      // [waves] blocks of order 4
    unsigned long long* degenerate;   // blocks of order >= 5 (zeroed by the caller)
    // emitting walk: in / out (record i of a kind: its labels ascending, and the buffer index of the block's origin)
    const uint64_t* wave_offsets3;
    const uint64_t* wave_offsets4;
    uint32_t* labels3;           // [N3][3]
    uint64_t* origin3;           // [N3]
    uint32_t* labels4;           // [N4][4]
    uint64_t* origin4;           // [N4]
};

// fills the task grid of `a` from its dims; returns the number of waves (= tasks) of a walk
uint64_t junction_plan(JunctionArgs& a, int itemsize);
// one walk over the blocks: emit == false counts per wave, emit == true writes the records at the scanned offsets
void launch_junction_pass(hipStream_t s, const JunctionArgs& a, int itemsize, bool emit);

// sort keys of the records in the order `order` (NULL: 0, 1, 2, ..., which is then also written to index_out): the label
// columns col_hi (< 0: none) and col_lo of a record of K labels, packed as hi << label_bits | lo.  The kernel strides over the
// records behind JN_KEY_MAX_GROUPS workgroups at most; returns its workgroups.
constexpr uint32_t JN_KEY_MAX_GROUPS = 8192;
uint32_t launch_junction_keys(hipStream_t s, const uint32_t* labels, int K, uint64_t n, const uint32_t* order, int col_hi, int col_lo,
                              int label_bits, uint64_t* keys_out, uint32_t* index_out);

// the sorted records order[0 .. n): a record whose labels differ from its predecessor's starts a row
constexpr uint32_t JN_ROW_BLOCK = 256;
inline uint64_t junction_row_blocks(uint64_t n) { return (n + JN_ROW_BLOCK - 1) / JN_ROW_BLOCK; }
// block_counts[b] = rows that start in block b of JN_ROW_BLOCK records (the caller scans them)
void launch_junction_heads(hipStream_t s, const uint32_t* labels, int K, const uint32_t* order, uint64_t n, uint32_t* block_counts);

struct JunctionRows {
    uint32_t* labels;            // [R][K]
    unsigned long long* n;       // [R]    (zeroed by the caller)
    unsigned long long* sums;    // [R][3] (zeroed by the caller), array-axis order
    int64_t n0, n1, n2;          // buffer dims, to take a block's origin apart
    int64_t origin0;             // global coordinate of buffer plane 0 along memory axis 0
    int32_t flat[3];             // memory axis k has one voxel: its position is 0
    int32_t axis[3];             // array axis of memory axis k
};
// the segmented reduce: every record adds (1, position) to its row; the first record of a row writes the row's labels
void launch_junction_reduce(hipStream_t s, const uint32_t* labels, const uint64_t* origins, int K, const uint32_t* order, uint64_t n,
                            const uint64_t* block_offsets, const JunctionRows& rows);

}  // namespace ta
