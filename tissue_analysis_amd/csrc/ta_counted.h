// ta_counted.h -- what the count-then-emit passes share (host only, private to csrc/).  Such a pass counts what it will emit,
// scans the counts, lets the host read one total and size its buffers, emits, radix-sorts and reduces into a table: the cell
// junctions, the label components, the label overlap, the cell meshes, the adjacency pair sort, the wall starts.  Two formats are
// stated here and nowhere else: the count/scan block (ScanBlock) and the workspace of the radix sort (SortLayout, SortView); the
// timings of these passes sum their intervals with summed_ms.  The
// layouts are plain host C++ (tests/native/counted.cpp compiles them on their own, with TA_COUNTED_LAYOUT_ONLY defined); the calls
// that enqueue work need HIP.
#pragma once
#include "ta_parts.h"

namespace ta {

// The exclusive scan of kernels_walls.hip takes SCAN_PER_BLOCK counts a workgroup.  Its scratch: block sums u64[blocks] | total
// u64 | 16 bytes of slack; the sum of all counts is left in the word behind the block sums.
constexpr int SCAN_PER_BLOCK = 2048;   // 256 threads x 8
constexpr uint64_t scan_blocks(uint64_t n) { return (n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK; }
constexpr uint64_t scan_u32_scratch_bytes(uint64_t n) { return (scan_blocks(n) + 1) * 8 + 16; }
constexpr uint64_t scan_u32_total(uint64_t n) { return scan_blocks(n); }      // the word of the scratch that holds the total

uint64_t wall_sort_temp_bytes(uint64_t n);             // kernels_wallsort.hip

}  // namespace ta

#ifndef TA_COUNTED_LAYOUT_ONLY
#include "ta_kernels.h"

#include <initializer_list>

// The timed intervals of such a pass lie on both sides of the host's read of the total: the intervals between the pairs of
// recorded events in `pairs`, summed in list order, once `last` is complete.
struct EventPair { hipEvent_t a, b; };
inline hipError_t summed_ms(hipEvent_t last, std::initializer_list<EventPair> pairs, double* ms) {
    hipError_t e = hipEventSynchronize(last);
    double sum = 0.0;
    for (const EventPair& p : pairs) {
        float t = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, p.a, p.b);
        sum += (double)t;
    }
    if (e == hipSuccess) *ms = sum;
    return e;
}
#endif

// The count/scan block of n counts, from byte `from` of a buffer: counts u32[n] | offsets u64[n] | scan scratch, each from a
// multiple of 16; `end` is where the next part may start.  A kernel writes the counts, scan() turns them into offsets, read_total()
// brings their sum to the host.  n == 0: no scan is launched, nothing on the device is read, the total is 0.
struct ScanBlock {
    uint64_t n = 0, end = 0;
    Part counts_part, offsets_part, scratch_part;
    constexpr explicit ScanBlock(uint64_t n_ = 0, uint64_t from = 0) : n(n_) {
        PartCursor at(from);
        counts_part = at.take(n * 4, 16); offsets_part = at.take(n * 8, 16); scratch_part = at.take(ta::scan_u32_scratch_bytes(n), 16);
        end = at.end(16);
    }
    uint32_t* counts(void* base) const { return (uint32_t*)((char*)base + counts_part.at); }
    const uint64_t* offsets(void* base) const { return (const uint64_t*)((char*)base + offsets_part.at); }
#ifndef TA_COUNTED_LAYOUT_ONLY
    void scan(hipStream_t s, void* base) const {
        ta::launch_scan_u32_exclusive(s, counts(base), n, (char*)base + scratch_part.at, (uint64_t*)((char*)base + offsets_part.at));
    }
    hipError_t read_total(hipStream_t s, void* base, uint64_t* host) const {
        *host = 0;
        return n ? hipMemcpyAsync(host, (const uint64_t*)((char*)base + scratch_part.at) + ta::scan_u32_total(n), 8, hipMemcpyDeviceToHost, s) : hipSuccess;
    }
#endif
};

// The workspace of launch_radix_sort_u32 / _u64 for n records, as byte offsets from `from` (a multiple of 16): keys (of key_bytes) x 2 |
// index u32 x 2 | temp, each from a multiple of 16
struct SortLayout {
    uint64_t keys[2], idx[2], temp, end;
    SortLayout(uint64_t n, int key_bytes, uint64_t from = 0) {
        PartCursor at(from);
        for (auto& k : keys) k = at.take(n * key_bytes, 16).at;
        for (auto& i : idx) i = at.take(n * 4, 16).at;
        temp = at.take(ta::wall_sort_temp_bytes(n), 16).at; end = at.end(16);
    }
};

// ... and its buffers at `base`, for keys of type K (uint32_t or uint64_t).  A kernel writes keys() / idx() (pair 0 of a new view);
// sort() leaves the view at the pair that holds the sorted records, and the other pair is the spare of the next sort.
template <class K> struct SortView {
    K* key_buf[2];
    uint32_t* idx_buf[2];
    void* temp;
    int cur = 0;
    SortView(const SortLayout& l, void* base) : temp((char*)base + l.temp) {
        for (int b = 0; b < 2; ++b) { key_buf[b] = (K*)((char*)base + l.keys[b]); idx_buf[b] = (uint32_t*)((char*)base + l.idx[b]); }
    }
    K* keys() const { return key_buf[cur]; }
    uint32_t* idx() const { return idx_buf[cur]; }
    K* spare_keys() const { return key_buf[cur ^ 1]; }
    uint32_t* spare_idx() const { return idx_buf[cur ^ 1]; }
    void sorted_into(const K* sorted) { if (sorted != keys()) cur ^= 1; }      // a sort left its result in `sorted`
#ifndef TA_COUNTED_LAYOUT_ONLY
    hipError_t sort(hipStream_t s, uint64_t n, int key_bits) {
        K* ks = keys();
        uint32_t* is = idx();
        hipError_t e;
        if constexpr (sizeof(K) == 4) e = ta::launch_radix_sort_u32(s, n, keys(), spare_keys(), idx(), spare_idx(), temp, key_bits, &ks, &is);
        else e = ta::launch_radix_sort_u64(s, n, keys(), spare_keys(), idx(), spare_idx(), temp, key_bits, &ks, &is);
        sorted_into(ks);
        return e;
    }
#endif
};
