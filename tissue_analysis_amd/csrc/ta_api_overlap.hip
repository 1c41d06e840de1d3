// ta_api_overlap.hip -- the C ABI of include/tissue_scan_overlap.h on top of kernels_overlap.hip.
#include "../../include/tissue_scan_overlap.h"
#include "ta_ctx.h"
#include "ta_overlap.h"

namespace {

constexpr CompanionKind B_VOLUME = {"B", 2, 4};        // uint16 or uint32
constexpr int OV_MIN_LOG2 = 4, OV_MAX_LOG2 = 31;       // (the sort's values are u32 slot numbers)
const char* const NO_TABLE = "no overlap table for the current volume and B (run ta_overlap_extract)";

// the parts of OverlapState::rows for P pairs
struct OverlapTable {
    Part a, b, n;
    uint64_t bytes = 0;
    constexpr explicit OverlapTable(uint64_t P) {
        PartCursor at;
        a = at.take(4 * P); b = at.take(4 * P); n = at.take(8 * P);
        bytes = at.end() + 16;
    }
};
static_assert(OverlapTable(3).b.at == 12 && OverlapTable(3).n.at == 24 && OverlapTable(3).bytes == 64, "a u32[P] | b u32[P] | n u64[P]");

uint64_t overlap_voxels(const ta_ctx* c) { return (uint64_t)(c->mdims[0] - c->first_owned) * (uint64_t)c->mdims[1] * (uint64_t)c->mdims[2]; }

// the table no pass over this volume can fill: two slots a voxel
int overlap_top_log2(const ta_ctx* c) {
    int l = OV_MIN_LOG2;
    while (l < OV_MAX_LOG2 && (1ull << l) < 2 * overlap_voxels(c)) ++l;
    return l;
}

// the automatic table: a slot per 512 voxels (two Voronoi frames hold a pair per ~3000 voxels), 2^16 .. 2^24 slots
int overlap_auto_log2(const ta_ctx* c) {
    int l = 16;
    while (l < 24 && (1ull << l) < overlap_voxels(c) / 512) ++l;
    return l;
}

// clear a table of 2^ov_log2 slots and enqueue the pass, then the count and the scan of its occupied slots
int overlap_launch(ta_ctx* c) {
    const uint64_t slots = 1ull << c->ov.log2, blocks = ta::overlap_compact_blocks(slots);
    int rc;
    if ((rc = c->ov.table.reserve(slots * 16)) != TA_OK) return rc;
    if ((rc = c->ov.small.reserve(32)) != TA_OK) return rc;
    const ScanBlock wl(blocks);                    // OverlapState::work: the occupied slots of the blocks of the table
    if ((rc = c->ov.work.reserve(wl.end)) != TA_OK) return rc;
    if ((rc = ensure_events(c->ov.ev)) != TA_OK) return rc;
    ta::OverlapArgs a;
    a.a = c->vol;                  // (the ids as the caller stored them: never the rank copy of a compacted context)
    a.b = c->ov.b.p;
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.first_owned = c->first_owned;
    a.keys = (unsigned long long*)c->ov.table.p;
    a.counts = a.keys + slots;
    a.mask = (uint32_t)(slots - 1);
    a.flags = (uint32_t*)c->ov.small.p;
    a.top = (unsigned long long*)((char*)c->ov.small.p + 16);
    a.tiles_per_group = 0;
    TA_HIP(hipMemsetAsync(a.keys, 0xff, slots * 8, c->stream));
    TA_HIP(hipMemsetAsync(a.counts, 0, slots * 8, c->stream));
    TA_HIP(hipMemsetAsync(c->ov.small.p, 0, 32, c->stream));
    TA_HIP(hipEventRecord(c->ov.ev[0], c->stream));
    c->ov.plan = ta::launch_overlap(c->stream, a, c->itemsize, c->ov.b.itemsize);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->ov.ev[1], c->stream));
    ta::launch_overlap_count(c->stream, a.keys, slots, wl.counts(c->ov.work.p));
    wl.scan(c->stream, c->ov.work.p);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->ov.ev[2], c->stream));
    c->ov.passes += 1;
    return TA_OK;
}

// drain the stream; a table that overflowed is grown and the pass repeated; then the occupied slots become the sorted rows
int overlap_settle(ta_ctx* c) {
    if (c->ov.state == 2) return TA_OK;
    if (c->ov.state != 1) return fail(TA_EINVAL, NO_TABLE);
    int rc;
    uint64_t occupied = 0, top = 0;
    for (;;) {
        const uint64_t blocks = ta::overlap_compact_blocks(1ull << c->ov.log2);
        uint32_t small[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        TA_HIP(hipMemcpyAsync(small, c->ov.small.p, sizeof(small), hipMemcpyDeviceToHost, c->stream));
        TA_HIP(ScanBlock(blocks).read_total(c->stream, c->ov.work.p, &occupied));
        TA_HIP(hipStreamSynchronize(c->stream));
        memcpy(&top, &small[4], 8);
        c->ov.lds_spills = small[ta::OV_FLAG_LDS_SPILL];               // (of the run just read: in the end, of the last one)
        if (!small[ta::OV_FLAG_OVERFLOW]) break;
        const int most = overlap_top_log2(c);
        if (c->ov.log2 >= most) {
            c->ov.state = 0;
            return fail(TA_ENOMEM, "the overlap table overflowed at its largest size (2^%d slots)", c->ov.log2);
        }
        c->ov.log2 = std::min(c->ov.log2 + 3, most);
        if (!c->ov.opt_log2) c->ov.grown_log2 = c->ov.log2;
        if ((rc = overlap_launch(c)) != TA_OK) { c->ov.state = 0; return rc; }
    }
    const uint64_t slots = 1ull << c->ov.log2, blocks = ta::overlap_compact_blocks(slots);
    const uint64_t P = occupied + (top ? 1 : 0);
    const uint64_t n = occupied;
    const SortLayout S(n, 8);
    const OverlapTable tb(P);
    if ((rc = c->ov.sort.reserve(S.end + 16)) != TA_OK) return rc;
    if ((rc = c->ov.rows.reserve(tb.bytes)) != TA_OK) return rc;
    SortView<uint64_t> v(S, c->ov.sort.p);
    const unsigned long long* keys = (const unsigned long long*)c->ov.table.p;
    const int shift_b = 8 * c->ov.b.itemsize;
    TA_HIP(hipEventRecord(c->ov.ev[3], c->stream));
    ta::launch_overlap_emit(c->stream, keys, slots, ScanBlock(blocks).offsets(c->ov.work.p), shift_b, v.keys(), v.idx());
    TA_HIP(v.sort(c->stream, n, 8 * c->itemsize + shift_b));
    char* rp = (char*)c->ov.rows.p;
    ta::launch_overlap_rows(c->stream, v.keys(), v.idx(), n, keys + slots, shift_b, top, (uint32_t*)(rp + tb.a.at), (uint32_t*)(rp + tb.b.at), (uint64_t*)(rp + tb.n.at));
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->ov.ev[4], c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    c->ov.npairs = P;
    c->ov.state = 2;
    return TA_OK;
}

// the checks every function behind the extract shares; settles
int overlap_ready(ta_ctx* c) {
    const int rc = results_ready(c, [](const ta_ctx* c) { return c->ov.state != 0; }, NO_TABLE);
    return rc != TA_OK ? rc : overlap_settle(c);
}

}  // namespace

// a new label volume (or new label values in it): the overlap table is stale; a B of other dims is dropped
void overlap_on_new_volume(ta_ctx* c) {
    c->ov.state = 0;
    c->ov.grown_log2 = 0;
    companion_on_new_volume(c, c->ov.b);
}

// the resample pass rewrites (or has moved) the buffer B was adopted from: the table is stale, a B that is gone is dropped
void overlap_on_resampled(ta_ctx* c, const void* buf, const void* now, int itemsize) {
    if (!buf || c->ov.b.p != buf || c->ov.b.owned.p) return;
    c->ov.state = 0;
    if (now != buf || itemsize != c->ov.b.itemsize) { c->ov.b.p = nullptr; c->ov.b.itemsize = 0; }
}

extern "C" {

TA_API int ta_overlap_set(ta_ctx* c, const void* host_ptr, int itemsize, const int64_t dims[3], const int64_t strides_bytes[3]) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    const int rc = companion_set_host(c, c->ov.b, B_VOLUME, host_ptr, itemsize, dims, strides_bytes);
    if (rc == TA_OK || !c->ov.b.p) c->ov.state = 0;      // (also when the upload failed and left no B -- a table implies a B: deliberate, as inherited)
    return rc;
}

TA_API int ta_overlap_set_device(ta_ctx* c, const void* dev_ptr, int itemsize) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    const int rc = companion_set_device(c, c->ov.b, B_VOLUME, dev_ptr, itemsize);
    if (rc == TA_OK) c->ov.state = 0;
    return rc;
}

TA_API int ta_overlap_set_capacity(ta_ctx* c, int log2_slots) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (log2_slots != 0 && (log2_slots < OV_MIN_LOG2 || log2_slots > OV_MAX_LOG2))
        return fail(TA_EINVAL, "the overlap table takes 2^%d .. 2^%d slots, or 0 for an automatic size", OV_MIN_LOG2, OV_MAX_LOG2);
    c->ov.opt_log2 = log2_slots;
    c->ov.grown_log2 = 0;
    return TA_OK;
}

TA_API int ta_overlap_extract(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->vol) return fail(TA_EINVAL, "no label volume set");
    if (!c->ov.b.p) return fail(TA_EINVAL, "no second label volume set (ta_overlap_set)");
    if (!companion_matches(c, c->ov.b)) return fail(TA_EINVAL, "B does not match the label volume");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    c->ov.state = 0;
    c->ov.passes = 0;
    c->ov.log2 = c->ov.opt_log2 ? c->ov.opt_log2 : std::max(overlap_auto_log2(c), c->ov.grown_log2);
    if ((rc = overlap_launch(c)) != TA_OK) return rc;
    c->ov.state = 1;
    return TA_OK;
}

TA_API int ta_overlap_size(ta_ctx* c, uint64_t* npairs) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!npairs) return fail(TA_EINVAL, "NULL argument");
    const int rc = overlap_ready(c);
    if (rc == TA_OK) *npairs = c->ov.npairs;
    return rc;
}

TA_API int ta_overlap_get(ta_ctx* c, uint32_t* a, uint32_t* b, uint64_t* n) {
    const int rc = overlap_ready(c);
    if (rc != TA_OK || !c->ov.npairs) return rc;
    const OverlapTable tb(c->ov.npairs);
    return read_columns(c, c->ov.rows.p, {{a, tb.a}, {b, tb.b}, {n, tb.n}});
}

TA_API int ta_overlap_debug(ta_ctx* c, uint32_t out[4]) {
    const int rc = overlap_ready(c);
    if (rc == TA_OK) range_debug_words(out, c->ov.lds_spills, (uint32_t)c->ov.passes, c->ov.plan);
    return rc;
}

TA_API int ta_overlap_timing(ta_ctx* c, double* ms) {
    return pass_timing(c, ms, [](ta_ctx* c) { return c->ov.state != 0 && c->ov.ev[1] ? c->ov.ev : nullptr; }, "no overlap pass has been run");
}

TA_API int ta_overlap_timing_compaction(ta_ctx* c, double* ms, int* passes) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!ms) return fail(TA_EINVAL, "NULL argument");
    if (c->ov.state != 2) return fail(TA_EINVAL, "no settled overlap table (ask ta_overlap_size first)");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    hipEvent_t* ev = c->ov.ev;
    TA_HIP(summed_ms(ev[4], {{ev[1], ev[2]}, {ev[3], ev[4]}}, ms));
    if (passes) *passes = c->ov.passes;
    return TA_OK;
}

}  // extern "C"
