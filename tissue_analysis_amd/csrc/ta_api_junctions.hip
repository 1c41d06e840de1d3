// ta_api_junctions.hip -- the C ABI of include/tissue_scan_junctions.h on top of kernels_junctions.hip.
#include "../../include/tissue_scan_junctions.h"
#include "ta_ctx.h"
#include "ta_junctions.h"

namespace {

// where the parts of JunctionState::work lie, for W waves
struct JunctionWork {
    uint64_t counts[2], offsets[2], scratch[2], bytes;
    explicit JunctionWork(uint64_t W) {
        PartCursor at;
        for (auto& p : counts) p = at.take(W * 4, 16).at;
        for (auto& p : offsets) p = at.take(W * 8, 16).at;
        for (auto& p : scratch) p = at.take(ta::scan_u32_scratch_bytes(W), 16).at;
        bytes = at.end(16) + 16;
    }
};

// where the parts of JunctionState::sort[k] lie, for N records
struct JunctionSort {
    SortLayout sort;
    uint64_t counts, offsets, scratch, bytes;
    explicit JunctionSort(uint64_t N) : sort(N, 8) {
        const uint64_t B = ta::junction_row_blocks(N);
        PartCursor at(sort.end);
        counts = at.take(B * 4, 16).at;
        offsets = at.take(B * 8, 16).at;
        scratch = at.take(ta::scan_u32_scratch_bytes(B), 16).at;
        bytes = at.end(16) + 16;
    }
};

// the parts of JunctionState::rows[k], for R rows of K labels
struct JunctionTable {
    Part n, sums, labels;
    uint64_t bytes = 0;
    constexpr JunctionTable(uint64_t R, uint64_t K) {
        PartCursor at;
        n = at.take(R * 8); sums = at.take(R * 24); labels = at.take(R * 4 * K);
        bytes = at.end() + 16;
    }
};
static_assert(JunctionTable(5, 3).sums.at == 40 && JunctionTable(5, 3).labels.at == 160 && JunctionTable(5, 3).bytes == 236, "n [R] | sums [R][3] | labels u32[R][K]");

const char* const NO_TABLES = "no junction tables for the current volume (run ta_junctions_extract)";

ta::JunctionArgs junction_args(ta_ctx* c) {
    ta::JunctionArgs a = {};
    a.vol = c->vol;                // (the ids as the caller stored them: never the rank copy of a compacted context, so that
                                   //  the rows sort by id and need no translation)
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    c->jn.waves = ta::junction_plan(a, c->itemsize);
    const JunctionWork w(c->jn.waves);
    char* p = (char*)c->jn.work.p;
    a.wave_counts3 = (uint32_t*)(p + w.counts[0]); a.wave_counts4 = (uint32_t*)(p + w.counts[1]);
    a.wave_offsets3 = (const uint64_t*)(p + w.offsets[0]); a.wave_offsets4 = (const uint64_t*)(p + w.offsets[1]);
    a.degenerate = (unsigned long long*)c->jn.small.p;
    return a;
}

// drain the stream, read the record counts, allocate, run the emitting walk, sort and reduce the records into the tables
int junctions_settle(ta_ctx* c) {
    if (c->jn.state == 2) return TA_OK;
    if (c->jn.state != 1) return fail(TA_EINVAL, NO_TABLES);
    c->jn.state = 0;                               // (whatever fails below: no tables)
    int rc;
    ta::JunctionArgs a = junction_args(c);
    const JunctionWork w(c->jn.waves);
    char* wp = (char*)c->jn.work.p;
    uint64_t N[2] = {0, 0}, degenerate = 0;
    for (int k = 0; k < 2; ++k)
        TA_HIP(hipMemcpyAsync(&N[k], ta::scan_u32_total(wp + w.scratch[k], c->jn.waves), 8, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipMemcpyAsync(&degenerate, c->jn.small.p, 8, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 2; ++k)
        if (N[k] >= (1ull << 32)) return fail(TA_ENOMEM, "%llu junction records: the sort takes fewer than 2^32", (unsigned long long)N[k]);
    const int K[2] = {3, 4};
    PartCursor rec;                                // JunctionState::rec, each part from a multiple of 16
    const uint64_t org_at[2] = {rec.take(N[0] * 8, 16).at, rec.take(N[1] * 8, 16).at};
    const uint64_t lab_at[2] = {rec.take(N[0] * 12, 16).at, rec.take(N[1] * 16, 16).at};
    if ((rc = c->jn.rec.reserve(rec.end(16) + 16)) != TA_OK) return rc;
    for (int k = 0; k < 2; ++k)
        if ((rc = c->jn.sort[k].reserve(JunctionSort(N[k]).bytes)) != TA_OK) return rc;
    char* rp = (char*)c->jn.rec.p;
    uint64_t* origins[2] = {(uint64_t*)(rp + org_at[0]), (uint64_t*)(rp + org_at[1])};
    uint32_t* labels[2] = {(uint32_t*)(rp + lab_at[0]), (uint32_t*)(rp + lab_at[1])};
    a.origin3 = origins[0]; a.origin4 = origins[1];
    a.labels3 = labels[0]; a.labels4 = labels[1];
    TA_HIP(hipEventRecord(c->jn.ev[3], c->stream));
    if (N[0] || N[1]) ta::launch_junction_pass(c->stream, a, c->itemsize, true);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->jn.ev[4], c->stream));
    // stable sorts over the label columns from last to first, then the rows that start in every block of sorted records
    const int lb = 8 * c->itemsize;
    uint32_t* order[2] = {nullptr, nullptr};
    uint64_t R[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        const uint64_t n = N[k];
        c->jn.key_groups[k] = 0u;
        if (!n) continue;
        const JunctionSort q(n);
        char* sp = (char*)c->jn.sort[k].p;
        uint64_t* k0 = (uint64_t*)(sp + q.sort.keys[0]); uint64_t* k1 = (uint64_t*)(sp + q.sort.keys[1]);
        uint32_t* i0 = (uint32_t*)(sp + q.sort.idx[0]); uint32_t* i1 = (uint32_t*)(sp + q.sort.idx[1]);
        c->jn.key_groups[k] = ta::launch_junction_keys(c->stream, labels[k], K[k], n, nullptr, K[k] - 2, K[k] - 1, lb, k0, i0);
        uint64_t* ks = k0; uint32_t* is = i0;
        TA_HIP(ta::launch_radix_sort_u64(c->stream, n, k0, k1, i0, i1, sp + q.sort.temp, 2 * lb, &ks, &is));
        // the leading columns of the records in that order, into the key buffer the order came out with
        uint64_t* ko = ks == k0 ? k1 : k0; uint32_t* io = is == i0 ? i1 : i0;
        ta::launch_junction_keys(c->stream, labels[k], K[k], n, is, K[k] == 4 ? 0 : -1, K[k] == 4 ? 1 : 0, lb, ks, nullptr);
        uint64_t* ks2 = ks; uint32_t* is2 = is;
        TA_HIP(ta::launch_radix_sort_u64(c->stream, n, ks, ko, is, io, sp + q.sort.temp, K[k] == 4 ? 2 * lb : lb, &ks2, &is2));
        order[k] = is2;
        const uint64_t B = ta::junction_row_blocks(n);
        ta::launch_junction_heads(c->stream, labels[k], K[k], is2, n, (uint32_t*)(sp + q.counts));
        ta::launch_scan_u32_exclusive(c->stream, (const uint32_t*)(sp + q.counts), B, sp + q.scratch, (uint64_t*)(sp + q.offsets));
        TA_HIP(hipGetLastError());
        TA_HIP(hipMemcpyAsync(&R[k], ta::scan_u32_total(sp + q.scratch, B), 8, hipMemcpyDeviceToHost, c->stream));
    }
    TA_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 2; ++k)
        if ((rc = c->jn.rows[k].reserve(JunctionTable(R[k], K[k]).bytes)) != TA_OK) return rc;
    for (int k = 0; k < 2; ++k) {
        if (!N[k]) continue;
        const JunctionSort q(N[k]);
        const JunctionTable tb(R[k], K[k]);
        char* sp = (char*)c->jn.sort[k].p;
        char* op = (char*)c->jn.rows[k].p;
        TA_HIP(hipMemsetAsync(op, 0, tb.labels.at, c->stream));
        ta::JunctionRows rows;
        rows.n = (unsigned long long*)(op + tb.n.at);
        rows.sums = (unsigned long long*)(op + tb.sums.at);
        rows.labels = (uint32_t*)(op + tb.labels.at);
        rows.n0 = c->mdims[0]; rows.n1 = c->mdims[1]; rows.n2 = c->mdims[2];
        rows.origin0 = c->a_origin - c->first_owned;
        for (int d = 0; d < 3; ++d) { rows.flat[d] = c->mdims[d] == 1 ? 1 : 0; rows.axis[d] = c->perm[d]; }
        ta::launch_junction_reduce(c->stream, labels[k], origins[k], K[k], order[k], N[k], (const uint64_t*)(sp + q.offsets), rows);
        TA_HIP(hipGetLastError());
    }
    TA_HIP(hipEventRecord(c->jn.ev[5], c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    c->jn.nrows[0] = R[0]; c->jn.nrows[1] = R[1];
    c->jn.degenerate = degenerate;
    c->jn.state = 2;
    return TA_OK;
}

// the checks every function behind the extract shares; settles
int junctions_ready(ta_ctx* c) {
    const int rc = results_ready(c, [](const ta_ctx* c) { return c->jn.state != 0; }, NO_TABLES);
    return rc != TA_OK ? rc : junctions_settle(c);
}

int junctions_get(ta_ctx* c, int k, uint32_t* labels, uint64_t* n, uint64_t* sums) {
    const int rc = junctions_ready(c);
    if (rc != TA_OK || !c->jn.nrows[k]) return rc;
    const JunctionTable tb(c->jn.nrows[k], k ? 4 : 3);
    return read_columns(c, c->jn.rows[k].p, {{n, tb.n}, {sums, tb.sums}, {labels, tb.labels}});
}

}  // namespace

// a new label volume (or new label values in it): the junction tables are stale
void junctions_on_new_volume(ta_ctx* c) { c->jn.state = 0; }

extern "C" {

TA_API int ta_junctions_extract(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->vol) return fail(TA_EINVAL, "no label volume set");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    c->jn.state = 0;
    if ((rc = c->jn.small.reserve(16)) != TA_OK) return rc;
    {
        ta::JunctionArgs plan = {};
        plan.n0 = c->mdims[0]; plan.n1 = c->mdims[1]; plan.n2 = c->mdims[2];
        if ((rc = c->jn.work.reserve(JunctionWork(ta::junction_plan(plan, c->itemsize)).bytes)) != TA_OK) return rc;
    }
    if ((rc = ensure_events(c->jn.ev)) != TA_OK) return rc;
    const ta::JunctionArgs a = junction_args(c);
    const JunctionWork w(c->jn.waves);
    char* wp = (char*)c->jn.work.p;
    TA_HIP(hipMemsetAsync(c->jn.small.p, 0, 16, c->stream));
    TA_HIP(hipEventRecord(c->jn.ev[0], c->stream));
    ta::launch_junction_pass(c->stream, a, c->itemsize, false);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->jn.ev[1], c->stream));
    for (int k = 0; k < 2; ++k)
        ta::launch_scan_u32_exclusive(c->stream, (const uint32_t*)(wp + w.counts[k]), c->jn.waves, wp + w.scratch[k], (uint64_t*)(wp + w.offsets[k]));
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->jn.ev[2], c->stream));
    c->jn.state = 1;
    return TA_OK;
}

TA_API int ta_junctions_size(ta_ctx* c, uint64_t* nedges, uint64_t* nvertices, uint64_t* degenerate) {
    const int rc = junctions_ready(c);
    if (rc != TA_OK) return rc;
    if (nedges) *nedges = c->jn.nrows[0];
    if (nvertices) *nvertices = c->jn.nrows[1];
    if (degenerate) *degenerate = c->jn.degenerate;
    return TA_OK;
}

TA_API int ta_junctions_get_edges(ta_ctx* c, uint32_t* labels, uint64_t* n, uint64_t* sums) { return junctions_get(c, 0, labels, n, sums); }

TA_API int ta_junctions_get_vertices(ta_ctx* c, uint32_t* labels, uint64_t* n, uint64_t* sums) { return junctions_get(c, 1, labels, n, sums); }

TA_API int ta_junctions_debug(ta_ctx* c, uint32_t out[4]) {
    const int rc = junctions_ready(c);
    if (rc != TA_OK) return rc;
    if (out) {
        out[0] = (uint32_t)std::min<uint64_t>(c->jn.waves, 0xFFFFFFFFull);
        out[1] = c->jn.key_groups[0]; out[2] = c->jn.key_groups[1]; out[3] = 0u;
    }
    return TA_OK;
}

TA_API int ta_junctions_timing(ta_ctx* c, double* ms_pass, double* ms_after) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (c->jn.state != 2) return fail(TA_EINVAL, "no settled junction tables (ask ta_junctions_size first)");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    TA_HIP(hipEventSynchronize(c->jn.ev[5]));
    double count = 0.0, scans = 0.0, emit = 0.0, rest = 0.0;
    if ((rc = elapsed_ms(c->jn.ev[0], c->jn.ev[1], &count)) != TA_OK || (rc = elapsed_ms(c->jn.ev[1], c->jn.ev[2], &scans)) != TA_OK ||
        (rc = elapsed_ms(c->jn.ev[3], c->jn.ev[4], &emit)) != TA_OK || (rc = elapsed_ms(c->jn.ev[4], c->jn.ev[5], &rest)) != TA_OK) return rc;
    if (ms_pass) *ms_pass = count + emit;
    if (ms_after) *ms_after = scans + rest;
    return TA_OK;
}

}  // extern "C"
