// ta_api_junctions.hip -- the C ABI of include/tissue_scan_junctions.h on top of kernels_junctions.hip.
#include "../../include/tissue_scan_junctions.h"
#include "ta_ctx.h"
#include "ta_junctions.h"

namespace {

// JunctionState::work for W waves: the count/scan block of the edge records, then the vertex records'
ScanBlock junction_counts(uint64_t W, int k) { return ScanBlock(W, k ? ScanBlock(W).end : 0); }

// JunctionState::sort[k] for N records: the sort workspace, then the count/scan block of the rows that start in a block of records
struct JunctionSort {
    SortLayout sort;
    ScanBlock heads;
    explicit JunctionSort(uint64_t N) : sort(N, 8), heads(ta::junction_row_blocks(N), sort.end) {}
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
    const ScanBlock w3 = junction_counts(c->jn.waves, 0), w4 = junction_counts(c->jn.waves, 1);
    a.wave_counts3 = w3.counts(c->jn.work.p); a.wave_counts4 = w4.counts(c->jn.work.p);
    a.wave_offsets3 = w3.offsets(c->jn.work.p); a.wave_offsets4 = w4.offsets(c->jn.work.p);
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
    uint64_t N[2] = {0, 0}, degenerate = 0;
    for (int k = 0; k < 2; ++k) TA_HIP(junction_counts(c->jn.waves, k).read_total(c->stream, c->jn.work.p, &N[k]));
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
        if ((rc = c->jn.sort[k].reserve(JunctionSort(N[k]).heads.end + 16)) != TA_OK) return rc;
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
    const uint32_t* order[2] = {nullptr, nullptr};
    uint64_t R[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        const uint64_t n = N[k];
        c->jn.key_groups[k] = 0u;
        if (!n) continue;
        const JunctionSort q(n);
        void* sp = c->jn.sort[k].p;
        SortView<uint64_t> v(q.sort, sp);
        c->jn.key_groups[k] = ta::launch_junction_keys(c->stream, labels[k], K[k], n, nullptr, K[k] - 2, K[k] - 1, lb, v.keys(), v.idx());
        TA_HIP(v.sort(c->stream, n, 2 * lb));
        // the leading columns of the records in that order, into the key buffer the order came out with
        ta::launch_junction_keys(c->stream, labels[k], K[k], n, v.idx(), K[k] == 4 ? 0 : -1, K[k] == 4 ? 1 : 0, lb, v.keys(), nullptr);
        TA_HIP(v.sort(c->stream, n, K[k] == 4 ? 2 * lb : lb));
        order[k] = v.idx();
        ta::launch_junction_heads(c->stream, labels[k], K[k], order[k], n, q.heads.counts(sp));
        q.heads.scan(c->stream, sp);
        TA_HIP(hipGetLastError());
        TA_HIP(q.heads.read_total(c->stream, sp, &R[k]));
    }
    TA_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 2; ++k)
        if ((rc = c->jn.rows[k].reserve(JunctionTable(R[k], K[k]).bytes)) != TA_OK) return rc;
    for (int k = 0; k < 2; ++k) {
        if (!N[k]) continue;
        const JunctionSort q(N[k]);
        const JunctionTable tb(R[k], K[k]);
        char* op = (char*)c->jn.rows[k].p;
        TA_HIP(hipMemsetAsync(op, 0, tb.labels.at, c->stream));
        ta::JunctionRows rows;
        rows.n = (unsigned long long*)(op + tb.n.at);
        rows.sums = (unsigned long long*)(op + tb.sums.at);
        rows.labels = (uint32_t*)(op + tb.labels.at);
        rows.n0 = c->mdims[0]; rows.n1 = c->mdims[1]; rows.n2 = c->mdims[2];
        rows.origin0 = c->a_origin - c->first_owned;
        for (int d = 0; d < 3; ++d) { rows.flat[d] = c->mdims[d] == 1 ? 1 : 0; rows.axis[d] = c->perm[d]; }
        ta::launch_junction_reduce(c->stream, labels[k], origins[k], K[k], order[k], N[k], q.heads.offsets(c->jn.sort[k].p), rows);
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
        if ((rc = c->jn.work.reserve(junction_counts(ta::junction_plan(plan, c->itemsize), 1).end + 16)) != TA_OK) return rc;
    }
    if ((rc = ensure_events(c->jn.ev)) != TA_OK) return rc;
    const ta::JunctionArgs a = junction_args(c);
    TA_HIP(hipMemsetAsync(c->jn.small.p, 0, 16, c->stream));
    TA_HIP(hipEventRecord(c->jn.ev[0], c->stream));
    ta::launch_junction_pass(c->stream, a, c->itemsize, false);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->jn.ev[1], c->stream));
    for (int k = 0; k < 2; ++k) junction_counts(c->jn.waves, k).scan(c->stream, c->jn.work.p);
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
    hipEvent_t* ev = c->jn.ev;                     // count + emit | scans + the rest
    double pass = 0.0, after = 0.0;
    TA_HIP(summed_ms(ev[5], {{ev[0], ev[1]}, {ev[3], ev[4]}}, &pass));
    TA_HIP(summed_ms(ev[5], {{ev[1], ev[2]}, {ev[4], ev[5]}}, &after));
    if (ms_pass) *ms_pass = pass;
    if (ms_after) *ms_after = after;
    return TA_OK;
}

}  // extern "C"
