// ta_api_topology.hip -- the C ABI of include/tissue_scan_topology.h on top of kernels_topology.hip.
#include "../../include/tissue_scan_topology.h"
#include "ta_ctx.h"
#include "ta_topology.h"

namespace {

const char* const NO_ROWS = "no Euler-number counts of the current extraction (run ta_topology_extract)";

// byte offsets of the parts of TopologyState::out for R rows
struct TopologyLayout {
    uint64_t flags = 0, mixed = 16, n0, n1, n2, n3, v, e, bytes;
    explicit TopologyLayout(uint64_t R) { n0 = 24; n1 = n0 + 8 * R; n2 = n1 + 24 * R; n3 = n2 + 24 * R; v = n3 + 8 * R; e = v + 8 * R; bytes = e + 24 * R; }
};

// drain the stream and look at the pass's flag words; spills: records that missed a workgroup's LDS table
int topology_finish(ta_ctx* c, uint32_t* spills = nullptr) {
    uint32_t flags[ta::TP_NFLAGS] = {0, 0, 0, 0};
    if (const int rc = read_pass_flags<ta::TP_NFLAGS>(c, c->tp.out.p, flags); rc != TA_OK) return rc;
    if (flags[ta::TP_FLAG_RANGE]) return fail(TA_ERANGE, "the Euler-number pass met a label above max_label=%u (the volume changed since ta_extract)", c->max_label);
    if (spills) *spills = flags[ta::TP_FLAG_SPILL];
    return TA_OK;
}

}  // namespace

// a new label volume (or new label values in it): the rows are stale
void topology_on_new_volume(ta_ctx* c) { c->tp.seq = 0; }

extern "C" {

TA_API int ta_topology_extract(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->vol) return fail(TA_EINVAL, "no label volume set");
    if (c->first_owned != 0 || c->a_origin != 0)
        return fail(TA_EINVAL, "the Euler-number pass does not take a slab (a block at a seam belongs to two buffers)");
    int rc = extraction_preflight(c, "Euler-number pass");
    if (rc != TA_OK) return rc;
    c->tp.seq = 0;
    const ta::RangePlan plan = ta::topology_plan(c->mdims, c->itemsize);
    const uint64_t R = (uint64_t)c->max_label + 1;
    const TopologyLayout L(R);
    if ((rc = c->tp.out.reserve(L.bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->tp.ev)) != TA_OK) return rc;
    char* o = (char*)c->tp.out.p;
    TA_HIP(hipMemsetAsync(o, 0, L.bytes, c->stream));
    ta::TopologyArgs a;
    a.vol = sweep_vol(c);
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.max_label = c->max_label;
    a.n0c = (unsigned long long*)(o + L.n0);
    a.n1c = (unsigned long long*)(o + L.n1);
    a.n2c = (unsigned long long*)(o + L.n2);
    a.n3c = (unsigned long long*)(o + L.n3);
    a.vc = (unsigned long long*)(o + L.v);
    a.ec = (unsigned long long*)(o + L.e);
    a.mixed = (unsigned long long*)(o + L.mixed);
    a.flags = (uint32_t*)o;
    a.tiles_per_group = 0;
    TA_HIP(hipEventRecord(c->tp.ev[0], c->stream));
    ta::launch_topology(c->stream, a, c->itemsize, plan);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->tp.ev[1], c->stream));
    c->tp.plan = plan;
    c->tp.seq = c->extract_seq;
    c->tp.rows = (uint32_t)R;
    return TA_OK;
}

TA_API int ta_topology_get(ta_ctx* c, uint64_t* n0, uint64_t* n1, uint64_t* n2, uint64_t* n3, uint64_t* v, uint64_t* e) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!pass_current(c, c->tp.seq)) return fail(TA_EINVAL, NO_ROWS);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = topology_finish(c)) != TA_OK) return rc;
    const uint64_t R = c->tp.rows;
    const TopologyLayout L(R);
    const char* o = (const char*)c->tp.out.p;
    if (n0) TA_HIP(hipMemcpyAsync(n0, o + L.n0, 8 * R, hipMemcpyDeviceToHost, c->stream));
    if (n1) TA_HIP(hipMemcpyAsync(n1, o + L.n1, 24 * R, hipMemcpyDeviceToHost, c->stream));
    if (n2) TA_HIP(hipMemcpyAsync(n2, o + L.n2, 24 * R, hipMemcpyDeviceToHost, c->stream));
    if (n3) TA_HIP(hipMemcpyAsync(n3, o + L.n3, 8 * R, hipMemcpyDeviceToHost, c->stream));
    if (v) TA_HIP(hipMemcpyAsync(v, o + L.v, 8 * R, hipMemcpyDeviceToHost, c->stream));
    if (e) TA_HIP(hipMemcpyAsync(e, o + L.e, 24 * R, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_topology_debug(ta_ctx* c, uint32_t out[4]) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!pass_current(c, c->tp.seq)) return fail(TA_EINVAL, NO_ROWS);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    uint32_t spills = 0;
    if ((rc = topology_finish(c, &spills)) != TA_OK) return rc;
    uint64_t mixed = 0;
    TA_HIP(hipMemcpyAsync(&mixed, (const char*)c->tp.out.p + TopologyLayout(c->tp.rows).mixed, 8, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    if (out) {
        out[0] = spills;
        out[1] = (uint32_t)std::min<uint64_t>(mixed, 0xFFFFFFFFull);
        out[2] = c->tp.plan.tiles_per_group;
        out[3] = c->tp.plan.groups;
    }
    return TA_OK;
}

TA_API int ta_topology_timing(ta_ctx* c, double* ms) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!ms) return fail(TA_EINVAL, "NULL argument");
    if (c->tp.seq == 0 || !c->tp.ev[1]) return fail(TA_EINVAL, "no Euler-number pass has been run");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    return interval_ms(c->tp.ev[0], c->tp.ev[1], ms);
}

}  // extern "C"
