// ta_api_topology.hip -- the C ABI of include/tissue_scan_topology.h on top of kernels_topology.hip.
#include "../../include/tissue_scan_topology.h"
#include "ta_ctx.h"
#include "ta_topology.h"

namespace {

const char* const NO_ROWS = "no Euler-number counts of the current extraction (run ta_topology_extract)";
const char* const NOUN = "Euler-number pass";
static_assert(ta::TP_NFLAGS == RANGE_NFLAGS && ta::TP_FLAG_RANGE == RANGE_FLAG_RANGE && ta::TP_FLAG_SPILL == RANGE_FLAG_SPILL,
              "range_pass_finish reads these words");

// the parts of TopologyState::out for R rows
struct TopologyLayout {
    Part flags, mixed, n0, n1, n2, n3, v, e;
    uint64_t bytes = 0;
    constexpr explicit TopologyLayout(uint64_t R) {
        PartCursor at;
        flags = at.take(16); mixed = at.take(8);
        n0 = at.take(8 * R); n1 = at.take(24 * R); n2 = at.take(24 * R); n3 = at.take(8 * R); v = at.take(8 * R); e = at.take(24 * R);
        bytes = at.end();
    }
};
static_assert(TopologyLayout(3).mixed.at == 16 && TopologyLayout(3).n0.at == 24 && TopologyLayout(3).n2.at == 120 && TopologyLayout(3).e.at == 240 &&
              TopologyLayout(3).bytes == 312, "flags u32[4] | mixed u64 | n0 [R] | n1 [R][3] | n2 [R][3] | n3 [R] | v [R] | e [R][3]");

bool topology_current(const ta_ctx* c) { return pass_current(c, c->tp.seq); }

}  // namespace

// a new label volume (or new label values in it): the rows are stale
void topology_on_new_volume(ta_ctx* c) { c->tp.seq = 0; }

extern "C" {

TA_API int ta_topology_extract(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->vol) return fail(TA_EINVAL, "no label volume set");
    if (c->first_owned != 0 || c->a_origin != 0)
        return fail(TA_EINVAL, "the Euler-number pass does not take a slab (a block at a seam belongs to two buffers)");
    int rc = extraction_preflight(c, NOUN);
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
    a.n0c = (unsigned long long*)(o + L.n0.at);
    a.n1c = (unsigned long long*)(o + L.n1.at);
    a.n2c = (unsigned long long*)(o + L.n2.at);
    a.n3c = (unsigned long long*)(o + L.n3.at);
    a.vc = (unsigned long long*)(o + L.v.at);
    a.ec = (unsigned long long*)(o + L.e.at);
    a.mixed = (unsigned long long*)(o + L.mixed.at);
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
    int rc = results_ready(c, topology_current, NO_ROWS);
    if (rc != TA_OK || (rc = range_pass_finish(c, c->tp.out.p, NOUN)) != TA_OK) return rc;
    const TopologyLayout L(c->tp.rows);
    return read_columns(c, c->tp.out.p, {{n0, L.n0}, {n1, L.n1}, {n2, L.n2}, {n3, L.n3}, {v, L.v}, {e, L.e}});
}

TA_API int ta_topology_debug(ta_ctx* c, uint32_t out[4]) {
    uint32_t spills = 0;
    int rc = results_ready(c, topology_current, NO_ROWS);
    if (rc != TA_OK || (rc = range_pass_finish(c, c->tp.out.p, NOUN, &spills)) != TA_OK) return rc;
    uint64_t mixed = 0;
    if ((rc = read_columns(c, c->tp.out.p, {{&mixed, TopologyLayout(c->tp.rows).mixed}})) != TA_OK) return rc;
    range_debug_words(out, spills, (uint32_t)std::min<uint64_t>(mixed, 0xFFFFFFFFull), c->tp.plan);
    return TA_OK;
}

TA_API int ta_topology_timing(ta_ctx* c, double* ms) {
    return pass_timing(c, ms, [](ta_ctx* c) { return c->tp.seq != 0 && c->tp.ev[1] ? c->tp.ev : nullptr; }, "no Euler-number pass has been run");
}

}  // extern "C"
