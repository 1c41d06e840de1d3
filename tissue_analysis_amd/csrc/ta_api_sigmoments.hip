// ta_api_sigmoments.hip -- the C ABI of include/tissue_scan_sigmoments.h on top of kernels_sigmoments.hip.
#include "../../include/tissue_scan_sigmoments.h"
#include "ta_ctx.h"
#include "ta_sigmoments.h"

namespace {

const char* const NO_ROWS = "no signal moments of the current extraction (run ta_sigmom_extract)";
const char* const NOUN = "signal-moment pass";
static_assert(ta::SM_NFLAGS == RANGE_NFLAGS && ta::SM_FLAG_RANGE == RANGE_FLAG_RANGE && ta::SM_FLAG_SPILL == RANGE_FLAG_SPILL,
              "range_pass_finish reads these words");

// the parts of SigMomentState::out for R rows
struct SigMomLayout {
    Part flags, n, w, m1, m2;
    uint64_t bytes = 0;
    constexpr explicit SigMomLayout(uint64_t R) {
        PartCursor at;
        flags = at.take(16); n = at.take(8 * R); w = at.take(8 * R); m1 = at.take(24 * R); m2 = at.take(96 * R);
        bytes = at.end();
    }
};
static_assert(SigMomLayout(3).n.at == 16 && SigMomLayout(3).w.at == 40 && SigMomLayout(3).m1.at == 64 && SigMomLayout(3).m2.at == 136 &&
              SigMomLayout(3).bytes == 424, "flags u32[4] | n [R] | w [R] | m1 [R][3] | m2 [R][6][2]");

bool sigmom_current(const ta_ctx* c) { return pass_current(c, c->sm.seq); }

}  // namespace

// a new label volume (or new label values in it), a new signal: the rows are stale
void sigmom_on_new_volume(ta_ctx* c) { c->sm.seq = 0; }
void sigmom_on_new_signal(ta_ctx* c) { c->sm.seq = 0; }

extern "C" {

TA_API int ta_sigmom_extract(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = signal_pass_preflight(c, NOUN);
    if (rc != TA_OK) return rc;
    c->sm.seq = 0;
    ta::RangePlan plan;
    const int verdict = ta::sigmoments_plan(c->mdims, c->first_owned, c->itemsize, c->sig.img.itemsize, &plan);
    if (verdict == 1)
        return fail(TA_EINVAL, "dims %lld x %lld x %lld are too large for the signal-moment pass: a first moment could pass 2^64",
                    (long long)c->mdims[0], (long long)c->mdims[1], (long long)c->mdims[2]);
    if (verdict == 2)
        return fail(TA_EINVAL, "dims %lld x %lld x %lld are too large for the signal-moment pass: the second moments of one tile could pass 2^64",
                    (long long)c->mdims[0], (long long)c->mdims[1], (long long)c->mdims[2]);
    const uint64_t R = (uint64_t)c->max_label + 1;
    const SigMomLayout L(R);
    if ((rc = c->sm.out.reserve(L.bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->sm.ev)) != TA_OK) return rc;
    char* o = (char*)c->sm.out.p;
    TA_HIP(hipMemsetAsync(o, 0, L.bytes, c->stream));
    ta::SigMomArgs a;
    a.vol = sweep_vol(c);
    a.sig = c->sig.img.p;
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.first_owned = c->first_owned;
    a.max_label = c->max_label;
    a.n = (unsigned long long*)(o + L.n.at);
    a.w = (unsigned long long*)(o + L.w.at);
    a.m1 = (unsigned long long*)(o + L.m1.at);
    a.m2 = (unsigned long long*)(o + L.m2.at);
    a.flags = (uint32_t*)o;
    a.tiles_per_group = 0;
    TA_HIP(hipEventRecord(c->sm.ev[0], c->stream));
    ta::launch_sigmoments(c->stream, a, c->itemsize, c->sig.img.itemsize, plan);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->sm.ev[1], c->stream));
    c->sm.plan = plan;
    c->sm.seq = c->extract_seq;
    c->sm.rows = (uint32_t)R;
    return TA_OK;
}

TA_API int ta_sigmom_get(ta_ctx* c, uint64_t* n, uint64_t* w, uint64_t* m1, uint64_t* m2) {
    int rc = results_ready(c, sigmom_current, NO_ROWS);
    if (rc != TA_OK || (rc = range_pass_finish(c, c->sm.out.p, NOUN)) != TA_OK) return rc;
    const SigMomLayout L(c->sm.rows);
    return read_columns(c, c->sm.out.p, {{n, L.n}, {w, L.w}, {m1, L.m1}, {m2, L.m2}});
}

TA_API int ta_sigmom_debug(ta_ctx* c, uint32_t out[4]) {
    uint32_t spills = 0;
    int rc = results_ready(c, sigmom_current, NO_ROWS);
    if (rc != TA_OK || (rc = range_pass_finish(c, c->sm.out.p, NOUN, &spills)) != TA_OK) return rc;
    range_debug_words(out, spills, 0, c->sm.plan);
    return TA_OK;
}

TA_API int ta_sigmom_timing(ta_ctx* c, double* ms) {
    return pass_timing(c, ms, [](ta_ctx* c) { return c->sm.seq != 0 && c->sm.ev[1] ? c->sm.ev : nullptr; }, "no signal-moment pass has been run");
}

}  // extern "C"
