// ta_api_sigmoments.hip -- the C ABI of include/tissue_scan_sigmoments.h on top of kernels_sigmoments.hip.
#include "../../include/tissue_scan_sigmoments.h"
#include "ta_ctx.h"
#include "ta_sigmoments.h"

namespace {

const char* const NO_ROWS = "no signal moments of the current extraction (run ta_sigmom_extract)";

// byte offsets of the parts of SigMomentState::out for R rows
struct SigMomLayout {
    uint64_t flags = 0, n, w, m1, m2, bytes;
    explicit SigMomLayout(uint64_t R) { n = 16; w = n + 8 * R; m1 = w + 8 * R; m2 = m1 + 24 * R; bytes = m2 + 96 * R; }
};

// drain the stream and look at the pass's flag words; spills: records that missed a workgroup's LDS table
int sigmom_finish(ta_ctx* c, uint32_t* spills = nullptr) {
    uint32_t flags[ta::SM_NFLAGS] = {0, 0, 0, 0};
    if (const int rc = read_pass_flags<ta::SM_NFLAGS>(c, c->sm.out.p, flags); rc != TA_OK) return rc;
    if (flags[ta::SM_FLAG_RANGE]) return fail(TA_ERANGE, "the signal-moment pass met a label above max_label=%u (the volume changed since ta_extract)", c->max_label);
    if (spills) *spills = flags[ta::SM_FLAG_SPILL];
    return TA_OK;
}

}  // namespace

// a new label volume (or new label values in it), a new signal: the rows are stale
void sigmom_on_new_volume(ta_ctx* c) { c->sm.seq = 0; }
void sigmom_on_new_signal(ta_ctx* c) { c->sm.seq = 0; }

extern "C" {

TA_API int ta_sigmom_extract(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = signal_pass_preflight(c, "signal-moment pass");
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
    a.n = (unsigned long long*)(o + L.n);
    a.w = (unsigned long long*)(o + L.w);
    a.m1 = (unsigned long long*)(o + L.m1);
    a.m2 = (unsigned long long*)(o + L.m2);
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
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!pass_current(c, c->sm.seq)) return fail(TA_EINVAL, NO_ROWS);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = sigmom_finish(c)) != TA_OK) return rc;
    const uint64_t R = c->sm.rows;
    const SigMomLayout L(R);
    const char* o = (const char*)c->sm.out.p;
    if (n) TA_HIP(hipMemcpyAsync(n, o + L.n, 8 * R, hipMemcpyDeviceToHost, c->stream));
    if (w) TA_HIP(hipMemcpyAsync(w, o + L.w, 8 * R, hipMemcpyDeviceToHost, c->stream));
    if (m1) TA_HIP(hipMemcpyAsync(m1, o + L.m1, 24 * R, hipMemcpyDeviceToHost, c->stream));
    if (m2) TA_HIP(hipMemcpyAsync(m2, o + L.m2, 96 * R, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_sigmom_debug(ta_ctx* c, uint32_t out[4]) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!pass_current(c, c->sm.seq)) return fail(TA_EINVAL, NO_ROWS);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    uint32_t spills = 0;
    if ((rc = sigmom_finish(c, &spills)) != TA_OK) return rc;
    if (out) { out[0] = spills; out[1] = 0; out[2] = c->sm.plan.tiles_per_group; out[3] = c->sm.plan.groups; }
    return TA_OK;
}

TA_API int ta_sigmom_timing(ta_ctx* c, double* ms) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!ms) return fail(TA_EINVAL, "NULL argument");
    if (c->sm.seq == 0 || !c->sm.ev[1]) return fail(TA_EINVAL, "no signal-moment pass has been run");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    return interval_ms(c->sm.ev[0], c->sm.ev[1], ms);
}

}  // extern "C"
