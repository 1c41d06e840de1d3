// ta_api_cosignal.hip -- the C ABI of include/tissue_scan_cosignal.h on top of kernels_cosignal.hip.
#include "../../include/tissue_scan_cosignal.h"
#include "ta_cosignal.h"
#include "ta_ctx.h"

namespace {

constexpr CompanionKind CHANNEL_B = {"the second signal", 1, 2};      // uint8 or uint16

const char* const NO_ROWS = "no two-channel rows of the current extraction (run ta_cosignal_extract)";
const char* const NOUN = "two-channel pass";
static_assert(ta::COSIG_NFLAGS == RANGE_NFLAGS && ta::COSIG_FLAG_RANGE == RANGE_FLAG_RANGE && ta::COSIG_FLAG_SPILL == RANGE_FLAG_SPILL,
              "range_pass_finish reads these words");

// the parts of CoSignalState::out for R rows
struct CoSignalLayout {
    Part flags, n, sum_a, sum_b, sq_aa, sq_bb, sq_ab, n_a, n_b, n_ab, over_a, over_b;
    uint64_t bytes = 0;
    constexpr explicit CoSignalLayout(uint64_t R) {
        PartCursor at;
        flags = at.take(16); n = at.take(8 * R); sum_a = at.take(8 * R); sum_b = at.take(8 * R);
        sq_aa = at.take(16 * R); sq_bb = at.take(16 * R); sq_ab = at.take(16 * R);
        n_a = at.take(8 * R); n_b = at.take(8 * R); n_ab = at.take(8 * R); over_a = at.take(8 * R); over_b = at.take(8 * R);
        bytes = at.end();
    }
};
static_assert(CoSignalLayout(3).n.at == 16 && CoSignalLayout(3).sq_aa.at == 88 && CoSignalLayout(3).n_a.at == 232 && CoSignalLayout(3).over_b.at == 328 &&
              CoSignalLayout(3).bytes == 352, "flags u32[4] | n | sum_a | sum_b [R] | sq_aa | sq_bb | sq_ab [R][2] | n_a | n_b | n_ab | over_a | over_b [R]");

bool cosig_current(const ta_ctx* c) { return pass_current(c, c->co.seq); }

}  // namespace

// a new label volume (or new label values in it): the rows are stale; a B of other dims is dropped
void cosig_on_new_volume(ta_ctx* c) {
    c->co.seq = 0;
    companion_on_new_volume(c, c->co.b);
}
// a new A: the rows read the old one
void cosig_on_new_signal(ta_ctx* c) { c->co.seq = 0; }

extern "C" {

TA_API int ta_cosignal_set(ta_ctx* c, const void* host_ptr, int itemsize, const int64_t dims[3], const int64_t strides_bytes[3]) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    const int rc = companion_set_host(c, c->co.b, CHANNEL_B, host_ptr, itemsize, dims, strides_bytes);
    if (rc == TA_OK) c->co.seq = 0;
    return rc;
}

TA_API int ta_cosignal_set_device(ta_ctx* c, const void* dev_ptr, int itemsize) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    const int rc = companion_set_device(c, c->co.b, CHANNEL_B, dev_ptr, itemsize);
    if (rc == TA_OK) c->co.seq = 0;
    return rc;
}

TA_API int ta_cosignal_extract(ta_ctx* c, uint32_t thr_a, uint32_t thr_b) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->co.b.p) return fail(TA_EINVAL, "no second signal set");
    if (!c->vol || !companion_matches(c, c->co.b)) return fail(TA_EINVAL, "the second signal does not match the label volume");
    int rc = signal_pass_preflight(c, NOUN);
    if (rc != TA_OK) return rc;
    c->co.seq = 0;
    const uint64_t R = (uint64_t)c->max_label + 1;
    const CoSignalLayout L(R);
    if ((rc = c->co.out.reserve(L.bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->co.ev)) != TA_OK) return rc;
    char* o = (char*)c->co.out.p;
    TA_HIP(hipMemsetAsync(o, 0, L.bytes, c->stream));
    auto rows = [o](const Part& part) { return (unsigned long long*)(o + part.at); };
    ta::CoSigArgs a;
    a.vol = sweep_vol(c);
    a.a = c->sig.img.p;
    a.b = c->co.b.p;
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.first_owned = c->first_owned;
    a.max_label = c->max_label;
    a.thr_a = thr_a; a.thr_b = thr_b;
    a.n = rows(L.n); a.sum_a = rows(L.sum_a); a.sum_b = rows(L.sum_b);
    a.sq_aa = rows(L.sq_aa); a.sq_bb = rows(L.sq_bb); a.sq_ab = rows(L.sq_ab);
    a.n_a = rows(L.n_a); a.n_b = rows(L.n_b); a.n_ab = rows(L.n_ab);
    a.over_a = rows(L.over_a); a.over_b = rows(L.over_b);
    a.flags = (uint32_t*)o;
    a.tiles_per_group = 0;
    TA_HIP(hipEventRecord(c->co.ev[0], c->stream));
    c->co.plan = ta::launch_cosignal(c->stream, a, c->itemsize, c->sig.img.itemsize, c->co.b.itemsize);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->co.ev[1], c->stream));
    c->co.seq = c->extract_seq;
    c->co.rows = (uint32_t)R;
    c->co.thr[0] = thr_a; c->co.thr[1] = thr_b;
    return TA_OK;
}

TA_API int ta_cosignal_get(ta_ctx* c, uint64_t* n, uint64_t* sum_a, uint64_t* sum_b, uint64_t* sq_aa, uint64_t* sq_bb, uint64_t* sq_ab,
                           uint64_t* n_a, uint64_t* n_b, uint64_t* n_ab, uint64_t* sum_a_over, uint64_t* sum_b_over) {
    int rc = results_ready(c, cosig_current, NO_ROWS);
    if (rc != TA_OK || (rc = range_pass_finish(c, c->co.out.p, NOUN)) != TA_OK) return rc;
    const CoSignalLayout L(c->co.rows);
    return read_columns(c, c->co.out.p, {{n, L.n}, {sum_a, L.sum_a}, {sum_b, L.sum_b}, {sq_aa, L.sq_aa}, {sq_bb, L.sq_bb}, {sq_ab, L.sq_ab},
                                         {n_a, L.n_a}, {n_b, L.n_b}, {n_ab, L.n_ab}, {sum_a_over, L.over_a}, {sum_b_over, L.over_b}});
}

TA_API int ta_cosignal_debug(ta_ctx* c, uint32_t out[4]) {
    uint32_t spills = 0;
    int rc = results_ready(c, cosig_current, NO_ROWS);
    if (rc != TA_OK || (rc = range_pass_finish(c, c->co.out.p, NOUN, &spills)) != TA_OK) return rc;
    range_debug_words(out, spills, 0, c->co.plan);
    return TA_OK;
}

TA_API int ta_cosignal_timing(ta_ctx* c, double* ms) {
    return pass_timing(c, ms, [](ta_ctx* c) { return c->co.seq != 0 && c->co.ev[1] ? c->co.ev : nullptr; }, "no two-channel pass has been run");
}

TA_API int ta_cosignal_thresholds(ta_ctx* c, uint32_t* thr_a, uint32_t* thr_b) {
    const int rc = results_ready(c, cosig_current, NO_ROWS);
    if (rc != TA_OK) return rc;
    if (thr_a) *thr_a = c->co.thr[0];
    if (thr_b) *thr_b = c->co.thr[1];
    return TA_OK;
}

}  // extern "C"
