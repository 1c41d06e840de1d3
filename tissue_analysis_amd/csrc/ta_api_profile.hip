// ta_api_profile.hip -- the C ABI of include/tissue_scan_profile.h on top of kernels_profile.hip.
#include "../../include/tissue_scan_profile.h"
#include "ta_ctx.h"
#include "ta_profile.h"

#include <cmath>
#include <limits>

namespace {

static_assert(TA_PROF_MAX_BINS == ta::PROF_MAX_BINS, "the public header and the kernel disagree on the shells of a row");
static_assert(sizeof(ProfileState::edges) == 8 * (ta::PROF_MAX_BINS + 1), "ProfileState::edges holds K + 1 edges for the largest K");

const char* const NO_RESULTS = "no distance-shell profile of the current distance map (run ta_profile_extract)";
const char* const NOUN = "profile pass";
static_assert(ta::PROF_NFLAGS == RANGE_NFLAGS && ta::PROF_FLAG_RANGE == RANGE_FLAG_RANGE && ta::PROF_FLAG_SPILL == RANGE_FLAG_SPILL,
              "range_pass_finish reads these words");

// the table belongs to the current extraction AND to the distance map the context holds (a new one ends it: profile_on_new_distance)
bool profile_current(const ta_ctx* c) { return pass_current(c, c->prof.seq) && c->dist.seq == c->extract_seq; }

// the parts of ProfileState::out for N = rows x bins entries; the buffer ends behind n in a pass without signal
struct ProfileLayout {
    Part flags, edges, n, sum, sumsq, vmin, vmax;
    uint64_t bytes = 0;
    constexpr ProfileLayout(uint64_t N, bool signal) {
        PartCursor at;
        flags = at.take(16); edges = at.take(8 * (ta::PROF_MAX_BINS + 1)); n = at.take(8 * N, 16);
        sum = at.take(8 * N); sumsq = at.take(16 * N); vmin = at.take(4 * N); vmax = at.take(4 * N);
        bytes = signal ? at.end() : sum.at;
    }
};
static_assert(ta::PROF_MAX_BINS == 64 && ProfileLayout(6, true).edges.at == 16 && ProfileLayout(6, true).n.at == 544 && ProfileLayout(6, true).sumsq.at == 640 &&
              ProfileLayout(6, true).vmin.at == 736 && ProfileLayout(6, true).vmax.at == 760 && ProfileLayout(6, true).bytes == 784 &&
              ProfileLayout(6, false).bytes == 592, "flags u32[4] | edges f64[65] | n [N] from a multiple of 16 | sum [N] | sumsq [N][2] | min u32[N] | max u32[N]");

}  // namespace

// a new label volume (or new label values in it), a new distance map, a new signal under a table that read the old one: stale
void profile_on_new_volume(ta_ctx* c) { c->prof.seq = 0; }
void profile_on_new_distance(ta_ctx* c) { c->prof.seq = 0; }
void profile_on_new_signal(ta_ctx* c) { if (c->prof.with_signal) c->prof.seq = 0; }

extern "C" {

TA_API int ta_profile_extract(ta_ctx* c, int nbins, const double* edges2, uint32_t what) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (what & ~TA_PROF_SIGNAL) return fail(TA_EINVAL, "bad profile mask 0x%x", what);
    if (nbins < 1 || nbins > TA_PROF_MAX_BINS) return fail(TA_EINVAL, "nbins=%d is not in [1, %d]", nbins, TA_PROF_MAX_BINS);
    if (!edges2) return fail(TA_EINVAL, "edges2 is NULL");
    if (!(edges2[0] >= 0.0)) return fail(TA_EINVAL, "edges2[0]=%g is negative or NaN", edges2[0]);
    for (int k = 0; k < nbins; ++k)
        if (!(edges2[k + 1] > edges2[k])) return fail(TA_EINVAL, "edges2[%d]=%g does not lie above edges2[%d]=%g", k + 1, edges2[k + 1], k, edges2[k]);
    const bool signal = what & TA_PROF_SIGNAL;
    if (!c->vol || !pass_current(c, c->dist.seq))
        return fail(TA_EINVAL, "the profile pass needs a ta_distance_extract of the current extraction first");
    if (signal && !c->sig.img.p) return fail(TA_EINVAL, "TA_PROF_SIGNAL without a signal set");
    if (signal && !companion_matches(c, c->sig.img)) return fail(TA_EINVAL, "the signal does not match the label volume");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = finish_extract(c)) != TA_OK) return rc;
    c->prof.seq = 0;
    const uint64_t R = (uint64_t)c->max_label + 1, K = (uint64_t)nbins, N = R * K;
    if (N > (1ull << 31)) return fail(TA_EINVAL, "too many (row, shell) entries: %llu rows x %d shells > 2^31", (unsigned long long)R, nbins);
    const ProfileLayout L(N, signal);
    if ((rc = c->prof.out.reserve(L.bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->prof.ev)) != TA_OK) return rc;
    char* o = (char*)c->prof.out.p;
    TA_HIP(hipMemsetAsync(o, 0, L.bytes, c->stream));
    if (signal) TA_HIP(hipMemsetAsync(o + L.vmin.at, 0xff, L.vmin.bytes, c->stream));
    ta::ProfileArgs a = {};
    a.vol = sweep_vol(c);
    a.d2 = (const double*)c->dist.d2.p;
    a.sig = signal ? c->sig.img.p : nullptr;
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.max_label = c->max_label;
    a.bins = (uint32_t)nbins;
    a.n = (unsigned long long*)(o + L.n.at);
    a.sum = (unsigned long long*)(o + L.sum.at);
    a.sumsq = (unsigned long long*)(o + L.sumsq.at);
    a.vmin = (uint32_t*)(o + L.vmin.at);
    a.vmax = (uint32_t*)(o + L.vmax.at);
    a.flags = (uint32_t*)o;
    for (int k = 0; k <= ta::PROF_MAX_BINS; ++k) c->prof.edges[k] = k <= nbins ? edges2[k] : std::numeric_limits<double>::infinity();
    TA_HIP(hipMemcpyAsync(o + L.edges.at, c->prof.edges, sizeof(c->prof.edges), hipMemcpyHostToDevice, c->stream));
    a.edges = (const double*)(o + L.edges.at);
    TA_HIP(hipEventRecord(c->prof.ev[0], c->stream));
    c->prof.plan = ta::launch_profile(c->stream, a, c->itemsize, signal ? c->sig.img.itemsize : 0);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->prof.ev[1], c->stream));
    c->prof.seq = c->extract_seq;
    c->prof.rows = (uint32_t)R;
    c->prof.bins = (uint32_t)nbins;
    c->prof.with_signal = signal;
    return TA_OK;
}

TA_API int ta_profile_get(ta_ctx* c, uint64_t* n, uint64_t* sum, uint64_t* sumsq, uint32_t* vmin, uint32_t* vmax) {
    int rc = results_ready(c, profile_current, NO_RESULTS);
    if (rc != TA_OK) return rc;
    if (!c->prof.with_signal && (sum || sumsq || vmin || vmax))
        return fail(TA_EINVAL, "the profile pass ran without a signal (TA_PROF_SIGNAL): it has no sum, sumsq, min or max");
    if ((rc = range_pass_finish(c, c->prof.out.p, NOUN)) != TA_OK) return rc;
    const ProfileLayout L((uint64_t)c->prof.rows * c->prof.bins, c->prof.with_signal);
    return read_columns(c, c->prof.out.p, {{n, L.n}, {sum, L.sum}, {sumsq, L.sumsq}, {vmin, L.vmin}, {vmax, L.vmax}});
}

TA_API int ta_profile_debug(ta_ctx* c, uint32_t out[4]) {
    uint32_t spills = 0;
    int rc = results_ready(c, profile_current, NO_RESULTS);
    if (rc != TA_OK || (rc = range_pass_finish(c, c->prof.out.p, NOUN, &spills)) != TA_OK) return rc;
    range_debug_words(out, spills, 0, c->prof.plan);
    return TA_OK;
}

TA_API int ta_profile_timing(ta_ctx* c, double* ms) {
    return pass_timing(c, ms, [](ta_ctx* c) { return profile_current(c) ? c->prof.ev : nullptr; }, NO_RESULTS);
}

}  // extern "C"
