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

// the table belongs to the current extraction AND to the distance map the context holds (a new one ends it: profile_on_new_distance)
bool profile_current(const ta_ctx* c) { return pass_current(c, c->prof.seq) && c->dist.seq == c->extract_seq; }

// byte offsets of the parts of ProfileState::out for N = rows x bins entries; the signal columns only in a pass with signal
struct ProfileLayout {
    uint64_t flags = 0, edges = 16, n, sum, sumsq, vmin, vmax, bytes;
    ProfileLayout(uint64_t N, bool signal) {
        n = align16(edges + 8 * (ta::PROF_MAX_BINS + 1)); sum = n + 8 * N; sumsq = sum + 8 * N; vmin = sumsq + 16 * N; vmax = vmin + 4 * N;
        bytes = signal ? vmax + 4 * N : sum;
    }
};

int profile_ready(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!profile_current(c)) return fail(TA_EINVAL, NO_RESULTS);
    return use_device(c);
}

// drain the stream and look at the pass's flag words
int profile_finish(ta_ctx* c, uint32_t* spills = nullptr) {
    uint32_t flags[ta::PROF_NFLAGS] = {0, 0, 0, 0};
    if (const int rc = read_pass_flags<ta::PROF_NFLAGS>(c, c->prof.out.p, flags); rc != TA_OK) return rc;
    if (flags[ta::PROF_FLAG_RANGE])
        return fail(TA_ERANGE, "the profile pass met a label above max_label=%u (the volume changed since ta_extract)", c->max_label);
    if (spills) *spills = flags[ta::PROF_FLAG_SPILL];
    return TA_OK;
}

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
    if (signal) TA_HIP(hipMemsetAsync(o + L.vmin, 0xff, 4 * N, c->stream));
    ta::ProfileArgs a = {};
    a.vol = sweep_vol(c);
    a.d2 = (const double*)c->dist.d2.p;
    a.sig = signal ? c->sig.img.p : nullptr;
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.max_label = c->max_label;
    a.bins = (uint32_t)nbins;
    a.n = (unsigned long long*)(o + L.n);
    a.sum = (unsigned long long*)(o + L.sum);
    a.sumsq = (unsigned long long*)(o + L.sumsq);
    a.vmin = (uint32_t*)(o + L.vmin);
    a.vmax = (uint32_t*)(o + L.vmax);
    a.flags = (uint32_t*)o;
    for (int k = 0; k <= ta::PROF_MAX_BINS; ++k) c->prof.edges[k] = k <= nbins ? edges2[k] : std::numeric_limits<double>::infinity();
    TA_HIP(hipMemcpyAsync(o + L.edges, c->prof.edges, sizeof(c->prof.edges), hipMemcpyHostToDevice, c->stream));
    a.edges = (const double*)(o + L.edges);
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
    int rc = profile_ready(c);
    if (rc != TA_OK) return rc;
    if (!c->prof.with_signal && (sum || sumsq || vmin || vmax))
        return fail(TA_EINVAL, "the profile pass ran without a signal (TA_PROF_SIGNAL): it has no sum, sumsq, min or max");
    if ((rc = profile_finish(c)) != TA_OK) return rc;
    const uint64_t N = (uint64_t)c->prof.rows * c->prof.bins;
    const ProfileLayout L(N, c->prof.with_signal);
    const char* o = (const char*)c->prof.out.p;
    if (n) TA_HIP(hipMemcpyAsync(n, o + L.n, 8 * N, hipMemcpyDeviceToHost, c->stream));
    if (sum) TA_HIP(hipMemcpyAsync(sum, o + L.sum, 8 * N, hipMemcpyDeviceToHost, c->stream));
    if (sumsq) TA_HIP(hipMemcpyAsync(sumsq, o + L.sumsq, 16 * N, hipMemcpyDeviceToHost, c->stream));
    if (vmin) TA_HIP(hipMemcpyAsync(vmin, o + L.vmin, 4 * N, hipMemcpyDeviceToHost, c->stream));
    if (vmax) TA_HIP(hipMemcpyAsync(vmax, o + L.vmax, 4 * N, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_profile_debug(ta_ctx* c, uint32_t out[4]) {
    int rc = profile_ready(c);
    if (rc != TA_OK) return rc;
    uint32_t spills = 0;
    if ((rc = profile_finish(c, &spills)) != TA_OK) return rc;
    if (out) { out[0] = spills; out[1] = 0; out[2] = c->prof.plan.tiles_per_group; out[3] = c->prof.plan.groups; }
    return TA_OK;
}

TA_API int ta_profile_timing(ta_ctx* c, double* ms) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!ms) return fail(TA_EINVAL, "NULL argument");
    int rc = profile_ready(c);
    if (rc != TA_OK) return rc;
    return interval_ms(c->prof.ev[0], c->prof.ev[1], ms);
}

}  // extern "C"
