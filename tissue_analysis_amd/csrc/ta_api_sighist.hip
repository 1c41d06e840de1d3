// ta_api_sighist.hip -- the C ABI of include/tissue_scan_sighist.h on top of kernels_sighist.hip.
#include "../../include/tissue_scan_sighist.h"
#include "ta_ctx.h"
#include "ta_sighist.h"

#include <limits>

namespace {

static_assert(TA_SIGRANK_MAX_RANKS == ta::SH_MAX_RANKS, "the public header and the kernel disagree on the ranks of a row");

const char* const NO_HIST = "no signal histogram of the current extraction (run ta_sighist_extract)";
const char* const NO_RANK = "no order statistics of the current extraction (run ta_sigrank_extract)";

// byte offsets of the parts of SigHistState::rank for R rows of n ranks; counts2 only for a uint16 signal
struct RankLayout {
    uint64_t flags = 0, ranks, rem, hi, sel, map, values, counts1, counts2, bytes;
    RankLayout(uint64_t R, uint64_t n, bool two) {
        const uint64_t N = R * n;
        ranks = 2 * sizeof(uint32_t) * ta::SH_NFLAGS; rem = ranks + 8 * N; hi = rem + 8 * N; sel = align16(hi + 4 * N); map = align16(sel + 4 * N);
        values = align16(map + 4 * N); counts1 = align16(values + 4 * N); counts2 = counts1 + 8 * 256 * R;
        bytes = two ? counts2 + 8 * 256 * N : counts2;
    }
};

ta::DigitArgs digit_args(const ta_ctx* c) {
    ta::DigitArgs a = {};
    a.vol = sweep_vol(c);
    a.sig = c->sig.img.p;
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.first_owned = c->first_owned;
    a.max_label = c->max_label;
    return a;
}

// drain the stream and look at the flag words of `passes` digit passes at `flags`; spills: those of the last of them
int digits_finish(ta_ctx* c, const void* flags, int passes, uint32_t* spills = nullptr) {
    uint32_t f[2 * ta::SH_NFLAGS] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int rc = passes == 2 ? read_pass_flags<2 * ta::SH_NFLAGS>(c, flags, f) : read_pass_flags<ta::SH_NFLAGS>(c, flags, f);
    if (rc != TA_OK) return rc;
    if (f[ta::SH_FLAG_RANGE] || f[ta::SH_NFLAGS + ta::SH_FLAG_RANGE])
        return fail(TA_ERANGE, "the pass met a label above max_label=%u (the volume changed since ta_extract)", c->max_label);
    if (spills) *spills = f[(passes - 1) * ta::SH_NFLAGS + ta::SH_FLAG_SPILL];
    return TA_OK;
}

}  // namespace

// a new label volume (or new label values in it), a new signal: both tables are stale
void sighist_on_new_volume(ta_ctx* c) { c->sh.hist_seq = c->sh.rank_seq = 0; c->sh.last = 0; }
void sighist_on_new_signal(ta_ctx* c) { sighist_on_new_volume(c); }

extern "C" {

TA_API int ta_sighist_extract(ta_ctx* c, int log2_width) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = signal_pass_preflight(c, "pass");
    if (rc != TA_OK) return rc;
    const int bits = 8 * c->sig.img.itemsize;
    if (log2_width < bits - 8 || log2_width > bits)
        return fail(TA_EINVAL, "log2_width=%d is not in [%d, %d] (1 .. 256 bins of a %d-bit signal)", log2_width, bits - 8, bits, bits);
    c->sh.hist_seq = 0;
    const uint64_t R = (uint64_t)c->max_label + 1, B = 1ull << (bits - log2_width);
    if (R * 256 > (1ull << 31)) return fail(TA_EINVAL, "too many keys: %llu rows x 256 > 2^31", (unsigned long long)R);
    const uint64_t bytes = 16 + 8 * R * B;
    if ((rc = c->sh.out.reserve(bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->sh.ev)) != TA_OK) return rc;
    char* o = (char*)c->sh.out.p;
    TA_HIP(hipMemsetAsync(o, 0, bytes, c->stream));
    ta::DigitArgs a = digit_args(c);
    a.shift = (uint32_t)log2_width;
    a.stride = (uint32_t)B;
    a.nsel = 0; a.sel = nullptr;
    a.counts = (unsigned long long*)(o + 16);
    a.flags = (uint32_t*)o;
    TA_HIP(hipEventRecord(c->sh.ev[0], c->stream));
    c->sh.plan = ta::launch_sighist_digits(c->stream, a, c->itemsize, c->sig.img.itemsize);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->sh.ev[1], c->stream));
    c->sh.hist_seq = c->extract_seq;
    c->sh.rows = (uint32_t)R;
    c->sh.bins = (uint32_t)B;
    c->sh.last = 1;
    return TA_OK;
}

TA_API int ta_sighist_get(ta_ctx* c, uint64_t* counts) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!pass_current(c, c->sh.hist_seq)) return fail(TA_EINVAL, NO_HIST);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = digits_finish(c, c->sh.out.p, 1)) != TA_OK) return rc;
    if (counts) {
        TA_HIP(hipMemcpyAsync(counts, (const char*)c->sh.out.p + 16, 8 * (uint64_t)c->sh.rows * c->sh.bins, hipMemcpyDeviceToHost, c->stream));
        TA_HIP(hipStreamSynchronize(c->stream));
    }
    return TA_OK;
}

TA_API int ta_sigrank_extract(ta_ctx* c, int nranks, const uint64_t* ranks) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (nranks < 1 || nranks > TA_SIGRANK_MAX_RANKS) return fail(TA_EINVAL, "nranks=%d is not in [1, %d]", nranks, TA_SIGRANK_MAX_RANKS);
    if (!ranks) return fail(TA_EINVAL, "ranks is NULL");
    int rc = signal_pass_preflight(c, "pass");
    if (rc != TA_OK) return rc;
    if (c->first_owned || c->a_origin)
        return fail(TA_EINVAL, "order statistics of a slab are not those of the volume: ta_sigrank_extract takes whole volumes only");
    c->sh.rank_seq = 0;
    const uint64_t R = (uint64_t)c->max_label + 1, N = R * (uint64_t)nranks;
    if (N * 256 > (1ull << 31)) return fail(TA_EINVAL, "too many keys: %llu rows x %d ranks x 256 > 2^31", (unsigned long long)R, nranks);
    const bool two = c->sig.img.itemsize == 2;
    const RankLayout L(R, (uint64_t)nranks, two);
    if ((rc = c->sh.rank.reserve(L.bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->sh.ev)) != TA_OK) return rc;
    try { c->sh.h_ranks.assign(ranks, ranks + N); } catch (...) { return fail(TA_ENOMEM, "out of host memory"); }
    char* o = (char*)c->sh.rank.p;
    TA_HIP(hipMemsetAsync(o, 0, L.bytes, c->stream));
    TA_HIP(hipMemcpyAsync(o + L.ranks, c->sh.h_ranks.data(), 8 * N, hipMemcpyHostToDevice, c->stream));
    ta::SelectArgs sa = {};
    sa.rows = (uint32_t)R; sa.nranks = (uint32_t)nranks;
    sa.ranks = (const unsigned long long*)(o + L.ranks);
    sa.counts1 = (const unsigned long long*)(o + L.counts1);
    sa.counts2 = (const unsigned long long*)(o + L.counts2);
    sa.rem = (unsigned long long*)(o + L.rem);
    sa.hi = (uint32_t*)(o + L.hi); sa.sel = (uint32_t*)(o + L.sel); sa.map = (uint32_t*)(o + L.map); sa.values = (uint32_t*)(o + L.values);
    ta::DigitArgs a = digit_args(c);
    a.shift = two ? 8u : 0u;
    a.stride = 256;
    a.nsel = 0; a.sel = nullptr;
    a.counts = (unsigned long long*)(o + L.counts1);
    a.flags = (uint32_t*)o;
    TA_HIP(hipEventRecord(c->sh.ev[2], c->stream));
    c->sh.plan = ta::launch_sighist_digits(c->stream, a, c->itemsize, c->sig.img.itemsize);
    ta::launch_sighist_select_first(c->stream, sa, !two);
    if (two) {
        a.shift = 0;
        a.nsel = (uint32_t)nranks; a.sel = sa.sel;
        a.counts = (unsigned long long*)(o + L.counts2);
        a.flags = (uint32_t*)o + ta::SH_NFLAGS;
        c->sh.plan = ta::launch_sighist_digits(c->stream, a, c->itemsize, 2);
        ta::launch_sighist_select_second(c->stream, sa);
    }
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->sh.ev[3], c->stream));
    c->sh.rank_seq = c->extract_seq;
    c->sh.rank_rows = (uint32_t)R;
    c->sh.nranks = (uint32_t)nranks;
    c->sh.rank_passes = two ? 2 : 1;
    c->sh.last = 2;
    return TA_OK;
}

TA_API int ta_sigrank_get(ta_ctx* c, uint32_t* values) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!pass_current(c, c->sh.rank_seq)) return fail(TA_EINVAL, NO_RANK);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = digits_finish(c, c->sh.rank.p, c->sh.rank_passes)) != TA_OK) return rc;
    if (values) {
        const RankLayout L(c->sh.rank_rows, c->sh.nranks, c->sh.rank_passes == 2);
        TA_HIP(hipMemcpyAsync(values, (const char*)c->sh.rank.p + L.values, 4 * (uint64_t)c->sh.rank_rows * c->sh.nranks, hipMemcpyDeviceToHost, c->stream));
        TA_HIP(hipStreamSynchronize(c->stream));
    }
    return TA_OK;
}

TA_API int ta_sighist_debug(ta_ctx* c, uint32_t out[4]) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    const bool hist = c->sh.last == 1 && pass_current(c, c->sh.hist_seq), rank = c->sh.last == 2 && pass_current(c, c->sh.rank_seq);
    if (!hist && !rank) return fail(TA_EINVAL, NO_HIST);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    uint32_t spills = 0;
    if ((rc = hist ? digits_finish(c, c->sh.out.p, 1, &spills) : digits_finish(c, c->sh.rank.p, c->sh.rank_passes, &spills)) != TA_OK) return rc;
    if (out) { out[0] = spills; out[1] = 0; out[2] = c->sh.plan.tiles_per_group; out[3] = c->sh.plan.groups; }
    return TA_OK;
}

TA_API int ta_sighist_timing(ta_ctx* c, double* ms_hist, double* ms_rank) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    const bool hist = pass_current(c, c->sh.hist_seq), rank = pass_current(c, c->sh.rank_seq);
    if (!hist && !rank) return fail(TA_EINVAL, NO_HIST);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double h = nan, r = nan;
    if (hist && (rc = interval_ms(c->sh.ev[0], c->sh.ev[1], &h)) != TA_OK) return rc;
    if (rank && (rc = interval_ms(c->sh.ev[2], c->sh.ev[3], &r)) != TA_OK) return rc;
    if (ms_hist) *ms_hist = h;
    if (ms_rank) *ms_rank = r;
    return TA_OK;
}

}  // extern "C"
