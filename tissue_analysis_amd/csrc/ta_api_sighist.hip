// ta_api_sighist.hip -- the C ABI of include/tissue_scan_sighist.h on top of kernels_sighist.hip.
#include "../../include/tissue_scan_sighist.h"
#include "ta_ctx.h"
#include "ta_sighist.h"

#include <limits>

namespace {

static_assert(TA_SIGRANK_MAX_RANKS == ta::SH_MAX_RANKS, "the public header and the kernel disagree on the ranks of a row");

const char* const NO_HIST = "no signal histogram of the current extraction (run ta_sighist_extract)";
const char* const NO_RANK = "no order statistics of the current extraction (run ta_sigrank_extract)";

const char* const NOUN = "pass";
static_assert(ta::SH_NFLAGS == RANGE_NFLAGS && ta::SH_FLAG_RANGE == RANGE_FLAG_RANGE && ta::SH_FLAG_SPILL == RANGE_FLAG_SPILL,
              "range_pass_finish reads these words");

// the parts of SigHistState::out for R rows of B bins
struct HistLayout {
    Part flags, counts;
    uint64_t bytes = 0;
    constexpr HistLayout(uint64_t R, uint64_t B) {
        PartCursor at;
        flags = at.take(16); counts = at.take(8 * R * B);
        bytes = at.end();
    }
};
static_assert(HistLayout(3, 4).counts.at == 16 && HistLayout(3, 4).bytes == 112, "flags u32[4] | counts [R][B]");

// the parts of SigHistState::rank for R rows of n ranks; counts2 is empty unless the signal is uint16 (two digit passes)
struct RankLayout {
    Part flags, ranks, rem, hi, sel, map, values, counts1, counts2;
    uint64_t bytes = 0;
    constexpr RankLayout(uint64_t R, uint64_t n, bool two) {
        const uint64_t N = R * n;
        PartCursor at;
        flags = at.take(2 * sizeof(uint32_t) * ta::SH_NFLAGS); ranks = at.take(8 * N); rem = at.take(8 * N); hi = at.take(4 * N);
        sel = at.take(4 * N, 16); map = at.take(4 * N, 16); values = at.take(4 * N, 16);
        counts1 = at.take(8 * 256 * R, 16); counts2 = at.take(two ? 8 * 256 * N : 0);
        bytes = at.end();
    }
};
static_assert(RankLayout(3, 1, true).ranks.at == 32 && RankLayout(3, 1, true).hi.at == 80 && RankLayout(3, 1, true).sel.at == 96 &&
              RankLayout(3, 1, true).map.at == 112 && RankLayout(3, 1, true).values.at == 128 && RankLayout(3, 1, true).counts1.at == 144 &&
              RankLayout(3, 1, true).counts2.at == 6288 && RankLayout(3, 1, true).bytes == 12432 && RankLayout(3, 1, false).bytes == 6288,
              "flags u32[2][4] | ranks [N] | rem [N] | hi u32[N] | sel, map, values u32[N] and counts1 [R][256] from multiples of 16 | counts2 [N][256]");

bool hist_current(const ta_ctx* c) { return pass_current(c, c->sh.hist_seq); }
bool rank_current(const ta_ctx* c) { return pass_current(c, c->sh.rank_seq); }
// ta_sighist_debug answers for whichever table's digit pass ran last
bool last_current(const ta_ctx* c) { return c->sh.last == 1 ? hist_current(c) : c->sh.last == 2 && rank_current(c); }

ta::DigitArgs digit_args(const ta_ctx* c) {
    ta::DigitArgs a = {};
    a.vol = sweep_vol(c);
    a.sig = c->sig.img.p;
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.first_owned = c->first_owned;
    a.max_label = c->max_label;
    return a;
}

}  // namespace

// a new label volume (or new label values in it), a new signal: both tables are stale
void sighist_on_new_volume(ta_ctx* c) { c->sh.hist_seq = c->sh.rank_seq = 0; c->sh.last = 0; }
void sighist_on_new_signal(ta_ctx* c) { sighist_on_new_volume(c); }

extern "C" {

TA_API int ta_sighist_extract(ta_ctx* c, int log2_width) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = signal_pass_preflight(c, NOUN);
    if (rc != TA_OK) return rc;
    const int bits = 8 * c->sig.img.itemsize;
    if (log2_width < bits - 8 || log2_width > bits)
        return fail(TA_EINVAL, "log2_width=%d is not in [%d, %d] (1 .. 256 bins of a %d-bit signal)", log2_width, bits - 8, bits, bits);
    c->sh.hist_seq = 0;
    const uint64_t R = (uint64_t)c->max_label + 1, B = 1ull << (bits - log2_width);
    if (R * 256 > (1ull << 31)) return fail(TA_EINVAL, "too many keys: %llu rows x 256 > 2^31", (unsigned long long)R);
    const HistLayout L(R, B);
    if ((rc = c->sh.out.reserve(L.bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->sh.ev)) != TA_OK) return rc;
    char* o = (char*)c->sh.out.p;
    TA_HIP(hipMemsetAsync(o, 0, L.bytes, c->stream));
    ta::DigitArgs a = digit_args(c);
    a.shift = (uint32_t)log2_width;
    a.stride = (uint32_t)B;
    a.nsel = 0; a.sel = nullptr;
    a.counts = (unsigned long long*)(o + L.counts.at);
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
    int rc = results_ready(c, hist_current, NO_HIST);
    if (rc != TA_OK || (rc = range_pass_finish(c, c->sh.out.p, NOUN)) != TA_OK || !counts) return rc;
    return read_columns(c, c->sh.out.p, {{counts, HistLayout(c->sh.rows, c->sh.bins).counts}});
}

TA_API int ta_sigrank_extract(ta_ctx* c, int nranks, const uint64_t* ranks) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (nranks < 1 || nranks > TA_SIGRANK_MAX_RANKS) return fail(TA_EINVAL, "nranks=%d is not in [1, %d]", nranks, TA_SIGRANK_MAX_RANKS);
    if (!ranks) return fail(TA_EINVAL, "ranks is NULL");
    int rc = signal_pass_preflight(c, NOUN);
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
    TA_HIP(hipMemcpyAsync(o + L.ranks.at, c->sh.h_ranks.data(), L.ranks.bytes, hipMemcpyHostToDevice, c->stream));
    ta::SelectArgs sa = {};
    sa.rows = (uint32_t)R; sa.nranks = (uint32_t)nranks;
    sa.ranks = (const unsigned long long*)(o + L.ranks.at);
    sa.counts1 = (const unsigned long long*)(o + L.counts1.at);
    sa.counts2 = (const unsigned long long*)(o + L.counts2.at);
    sa.rem = (unsigned long long*)(o + L.rem.at);
    sa.hi = (uint32_t*)(o + L.hi.at); sa.sel = (uint32_t*)(o + L.sel.at); sa.map = (uint32_t*)(o + L.map.at); sa.values = (uint32_t*)(o + L.values.at);
    ta::DigitArgs a = digit_args(c);
    a.shift = two ? 8u : 0u;
    a.stride = 256;
    a.nsel = 0; a.sel = nullptr;
    a.counts = (unsigned long long*)(o + L.counts1.at);
    a.flags = (uint32_t*)o;
    TA_HIP(hipEventRecord(c->sh.ev[2], c->stream));
    c->sh.plan = ta::launch_sighist_digits(c->stream, a, c->itemsize, c->sig.img.itemsize);
    ta::launch_sighist_select_first(c->stream, sa, !two);
    if (two) {
        a.shift = 0;
        a.nsel = (uint32_t)nranks; a.sel = sa.sel;
        a.counts = (unsigned long long*)(o + L.counts2.at);
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
    int rc = results_ready(c, rank_current, NO_RANK);
    if (rc != TA_OK || (rc = range_pass_finish(c, c->sh.rank.p, NOUN, nullptr, c->sh.rank_passes)) != TA_OK || !values) return rc;
    return read_columns(c, c->sh.rank.p, {{values, RankLayout(c->sh.rank_rows, c->sh.nranks, c->sh.rank_passes == 2).values}});
}

TA_API int ta_sighist_debug(ta_ctx* c, uint32_t out[4]) {
    uint32_t spills = 0;
    int rc = results_ready(c, last_current, NO_HIST);
    if (rc != TA_OK) return rc;
    const bool hist = c->sh.last == 1;
    if ((rc = range_pass_finish(c, hist ? c->sh.out.p : c->sh.rank.p, NOUN, &spills, hist ? 1 : c->sh.rank_passes)) != TA_OK) return rc;
    range_debug_words(out, spills, 0, c->sh.plan);
    return TA_OK;
}

TA_API int ta_sighist_timing(ta_ctx* c, double* ms_hist, double* ms_rank) {
    int rc = results_ready(c, [](const ta_ctx* c) { return hist_current(c) || rank_current(c); }, NO_HIST);
    if (rc != TA_OK) return rc;
    const bool hist = hist_current(c), rank = rank_current(c);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double h = nan, r = nan;
    if (hist && (rc = interval_ms(c->sh.ev[0], c->sh.ev[1], &h)) != TA_OK) return rc;
    if (rank && (rc = interval_ms(c->sh.ev[2], c->sh.ev[3], &r)) != TA_OK) return rc;
    if (ms_hist) *ms_hist = h;
    if (ms_rank) *ms_rank = r;
    return TA_OK;
}

}  // extern "C"
