// ta_api_signal.hip -- the C ABI of include/tissue_scan_signal.h on top of kernels_signal.hip.
#include "../../include/tissue_scan_signal.h"
#include "ta_ctx.h"
#include "ta_signal.h"

namespace {

constexpr CompanionKind SIGNAL = {"the signal", 1, 2};      // uint8 or uint16

// the parts of SignalState::out for R rows and P pairs
struct SignalLayout {
    Part flags, n, sum, sumsq, vmin, vmax, side_lo, side_hi;
    uint64_t bytes = 0;
    constexpr SignalLayout(uint64_t R, uint64_t P) {
        PartCursor at;
        flags = at.take(16); n = at.take(8 * R); sum = at.take(8 * R); sumsq = at.take(16 * R); vmin = at.take(4 * R); vmax = at.take(4 * R);
        side_lo = at.take(8 * P); side_hi = at.take(8 * P);
        bytes = at.end();
    }
};
static_assert(SignalLayout(3, 2).n.at == 16 && SignalLayout(3, 2).sumsq.at == 64 && SignalLayout(3, 2).vmin.at == 112 && SignalLayout(3, 2).vmax.at == 124 &&
              SignalLayout(3, 2).side_lo.at == 136 && SignalLayout(3, 2).side_hi.at == 152 && SignalLayout(3, 2).bytes == 168,
              "flags u32[4] | n [R] | sum [R] | sumsq [R][2] | min u32[R] | max u32[R] | side_lo [P] | side_hi [P]");

const char* const NO_LABELS = "no per-label signal results for the current extraction (run ta_signal_extract with TA_SIG_LABELS)";
const char* const NO_WALLS = "no per-wall signal results for the current extraction (run ta_signal_extract with TA_SIG_WALLS)";
bool signal_current(const ta_ctx* c) { return pass_current(c, c->sig.seq); }
bool signal_labels_current(const ta_ctx* c) { return signal_current(c) && (c->sig.what & TA_SIG_LABELS); }
bool signal_walls_current(const ta_ctx* c) { return signal_current(c) && (c->sig.what & TA_SIG_WALLS) && !c->exchanged; }

// drain the stream and look at the pass's flag words; spills: label records, pair records that missed a workgroup's LDS tables
int signal_finish(ta_ctx* c, uint32_t* spills = nullptr) {
    uint32_t flags[ta::SIG_NFLAGS] = {0, 0, 0, 0};
    if (const int rc = read_pass_flags<ta::SIG_NFLAGS>(c, c->sig.out.p, flags); rc != TA_OK) return rc;
    if (flags[ta::SIG_FLAG_RANGE]) return fail(TA_ERANGE, "the signal pass met a label above max_label=%u (the volume changed since ta_extract)", c->max_label);
    if (flags[ta::SIG_FLAG_PAIR_MISS]) return fail(TA_ERANGE, "the signal pass met a pair the extraction does not hold (the volume changed since ta_extract)");
    if (spills) { spills[0] = flags[ta::SIG_FLAG_LABEL_SPILL]; spills[1] = flags[ta::SIG_FLAG_PAIR_SPILL]; }
    return TA_OK;
}

}  // namespace

// pair -> row: an open-addressed table of the sorted pair list (ta_adjacency_get sorts it on the device once per extraction)
int build_pair_index(ta_ctx* c, DevBuf& into, const uint64_t** hkeys, const uint32_t** hrows, uint32_t* hmask) {
    const uint64_t P = (uint64_t)c->npairs;
    int rc = ta_adjacency_get(c, nullptr, nullptr, nullptr);
    if (rc != TA_OK) return rc;
    uint64_t cap = 64;
    while (cap < 2 * P) cap <<= 1;
    if (cap > (1ull << 32)) return fail(TA_EINVAL, "too many pairs (%llu)", (unsigned long long)P);
    if ((rc = into.reserve(cap * 12 + P * 8)) != TA_OK) return rc;
    uint64_t* keys = (uint64_t*)into.p;
    uint64_t* sorted = keys + cap;
    uint32_t* rows = (uint32_t*)(sorted + P);
    TA_HIP(hipMemsetAsync(keys, 0xff, cap * 8, c->stream));
    TA_HIP(hipMemcpyAsync(sorted, c->h_pairs.p, P * 8, hipMemcpyHostToDevice, c->stream));
    ta::launch_signal_hash(c->stream, sorted, P, keys, rows, (uint32_t)(cap - 1));
    *hkeys = keys; *hrows = rows; *hmask = (uint32_t)(cap - 1);
    return TA_OK;
}

// a new label volume: the signal results are stale (extracted is false); a signal of other dims is dropped
void signal_on_new_volume(ta_ctx* c) {
    c->sig.seq = 0;
    companion_on_new_volume(c, c->sig.img);
}

// the resample pass rewrites (or has moved) the buffer the signal was adopted from: its results are stale, a signal that is gone is dropped
void signal_on_resampled(ta_ctx* c, const void* buf, const void* now, int itemsize) {
    if (!buf || c->sig.img.p != buf || c->sig.img.owned.p) return;
    c->sig.seq = 0; profile_on_new_signal(c); sighist_on_new_signal(c); sigmom_on_new_signal(c); cosig_on_new_signal(c);
    if (now != buf || itemsize != c->sig.img.itemsize) { c->sig.img.p = nullptr; c->sig.img.itemsize = 0; }
}

extern "C" {

TA_API int ta_signal_set(ta_ctx* c, const void* host_ptr, int itemsize, const int64_t dims[3], const int64_t strides_bytes[3]) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    const int rc = companion_set_host(c, c->sig.img, SIGNAL, host_ptr, itemsize, dims, strides_bytes);
    if (rc == TA_OK) { c->sig.seq = 0; profile_on_new_signal(c); sighist_on_new_signal(c); sigmom_on_new_signal(c); cosig_on_new_signal(c); }     // (the results are stale only once a new signal is in place: deliberate, as inherited)
    return rc;
}

TA_API int ta_signal_set_device(ta_ctx* c, const void* dev_ptr, int itemsize) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    const int rc = companion_set_device(c, c->sig.img, SIGNAL, dev_ptr, itemsize);
    if (rc == TA_OK) { c->sig.seq = 0; profile_on_new_signal(c); sighist_on_new_signal(c); sigmom_on_new_signal(c); cosig_on_new_signal(c); }
    return rc;
}

TA_API int ta_signal_extract(ta_ctx* c, uint32_t what) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (what == 0 || (what & ~(TA_SIG_LABELS | TA_SIG_WALLS))) return fail(TA_EINVAL, "bad signal mask 0x%x", what);
    int rc = signal_pass_preflight(c, "signal pass");
    if (rc != TA_OK) return rc;
    const bool walls = what & TA_SIG_WALLS;
    if (walls && !(c->feature_mask & TA_F_ADJACENCY)) return fail(TA_EINVAL, "TA_SIG_WALLS needs an extraction with TA_F_ADJACENCY");
    if (walls && c->exchanged) return fail(TA_EINVAL, "TA_SIG_WALLS needs this context's own pair list (not a merged one)");
    const uint64_t R = (uint64_t)c->max_label + 1, P = walls ? (uint64_t)c->npairs : 0;
    const SignalLayout L(R, P);
    if ((rc = c->sig.out.reserve(L.bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->sig.ev)) != TA_OK) return rc;
    ta::SignalArgs a;
    a.hkeys = nullptr; a.hrows = nullptr; a.hmask = 0;
    if (walls && P) {
        if ((rc = build_pair_index(c, c->sig.hash, &a.hkeys, &a.hrows, &a.hmask)) != TA_OK) return rc;
    }
    char* o = (char*)c->sig.out.p;
    TA_HIP(hipMemsetAsync(o, 0, L.bytes, c->stream));
    TA_HIP(hipMemsetAsync(o + L.vmin.at, 0xff, L.vmin.bytes, c->stream));
    a.vol = sweep_vol(c);
    a.sig = c->sig.img.p;
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.first_owned = c->first_owned;
    a.max_label = c->max_label;
    a.n = (unsigned long long*)(o + L.n.at);
    a.sum = (unsigned long long*)(o + L.sum.at);
    a.sumsq = (unsigned long long*)(o + L.sumsq.at);
    a.vmin = (uint32_t*)(o + L.vmin.at);
    a.vmax = (uint32_t*)(o + L.vmax.at);
    a.side_lo = (unsigned long long*)(o + L.side_lo.at);
    a.side_hi = (unsigned long long*)(o + L.side_hi.at);
    a.flags = (uint32_t*)o;
    a.tiles_per_group = 0;
    TA_HIP(hipEventRecord(c->sig.ev[0], c->stream));
    c->sig.plan = ta::launch_signal(c->stream, a, c->itemsize, c->sig.img.itemsize, (what & TA_SIG_LABELS ? ta::SIG_LABELS : 0u) | (walls ? ta::SIG_WALLS : 0u));
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->sig.ev[1], c->stream));
    c->sig.seq = c->extract_seq;
    c->sig.what = what;
    c->sig.rows = (uint32_t)R;
    c->sig.npairs = (int64_t)P;
    return TA_OK;
}

TA_API int ta_signal_get_labels(ta_ctx* c, uint64_t* n, uint64_t* sum, uint64_t* sumsq, uint32_t* vmin, uint32_t* vmax) {
    int rc = results_ready(c, signal_labels_current, NO_LABELS);
    if (rc != TA_OK || (rc = signal_finish(c)) != TA_OK) return rc;
    const SignalLayout L(c->sig.rows, (uint64_t)c->sig.npairs);
    return read_columns(c, c->sig.out.p, {{n, L.n}, {sum, L.sum}, {sumsq, L.sumsq}, {vmin, L.vmin}, {vmax, L.vmax}});
}

TA_API int ta_signal_get_walls(ta_ctx* c, uint64_t* side_lo, uint64_t* side_hi) {
    int rc = results_ready(c, signal_walls_current, NO_WALLS);
    if (rc != TA_OK || (rc = signal_finish(c)) != TA_OK) return rc;
    const SignalLayout L(c->sig.rows, (uint64_t)c->sig.npairs);
    return read_columns(c, c->sig.out.p, {{side_lo, L.side_lo}, {side_hi, L.side_hi}});
}

TA_API int ta_signal_debug(ta_ctx* c, uint32_t out[4]) {
    uint32_t spills[2] = {0, 0};
    int rc = results_ready(c, signal_current, "no signal results for the current extraction (run ta_signal_extract)");
    if (rc != TA_OK || (rc = signal_finish(c, spills)) != TA_OK) return rc;
    range_debug_words(out, spills[0], spills[1], c->sig.plan);
    return TA_OK;
}

TA_API int ta_signal_timing(ta_ctx* c, double* ms) {
    return pass_timing(c, ms, [](ta_ctx* c) { return c->sig.seq != 0 && c->sig.ev[1] ? c->sig.ev : nullptr; }, "no signal pass has been run");
}

}  // extern "C"
