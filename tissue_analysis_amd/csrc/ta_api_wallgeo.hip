// ta_api_wallgeo.hip -- the C ABI of include/tissue_scan_wallgeo.h on top of kernels_wallgeo.hip.
#include "../../include/tissue_scan_wallgeo.h"
#include "ta_ctx.h"
#include "ta_wallgeo.h"

namespace {

const char* const NO_ROWS = "no wall-geometry rows for the current extraction (run ta_wallgeo_extract)";

bool wallgeo_current(const ta_ctx* c) { return pass_current(c, c->wg.seq) && !c->exchanged; }

// the parts of WallGeoState::out for P pairs
struct WallGeoLayout {
    Part flags, rows;
    uint64_t bytes = 0;
    constexpr explicit WallGeoLayout(uint64_t P) {
        PartCursor at;
        flags = at.take(16); rows = at.take(P * ta::WG_ROW * 8);
        bytes = at.end();
    }
};
static_assert(ta::WG_ROW == 15 && WallGeoLayout(2).rows.at == 16 && WallGeoLayout(2).bytes == 256, "flags u32[4] | rows u64[P][15]");

// drain the stream and look at the pass's flag words
int wallgeo_finish(ta_ctx* c, uint32_t* spills) {
    uint32_t flags[ta::WG_NFLAGS] = {0, 0, 0, 0};
    if (const int rc = read_pass_flags<ta::WG_NFLAGS>(c, c->wg.out.p, flags); rc != TA_OK) return rc;
    if (flags[ta::WG_FLAG_PAIR_MISS]) return fail(TA_ERANGE, "the wall-geometry pass met a pair the extraction does not hold (the volume changed since ta_extract)");
    if (spills) *spills = flags[ta::WG_FLAG_SPILL];
    return TA_OK;
}

}  // namespace

// a new label volume: the rows are stale
void wallgeo_on_new_volume(ta_ctx* c) { c->wg.seq = 0; }

extern "C" {

TA_API int ta_wallgeo_extract(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->vol) return fail(TA_EINVAL, "no label volume set");
    int rc = extraction_preflight(c, "wall-geometry pass");
    if (rc != TA_OK) return rc;
    if (!(c->feature_mask & TA_F_ADJACENCY)) return fail(TA_EINVAL, "the wall-geometry pass needs an extraction with TA_F_ADJACENCY");
    if (c->exchanged) return fail(TA_EINVAL, "the wall-geometry pass needs this context's own pair list (not a merged one)");
    c->wg.seq = 0;
    // 3 nvox (2 E)^2 < 2^64, E the largest global extent: no sum of the pass can wrap
    {
        const int64_t owned = c->mdims[0] - c->first_owned;
        const long double e = (long double)std::max(std::max(c->a_origin + owned, c->mdims[1]), c->mdims[2]);
        const long double nvox = (long double)owned * (long double)c->mdims[1] * (long double)c->mdims[2];
        if (3.0L * nvox * 4.0L * e * e >= 18446744073709551616.0L)
            return fail(TA_ERANGE, "the second sums of a wall of this volume may not fit 64 bits (3 nvox (2 extent)^2 >= 2^64)");
    }
    const uint64_t P = (uint64_t)c->npairs;
    const WallGeoLayout L(P);
    if ((rc = c->wg.out.reserve(L.bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->wg.ev)) != TA_OK) return rc;
    ta::WallGeoArgs a = {};
    if (P && (rc = build_pair_index(c, c->wg.hash, &a.hkeys, &a.hrows, &a.hmask)) != TA_OK) return rc;
    char* o = (char*)c->wg.out.p;
    TA_HIP(hipMemsetAsync(o, 0, L.bytes, c->stream));
    a.vol = sweep_vol(c);
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.first_owned = c->first_owned;
    a.origin0 = c->a_origin - c->first_owned;
    a.rows = (unsigned long long*)(o + L.rows.at);
    a.flags = (uint32_t*)o;
    TA_HIP(hipEventRecord(c->wg.ev[0], c->stream));
    // (a volume of one label has no pair and no row to add to: nothing to launch)
    c->wg.plan = P ? ta::launch_wallgeo(c->stream, a, c->itemsize) : ta::RangePlan();
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->wg.ev[1], c->stream));
    c->wg.seq = c->extract_seq;
    c->wg.npairs = (int64_t)P;
    return TA_OK;
}

TA_API int ta_wallgeo_get(ta_ctx* c, uint64_t* fwd, uint64_t* rev, uint64_t* sum1, uint64_t* sum2) {
    int rc = results_ready(c, wallgeo_current, NO_ROWS);
    if (rc != TA_OK || (rc = wallgeo_finish(c, nullptr)) != TA_OK) return rc;
    const uint64_t P = (uint64_t)c->wg.npairs;
    if (!P || (!fwd && !rev && !sum1 && !sum2)) return TA_OK;
    std::vector<uint64_t> h;
    try { h.resize(P * ta::WG_ROW); } catch (...) { return fail(TA_ENOMEM, "no host memory for %llu wall rows", (unsigned long long)P); }
    if ((rc = read_columns(c, c->wg.out.p, {{h.data(), WallGeoLayout(P).rows}})) != TA_OK) return rc;
    // the device rows are in memory-axis order: to array axes
    int slot[6];
    moment_slots(c, slot);
    for (uint64_t i = 0; i < P; ++i) {
        const uint64_t* r = h.data() + i * ta::WG_ROW;
        for (int k = 0; k < 3; ++k) {
            if (fwd) fwd[3 * i + c->perm[k]] = r[k];
            if (rev) rev[3 * i + c->perm[k]] = r[3 + k];
            if (sum1) sum1[3 * i + c->perm[k]] = r[6 + k];
        }
        if (sum2) for (int q = 0; q < 6; ++q) sum2[6 * i + slot[q]] = r[9 + q];
    }
    return TA_OK;
}

TA_API int ta_wallgeo_spills(ta_ctx* c, uint32_t* spills) {
    const int rc = results_ready(c, wallgeo_current, NO_ROWS);
    return rc != TA_OK ? rc : wallgeo_finish(c, spills);
}

TA_API int ta_wallgeo_debug(ta_ctx* c, uint32_t out[4]) {
    uint32_t spills = 0;
    int rc = results_ready(c, wallgeo_current, NO_ROWS);
    if (rc != TA_OK || (rc = wallgeo_finish(c, &spills)) != TA_OK) return rc;
    range_debug_words(out, spills, 0, c->wg.plan);
    return TA_OK;
}

TA_API int ta_wallgeo_timing(ta_ctx* c, double* ms) {
    return pass_timing(c, ms, [](ta_ctx* c) { return c->wg.seq != 0 && c->wg.ev[1] ? c->wg.ev : nullptr; }, "no wall-geometry pass has been run");
}

}  // extern "C"
