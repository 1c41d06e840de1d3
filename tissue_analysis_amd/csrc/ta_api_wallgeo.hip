// ta_api_wallgeo.hip -- the C ABI of include/tissue_scan_wallgeo.h on top of kernels_wallgeo.hip.
#include "../../include/tissue_scan_wallgeo.h"
#include "ta_ctx.h"
#include "ta_wallgeo.h"

namespace {

bool wallgeo_current(const ta_ctx* c) { return pass_current(c, c->wg.seq) && !c->exchanged; }

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
    const uint64_t bytes = 16 + P * ta::WG_ROW * 8;
    if ((rc = c->wg.out.reserve(bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->wg.ev)) != TA_OK) return rc;
    ta::WallGeoArgs a = {};
    if (P && (rc = build_pair_index(c, c->wg.hash, &a.hkeys, &a.hrows, &a.hmask)) != TA_OK) return rc;
    char* o = (char*)c->wg.out.p;
    TA_HIP(hipMemsetAsync(o, 0, bytes, c->stream));
    a.vol = sweep_vol(c);
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.first_owned = c->first_owned;
    a.origin0 = c->a_origin - c->first_owned;
    a.rows = (unsigned long long*)(o + 16);
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
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!wallgeo_current(c)) return fail(TA_EINVAL, "no wall-geometry rows for the current extraction (run ta_wallgeo_extract)");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = wallgeo_finish(c, nullptr)) != TA_OK) return rc;
    const uint64_t P = (uint64_t)c->wg.npairs;
    if (!P || (!fwd && !rev && !sum1 && !sum2)) return TA_OK;
    std::vector<uint64_t> h;
    try { h.resize(P * ta::WG_ROW); } catch (...) { return fail(TA_ENOMEM, "no host memory for %llu wall rows", (unsigned long long)P); }
    TA_HIP(hipMemcpyAsync(h.data(), (const char*)c->wg.out.p + 16, P * ta::WG_ROW * 8, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    // the device rows are in memory-axis order: to array axes
    auto pair_slot = [](int x, int y) { if (x > y) std::swap(x, y); return x == 0 ? y : (x == 1 ? 2 + y : 5); };
    static const int mem_pair[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    int slot[6];
    for (int q = 0; q < 6; ++q) slot[q] = pair_slot(c->perm[mem_pair[q][0]], c->perm[mem_pair[q][1]]);
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
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!wallgeo_current(c)) return fail(TA_EINVAL, "no wall-geometry rows for the current extraction (run ta_wallgeo_extract)");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    return wallgeo_finish(c, spills);
}

TA_API int ta_wallgeo_debug(ta_ctx* c, uint32_t out[4]) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!wallgeo_current(c)) return fail(TA_EINVAL, "no wall-geometry rows for the current extraction (run ta_wallgeo_extract)");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    uint32_t spills = 0;
    if ((rc = wallgeo_finish(c, &spills)) != TA_OK) return rc;
    if (out) { out[0] = spills; out[1] = 0u; out[2] = c->wg.plan.tiles_per_group; out[3] = c->wg.plan.groups; }
    return TA_OK;
}

TA_API int ta_wallgeo_timing(ta_ctx* c, double* ms) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!ms) return fail(TA_EINVAL, "NULL argument");
    if (c->wg.seq == 0 || !c->wg.ev[1]) return fail(TA_EINVAL, "no wall-geometry pass has been run");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    return interval_ms(c->wg.ev[0], c->wg.ev[1], ms);
}

}  // extern "C"
