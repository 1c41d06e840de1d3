// ta_api_extents.hip -- the C ABI of include/tissue_scan_extents.h on top of kernels_extents.hip.
#include "../../include/tissue_scan_extents.h"
#include "ta_ctx.h"
#include "ta_extents.h"

#include <cfloat>

namespace {

const char* const NO_ROWS = "no extents of the current extraction (run ta_extents_extract)";
const char* const NOUN = "extent pass";
static_assert(ta::EX_NFLAGS == RANGE_NFLAGS && ta::EX_FLAG_RANGE == RANGE_FLAG_RANGE && ta::EX_FLAG_SPILL == RANGE_FLAG_SPILL,
              "range_pass_finish reads these words");

// the parts of ExtentState::out for R rows
struct ExtentLayout {
    Part flags, lo, hi;
    uint64_t bytes = 0;
    constexpr explicit ExtentLayout(uint64_t R) {
        PartCursor at;
        flags = at.take(16); lo = at.take(24 * R); hi = at.take(24 * R);
        bytes = at.end();
    }
};
static_assert(ExtentLayout(3).lo.at == 16 && ExtentLayout(3).hi.at == 88 && ExtentLayout(3).bytes == 160, "flags u32[4] | lo [R][3] | hi [R][3]");

bool extents_current(const ta_ctx* c) { return pass_current(c, c->ex.seq); }

// the keys a getter read into `v`, as the float64 they stand for
void decode_keys(double* v, uint64_t count) {
    if (!v) return;
    for (uint64_t i = 0; i < count; ++i) {
        uint64_t k;
        std::memcpy(&k, v + i, 8);
        v[i] = ta::extent_of_key(k);
    }
}

}  // namespace

// a new label volume (or new label values in it): the rows are stale
void extents_on_new_volume(ta_ctx* c) { c->ex.seq = 0; }

extern "C" {

TA_API int ta_extents_extract(ta_ctx* c, const double* weights, uint32_t rows) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!weights) return fail(TA_EINVAL, "weights is NULL");
    if (!c->vol) return fail(TA_EINVAL, "no label volume set");
    if (c->first_owned != 0 || c->a_origin != 0)
        return fail(TA_EINVAL, "the extent pass does not take a slab (its coordinates count from the volume's first plane)");
    int rc = extraction_preflight(c, NOUN);
    if (rc != TA_OK) return rc;
    const uint64_t R = (uint64_t)c->max_label + 1;
    if ((uint64_t)rows != R) return fail(TA_EINVAL, "weights for %u rows, the extraction has %llu", rows, (unsigned long long)R);
    // three terms of at most DBL_MAX / 4 each: no projection overflows, none is NaN
    const double most = DBL_MAX / (4.0 * (double)std::max<int64_t>(std::max(c->mdims[0], c->mdims[1]), std::max<int64_t>(c->mdims[2], 1)));
    for (uint64_t i = 0; i < 9 * R; ++i) {
        if (!std::isfinite(weights[i])) return fail(TA_EINVAL, "weights[%llu][%d][%d] is not finite", (unsigned long long)(i / 9), (int)(i / 3 % 3), (int)(i % 3));
        if (std::fabs(weights[i]) > most)
            return fail(TA_EINVAL, "weights[%llu][%d][%d]=%g: a projection could overflow", (unsigned long long)(i / 9), (int)(i / 3 % 3), (int)(i % 3), weights[i]);
    }
    c->ex.seq = 0;
    const ta::RangePlan plan = ta::extents_plan(c->mdims, c->itemsize);
    const ExtentLayout L(R);
    if ((rc = c->ex.out.reserve(L.bytes)) != TA_OK || (rc = c->ex.weights.reserve(72 * R)) != TA_OK) return rc;
    if ((rc = ensure_events(c->ex.ev)) != TA_OK) return rc;
    TA_HIP(hipStreamSynchronize(c->stream));               // (a pass in flight may still be fed from h_weights)
    if ((rc = host_alloc([&] { c->ex.h_weights.assign(weights, weights + 9 * R); })) != TA_OK) return rc;
    char* o = (char*)c->ex.out.p;
    TA_HIP(hipMemsetAsync(o, 0, L.flags.bytes, c->stream));
    TA_HIP(hipMemcpyAsync(c->ex.weights.p, c->ex.h_weights.data(), 72 * R, hipMemcpyHostToDevice, c->stream));
    ta::ExtentArgs a;
    a.vol = sweep_vol(c);
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.max_label = c->max_label;
    a.weights = (const double*)c->ex.weights.p;
    a.lo = (unsigned long long*)(o + L.lo.at);
    a.hi = (unsigned long long*)(o + L.hi.at);
    a.flags = (uint32_t*)o;
    a.tiles_per_group = 0;
    ta::launch_extents_fill(c->stream, a.lo, a.hi, 3 * R);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->ex.ev[0], c->stream));
    ta::launch_extents(c->stream, a, c->itemsize, plan);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->ex.ev[1], c->stream));
    c->ex.plan = plan;
    c->ex.seq = c->extract_seq;
    c->ex.rows = (uint32_t)R;
    return TA_OK;
}

TA_API int ta_extents_get(ta_ctx* c, double* lo, double* hi) {
    int rc = results_ready(c, extents_current, NO_ROWS);
    if (rc != TA_OK || (rc = range_pass_finish(c, c->ex.out.p, NOUN)) != TA_OK) return rc;
    const ExtentLayout L(c->ex.rows);
    if ((rc = read_columns(c, c->ex.out.p, {{lo, L.lo}, {hi, L.hi}})) != TA_OK) return rc;
    decode_keys(lo, 3ull * c->ex.rows);
    decode_keys(hi, 3ull * c->ex.rows);
    return TA_OK;
}

TA_API int ta_extents_debug(ta_ctx* c, uint32_t out[4]) {
    uint32_t spills = 0;
    int rc = results_ready(c, extents_current, NO_ROWS);
    if (rc != TA_OK || (rc = range_pass_finish(c, c->ex.out.p, NOUN, &spills)) != TA_OK) return rc;
    range_debug_words(out, spills, 0, c->ex.plan);
    return TA_OK;
}

TA_API int ta_extents_timing(ta_ctx* c, double* ms) {
    return pass_timing(c, ms, [](ta_ctx* c) { return c->ex.seq != 0 && c->ex.ev[1] ? c->ex.ev : nullptr; }, "no extent pass has been run");
}

}  // extern "C"
