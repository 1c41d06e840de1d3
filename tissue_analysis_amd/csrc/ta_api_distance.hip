// ta_api_distance.hip -- the C ABI of include/tissue_scan_distance.h on top of kernels_distance.hip.
#include "../../include/tissue_scan_distance.h"
#include "ta_ctx.h"
#include "ta_distance.h"

#include <limits>

namespace {

const char* const NO_RESULTS = "no distance map for the current extraction (run ta_distance_extract)";

// the parts of DistanceState::table for R rows
struct DistanceLayout {
    Part min2, max2, pole, flags;
    uint64_t bytes = 0;
    constexpr explicit DistanceLayout(uint64_t R) {
        PartCursor at;
        min2 = at.take(8 * R); max2 = at.take(8 * R); pole = at.take(8 * R); flags = at.take(4 * ta::DIST_NFLAGS);
        bytes = at.end();
    }
};
static_assert(DistanceLayout(3).max2.at == 24 && DistanceLayout(3).pole.at == 48 && DistanceLayout(3).flags.at == 72 && DistanceLayout(3).bytes == 88,
              "min2 [R] | max2 [R] | pole [R] | flags u32[4]");

bool distance_current(const ta_ctx* c) { return pass_current(c, c->dist.seq); }

}  // namespace

// a new label volume (or new label values in it): the image and the table are stale
void distance_on_new_volume(ta_ctx* c) { c->dist.seq = 0; }

extern "C" {

TA_API int ta_distance_set_batch(ta_ctx* c, int64_t columns) {
    const int rc = check_batch_option(c, columns);
    if (rc == TA_OK) c->dist.opt_batch = columns;
    return rc;
}

TA_API int ta_distance_extract(ta_ctx* c, int mode, uint32_t site_label, const double spacing[3], uint32_t flags) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (mode != TA_DIST_OWN_WALL && mode != TA_DIST_FROM_LABEL) return fail(TA_EINVAL, "bad distance mode %d", mode);
    if (flags & ~TA_DIST_EDGE_IS_SITE) return fail(TA_EINVAL, "bad distance flags 0x%x", flags);
    ta::DistanceArgs a = {};
    int rc = check_spacing(spacing);
    if (rc != TA_OK || (rc = transform_preflight(c, "distance pass", spacing, a.w)) != TA_OK) return rc;
    c->dist.seq = 0;
    profile_on_new_distance(c);
    const uint64_t nvox = voxels(c), R = (uint64_t)c->max_label + 1;
    const DistanceLayout L(R);

    a.vol = sweep_vol(c);
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.mode = mode;
    a.flags = flags & TA_DIST_EDGE_IS_SITE ? ta::DIST_EDGE_IS_SITE : 0u;
    if (mode == TA_DIST_FROM_LABEL) a.has_site = stored_label(c, site_label, &a.site);

    const ta::BatchPlan plan = ta::plan_batches(c->mdims, c->dist.opt_batch, ta::DIST_STACK_ENTRY, ta::DIST_WORK_CAP);
    if ((rc = c->dist.d2.reserve(nvox * 8)) != TA_OK) return rc;
    if ((rc = c->dist.work.reserve(plan.work)) != TA_OK) return rc;
    if ((rc = c->dist.table.reserve(L.bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->dist.ev)) != TA_OK) return rc;
    a.d2 = (double*)c->dist.d2.p;

    TA_HIP(hipEventRecord(c->dist.ev[0], c->stream));
    ta::DistanceLaunch launched;
    launched.row_groups = ta::launch_distance_rows(c->stream, a, c->itemsize);
    for (int k = 0; k < 2; ++k) {                   // along memory axis 1, then 0
        const uint64_t columns = ta::column_pass(a.n0, a.n1, a.n2, 1 - k).columns, batch = plan.batch[k];
        for (uint64_t first = 0; first < columns; first += batch, ++launched.column_launches)
            ta::launch_distance_columns(c->stream, a, c->itemsize, 1 - k, first, std::min(batch, columns - first), c->dist.work.p, batch);
    }
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->dist.ev[1], c->stream));
    char* tp = (char*)c->dist.table.p;
    ta::DistanceTable t = {};
    t.min2 = (unsigned long long*)(tp + L.min2.at); t.max2 = (unsigned long long*)(tp + L.max2.at); t.pole = (unsigned long long*)(tp + L.pole.at);
    t.flags = (uint32_t*)(tp + L.flags.at);
    t.max_label = c->max_label;
    array_key_strides(c, t.key_stride);
    ta::launch_distance_table(c->stream, a, c->itemsize, t, launched);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->dist.ev[2], c->stream));
    c->dist.launched = launched;
    c->dist.seq = c->extract_seq;
    c->dist.rows = (uint32_t)R;
    return TA_OK;
}

TA_API int ta_distance_get(ta_ctx* c, double* min2, double* max2, int32_t* pole) {
    int rc = results_ready(c, distance_current, NO_RESULTS);
    if (rc != TA_OK) return rc;
    const uint64_t R = c->dist.rows;
    const DistanceLayout L(R);
    std::vector<uint64_t> key;
    std::vector<double> lo, hi;
    if ((rc = host_alloc([&] { key.resize(R); lo.resize(min2 ? 0 : R); hi.resize(max2 ? 0 : R); })) != TA_OK) return rc;
    if (!min2) min2 = lo.data();
    if (!max2) max2 = hi.data();
    uint32_t flags[ta::DIST_NFLAGS] = {0, 0, 0, 0};
    if ((rc = read_columns(c, c->dist.table.p, {{flags, L.flags}, {min2, L.min2}, {max2, L.max2}, {key.data(), L.pole}})) != TA_OK) return rc;
    if (flags[ta::DIST_FLAG_RANGE])
        return fail(TA_ERANGE, "the distance pass met a label above max_label=%u (the volume changed since ta_extract)", c->max_label);
    int64_t dims[3];
    array_dims(c, dims);
    const uint64_t d1 = (uint64_t)dims[1], d2 = (uint64_t)dims[2];
    for (uint64_t r = 0; r < R; ++r) {
        const bool absent = key[r] == ta::DIST_NO_POLE;
        if (absent) min2[r] = max2[r] = std::numeric_limits<double>::infinity();
        if (pole) {
            pole[3 * r + 0] = absent ? -1 : (int32_t)(key[r] / (d1 * d2));
            pole[3 * r + 1] = absent ? -1 : (int32_t)(key[r] / d2 % d1);
            pole[3 * r + 2] = absent ? -1 : (int32_t)(key[r] % d2);
        }
    }
    return TA_OK;
}

TA_API int ta_distance_image(ta_ctx* c, int64_t first_plane, int64_t nplanes, double* d2) {
    int rc = results_ready(c, distance_current, NO_RESULTS);
    if (rc != TA_OK) return rc;
    if ((rc = check_planes(c, first_plane, nplanes)) != TA_OK || !nplanes) return rc;
    if (!d2) return fail(TA_EINVAL, "d2 is NULL");
    const uint64_t plane = (uint64_t)c->mdims[1] * (uint64_t)c->mdims[2];
    return read_columns(c, c->dist.d2.p, {{d2, Part{(uint64_t)first_plane * plane * 8, (uint64_t)nplanes * plane * 8}}});
}

TA_API int ta_distance_debug(ta_ctx* c, uint32_t out[4]) {
    int rc = results_ready(c, distance_current, NO_RESULTS);
    if (rc != TA_OK) return rc;
    const ta::DistanceLaunch& l = c->dist.launched;
    if (out) { out[0] = l.row_groups; out[1] = l.voxel_groups; out[2] = l.init_groups; out[3] = l.column_launches; }
    return TA_OK;
}

TA_API int ta_distance_timing(ta_ctx* c, double* ms_pass, double* ms_after) {
    int rc = results_ready(c, distance_current, NO_RESULTS);
    return rc != TA_OK ? rc : two_intervals_ms(c->dist.ev, ms_pass, ms_after);
}

}  // extern "C"
