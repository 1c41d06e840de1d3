// ta_api_distance.hip -- the C ABI of include/tissue_scan_distance.h on top of kernels_distance.hip.
#include "../../include/tissue_scan_distance.h"
#include "ta_ctx.h"
#include "ta_distance.h"

#include <cmath>
#include <limits>

namespace {

const char* const NO_RESULTS = "no distance map for the current extraction (run ta_distance_extract)";

bool distance_current(const ta_ctx* c) { return c->dist.seq != 0 && c->extracted && c->dist.seq == c->extract_seq; }

uint64_t voxels(const ta_ctx* c) { return (uint64_t)c->mdims[0] * (uint64_t)c->mdims[1] * (uint64_t)c->mdims[2]; }

// byte offsets of the parts of DistanceState::table for R rows
struct DistanceLayout {
    uint64_t min2 = 0, max2, pole, flags, bytes;
    explicit DistanceLayout(uint64_t R) { max2 = 8 * R; pole = 16 * R; flags = 24 * R; bytes = flags + 4 * ta::DIST_NFLAGS; }
};

// columns of a launch along an axis of `len` voxels with `columns` columns: whole waves; what the option says, else what fits the cap
uint64_t batch_columns(const ta_ctx* c, uint64_t len, uint64_t columns) {
    const uint64_t b = c->dist.opt_batch > 0 ? ((uint64_t)c->dist.opt_batch + 63) / 64 * 64
                                             : std::max<uint64_t>(64, ta::DIST_WORK_CAP / (len * ta::DIST_STACK_ENTRY) / 64 * 64);
    return std::min(b, (columns + 63) / 64 * 64);
}

int distance_ready(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!distance_current(c)) return fail(TA_EINVAL, NO_RESULTS);
    return use_device(c);
}

}  // namespace

// a new label volume (or new label values in it): the image and the table are stale
void distance_on_new_volume(ta_ctx* c) { c->dist.seq = 0; }

extern "C" {

TA_API int ta_distance_set_batch(ta_ctx* c, int64_t columns) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (columns < 0 || columns > (1ll << 30)) return fail(TA_EINVAL, "the columns of a batch must be 0 (automatic) or in [1, 2^30]");
    c->dist.opt_batch = columns;
    return TA_OK;
}

TA_API int ta_distance_extract(ta_ctx* c, int mode, uint32_t site_label, const double spacing[3], uint32_t flags) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (mode != TA_DIST_OWN_WALL && mode != TA_DIST_FROM_LABEL) return fail(TA_EINVAL, "bad distance mode %d", mode);
    if (flags & ~TA_DIST_EDGE_IS_SITE) return fail(TA_EINVAL, "bad distance flags 0x%x", flags);
    if (!spacing) return fail(TA_EINVAL, "spacing is NULL");
    for (int k = 0; k < 3; ++k)
        if (!(spacing[k] > 0.0) || !std::isfinite(spacing[k])) return fail(TA_EINVAL, "spacing[%d]=%g is not positive and finite", k, spacing[k]);
    if (!c->vol) return fail(TA_EINVAL, "no label volume set");
    if (c->first_owned != 0 || c->a_origin != 0)
        return fail(TA_EINVAL, "the distance pass does not take a slab (an exact transform needs halos of unbounded depth)");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if (!c->extracted) return fail(TA_EINVAL, "the distance pass needs a ta_extract of the current volume first");
    if ((rc = finish_extract(c)) != TA_OK) return rc;
    c->dist.seq = 0;
    profile_on_new_distance(c);
    const uint64_t nvox = voxels(c), R = (uint64_t)c->max_label + 1;
    const DistanceLayout L(R);

    ta::DistanceArgs a = {};
    a.vol = sweep_vol(c);
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    for (int k = 0; k < 3; ++k) a.w[k] = spacing[c->perm[k]];
    a.mode = mode;
    a.flags = flags & TA_DIST_EDGE_IS_SITE ? ta::DIST_EDGE_IS_SITE : 0u;
    if (mode == TA_DIST_FROM_LABEL) {
        a.site = site_label;
        a.has_site = c->itemsize == 4 || site_label <= 0xFFFFu;
        if (c->ids.compact) {                       // the pass reads ranks: the id's rank, if the volume holds it
            const auto& ids = c->ids.h_ids;
            const auto it = std::lower_bound(ids.begin(), ids.end(), site_label);
            a.has_site = it != ids.end() && *it == site_label;
            a.site = (uint32_t)(it - ids.begin());
        }
    }

    uint64_t batch[2], work = 0;                    // [0]: along memory axis 1, [1]: along memory axis 0
    for (int k = 0; k < 2; ++k) {
        const int axis = 1 - k;
        const uint64_t len = (uint64_t)c->mdims[axis];
        batch[k] = batch_columns(c, len, ta::distance_columns(a, axis));
        work = std::max(work, len * batch[k] * ta::DIST_STACK_ENTRY);
    }
    if ((rc = c->dist.d2.reserve(nvox * 8)) != TA_OK) return rc;
    if ((rc = c->dist.work.reserve(work)) != TA_OK) return rc;
    if ((rc = c->dist.table.reserve(L.bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->dist.ev)) != TA_OK) return rc;
    a.d2 = (double*)c->dist.d2.p;

    TA_HIP(hipEventRecord(c->dist.ev[0], c->stream));
    ta::DistanceLaunch launched;
    launched.row_groups = ta::launch_distance_rows(c->stream, a, c->itemsize);
    for (int k = 0; k < 2; ++k) {
        const int axis = 1 - k;
        const uint64_t columns = ta::distance_columns(a, axis);
        for (uint64_t first = 0; first < columns; first += batch[k], ++launched.column_launches)
            ta::launch_distance_columns(c->stream, a, c->itemsize, axis, first, std::min(batch[k], columns - first), c->dist.work.p, batch[k]);
    }
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->dist.ev[1], c->stream));
    char* tp = (char*)c->dist.table.p;
    ta::DistanceTable t = {};
    t.min2 = (unsigned long long*)(tp + L.min2); t.max2 = (unsigned long long*)(tp + L.max2); t.pole = (unsigned long long*)(tp + L.pole);
    t.flags = (uint32_t*)(tp + L.flags);
    t.max_label = c->max_label;
    int64_t dims[3];
    for (int k = 0; k < 3; ++k) dims[c->perm[k]] = c->mdims[k];
    const uint64_t array_stride[3] = {(uint64_t)dims[1] * (uint64_t)dims[2], (uint64_t)dims[2], 1ull};
    for (int k = 0; k < 3; ++k) t.key_stride[k] = array_stride[c->perm[k]];
    ta::launch_distance_table(c->stream, a, c->itemsize, t, launched);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->dist.ev[2], c->stream));
    c->dist.launched = launched;
    c->dist.seq = c->extract_seq;
    c->dist.rows = (uint32_t)R;
    return TA_OK;
}

TA_API int ta_distance_get(ta_ctx* c, double* min2, double* max2, int32_t* pole) {
    int rc = distance_ready(c);
    if (rc != TA_OK) return rc;
    const uint64_t R = c->dist.rows;
    const DistanceLayout L(R);
    const char* tp = (const char*)c->dist.table.p;
    std::vector<uint64_t> key(R);
    std::vector<double> lo(min2 ? 0 : R), hi(max2 ? 0 : R);
    if (!min2) min2 = lo.data();
    if (!max2) max2 = hi.data();
    uint32_t flags[ta::DIST_NFLAGS] = {0, 0, 0, 0};
    TA_HIP(hipMemcpyAsync(flags, tp + L.flags, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipMemcpyAsync(min2, tp + L.min2, 8 * R, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipMemcpyAsync(max2, tp + L.max2, 8 * R, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipMemcpyAsync(key.data(), tp + L.pole, 8 * R, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    if (flags[ta::DIST_FLAG_RANGE])
        return fail(TA_ERANGE, "the distance pass met a label above max_label=%u (the volume changed since ta_extract)", c->max_label);
    int64_t dims[3];
    for (int k = 0; k < 3; ++k) dims[c->perm[k]] = c->mdims[k];
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
    int rc = distance_ready(c);
    if (rc != TA_OK) return rc;
    if (first_plane < 0 || nplanes < 0 || first_plane > c->mdims[0] || nplanes > c->mdims[0] - first_plane)
        return fail(TA_EINVAL, "planes %lld .. %lld are not inside the buffer's %lld", (long long)first_plane, (long long)(first_plane + nplanes),
                    (long long)c->mdims[0]);
    if (!nplanes) return TA_OK;
    if (!d2) return fail(TA_EINVAL, "d2 is NULL");
    const uint64_t plane = (uint64_t)c->mdims[1] * (uint64_t)c->mdims[2];
    TA_HIP(hipMemcpyAsync(d2, (const double*)c->dist.d2.p + (uint64_t)first_plane * plane, (uint64_t)nplanes * plane * 8, hipMemcpyDeviceToHost,
                          c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_distance_debug(ta_ctx* c, uint32_t out[4]) {
    int rc = distance_ready(c);
    if (rc != TA_OK) return rc;
    const ta::DistanceLaunch& l = c->dist.launched;
    if (out) { out[0] = l.row_groups; out[1] = l.voxel_groups; out[2] = l.init_groups; out[3] = l.column_launches; }
    return TA_OK;
}

TA_API int ta_distance_timing(ta_ctx* c, double* ms_pass, double* ms_after) {
    int rc = distance_ready(c);
    if (rc != TA_OK) return rc;
    TA_HIP(hipEventSynchronize(c->dist.ev[2]));
    double pass = 0.0, after = 0.0;
    if ((rc = elapsed_ms(c->dist.ev[0], c->dist.ev[1], &pass)) != TA_OK || (rc = elapsed_ms(c->dist.ev[1], c->dist.ev[2], &after)) != TA_OK) return rc;
    if (ms_pass) *ms_pass = pass;
    if (ms_after) *ms_after = after;
    return TA_OK;
}

}  // extern "C"
