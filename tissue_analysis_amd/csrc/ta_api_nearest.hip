// ta_api_nearest.hip -- the C ABI of include/tissue_scan_nearest.h on top of kernels_nearest.hip.
#include "../../include/tissue_scan_nearest.h"
#include "ta_ctx.h"

namespace {

const char* const NO_RESULTS = "no nearest-label map for the current extraction (run ta_nearest_extract)";

// the parts of NearestState::table for R rows
struct NearestLayout {
    Part gained, totals, flags;
    uint64_t bytes = 0;
    constexpr explicit NearestLayout(uint64_t R) {
        PartCursor at;
        gained = at.take(8 * R); totals = at.take(16); flags = at.take(4 * ta::NEAR_NFLAGS);
        bytes = at.end();
    }
};
static_assert(NearestLayout(3).totals.at == 24 && NearestLayout(3).flags.at == 40 && NearestLayout(3).bytes == 56, "gained [R] | totals [2] | flags u32[4]");

bool nearest_current(const ta_ctx* c) { return pass_current(c, c->near.seq); }

}  // namespace

// a new label volume (or new label values in it): the images and the counts are stale
void nearest_on_new_volume(ta_ctx* c) { c->near.seq = 0; }

extern "C" {

TA_API int ta_nearest_set_batch(ta_ctx* c, int64_t columns) {
    const int rc = check_batch_option(c, columns);
    if (rc == TA_OK) c->near.opt_batch = columns;
    return rc;
}

TA_API int ta_nearest_extract(ta_ctx* c, uint32_t empty_label, uint32_t not_from_label, const double spacing[3], double max_d2, uint32_t flags) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (flags & ~TA_NEAREST_NOT_FROM) return fail(TA_EINVAL, "bad nearest-label flags 0x%x", flags);
    ta::NearestArgs a = {};
    int rc = check_spacing(spacing);
    if (rc != TA_OK) return rc;
    if (!(max_d2 >= 0.0)) return fail(TA_EINVAL, "max_d2=%g is negative or not a number", max_d2);
    if ((rc = transform_preflight(c, "nearest-label pass", spacing, a.w)) != TA_OK) return rc;
    c->near.seq = 0;
    const uint64_t nvox = voxels(c), R = (uint64_t)c->max_label + 1;
    const NearestLayout L(R);

    a.vol = sweep_vol(c);
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.max_d2 = max_d2;
    a.has_empty = stored_label(c, empty_label, &a.empty);
    if (flags & TA_NEAREST_NOT_FROM) a.has_not_from = stored_label(c, not_from_label, &a.not_from);

    const ta::BatchPlan plan = ta::plan_batches(c->mdims, c->near.opt_batch, ta::NEAR_STACK_ENTRY, ta::NEAR_WORK_CAP);
    if ((rc = c->near.f.reserve(nvox * 8)) != TA_OK) return rc;
    if ((rc = c->near.lab.reserve(nvox * 4)) != TA_OK) return rc;
    if ((rc = c->near.work.reserve(plan.work)) != TA_OK) return rc;
    if ((rc = c->near.table.reserve(L.bytes)) != TA_OK) return rc;
    if ((rc = ensure_events(c->near.ev)) != TA_OK) return rc;
    a.f = (double*)c->near.f.p;
    a.lab = (uint32_t*)c->near.lab.p;

    TA_HIP(hipEventRecord(c->near.ev[0], c->stream));
    uint32_t launched[4] = {0, 0, 0, 0};
    launched[0] = ta::launch_nearest_rows(c->stream, a, c->itemsize);
    for (int k = 0; k < 2; ++k) {                   // along memory axis 1, then 0
        const uint64_t columns = ta::column_pass(a.n0, a.n1, a.n2, 1 - k).columns, batch = plan.batch[k];
        for (uint64_t first = 0; first < columns; first += batch, ++launched[3])
            ta::launch_nearest_columns(c->stream, a, 1 - k, first, std::min(batch, columns - first), c->near.work.p, batch);
    }
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->near.ev[1], c->stream));
    char* tp = (char*)c->near.table.p;
    ta::NearestTable t = {};
    t.gained = (unsigned long long*)(tp + L.gained.at); t.totals = (unsigned long long*)(tp + L.totals.at); t.flags = (uint32_t*)(tp + L.flags.at);
    t.max_label = c->max_label;
    TA_HIP(hipMemsetAsync(tp, 0, L.bytes, c->stream));
    launched[1] = ta::launch_nearest_count(c->stream, a, c->itemsize, t);
    launched[2] = ta::nearest_voxel_groups(a);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->near.ev[2], c->stream));
    std::copy(launched, launched + 4, c->near.launched);
    c->near.args = a;
    c->near.seq = c->extract_seq;
    c->near.rows = (uint32_t)R;
    return TA_OK;
}

TA_API int ta_nearest_get(ta_ctx* c, uint64_t* gained, uint64_t totals[2]) {
    int rc = results_ready(c, nearest_current, NO_RESULTS);
    if (rc != TA_OK) return rc;
    const NearestLayout L(c->near.rows);
    uint32_t flags[ta::NEAR_NFLAGS] = {0, 0, 0, 0};
    if ((rc = read_columns(c, c->near.table.p, {{flags, L.flags}, {gained, L.gained}, {totals, L.totals}})) != TA_OK) return rc;
    if (flags[ta::NEAR_FLAG_RANGE])
        return fail(TA_ERANGE, "the nearest-label pass met a label above max_label=%u (the volume changed since ta_extract)", c->max_label);
    return TA_OK;
}

TA_API int ta_nearest_image(ta_ctx* c, int64_t first_plane, int64_t nplanes, uint32_t* nearest, double* d2) {
    int rc = results_ready(c, nearest_current, NO_RESULTS);
    if (rc != TA_OK) return rc;
    if ((rc = check_planes(c, first_plane, nplanes)) != TA_OK || !nplanes) return rc;
    const uint64_t plane = (uint64_t)c->mdims[1] * (uint64_t)c->mdims[2], from = (uint64_t)first_plane * plane, count = (uint64_t)nplanes * plane;
    if (nearest) TA_HIP(hipMemcpyAsync(nearest, (const uint32_t*)c->near.lab.p + from, count * 4, hipMemcpyDeviceToHost, c->stream));
    if (d2) TA_HIP(hipMemcpyAsync(d2, (const double*)c->near.f.p + from, count * 8, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    if (nearest && c->ids.compact) {                // ranks -> ids
        const auto& ids = c->ids.h_ids;
        for (uint64_t v = 0; v < count; ++v)
            if (nearest[v] < ids.size()) nearest[v] = ids[nearest[v]];
    }
    return TA_OK;
}

TA_API int ta_nearest_apply(ta_ctx* c) {
    int rc = results_ready(c, nearest_current, NO_RESULTS);
    if (rc != TA_OK) return rc;
    const bool compact = c->ids.compact;
    (void)ta::launch_nearest_apply(c->stream, c->near.args, c->itemsize, const_cast<void*>(c->vol), compact ? c->ids.compact_vol.p : nullptr,
                                   compact ? (const uint32_t*)c->ids.census_ids.p : nullptr, compact ? (uint32_t)c->ids.census_n : 0u);
    TA_HIP(hipGetLastError());
    volume_labels_changed(c);
    return TA_OK;
}

TA_API int ta_nearest_debug(ta_ctx* c, uint32_t out[4]) {
    int rc = results_ready(c, nearest_current, NO_RESULTS);
    if (rc != TA_OK) return rc;
    if (out) std::copy(c->near.launched, c->near.launched + 4, out);
    return TA_OK;
}

TA_API int ta_nearest_timing(ta_ctx* c, double* ms_pass, double* ms_after) {
    int rc = results_ready(c, nearest_current, NO_RESULTS);
    return rc != TA_OK ? rc : two_intervals_ms(c->near.ev, ms_pass, ms_after);
}

}  // extern "C"
