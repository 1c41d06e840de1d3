// ta_api_components.hip -- the C ABI of include/tissue_scan_components.h on top of kernels_components.hip.
#include "../../include/tissue_scan_components.h"
#include "ta_ctx.h"
#include "ta_components.h"

namespace {

const char* const NO_TABLES = "no component tables for the current volume (run ta_components_extract)";

// where the parts of ComponentState::slots lie, for S slots; [zero, fill) is zeroed, [fill, box) set to all ones, the box to 0x7F
struct ComponentSlots {
    uint64_t root, row, zero, n, sum1, fill, first, box, bytes;
    explicit ComponentSlots(uint64_t S) {
        PartCursor at;
        root = at.take(S * 4, 16).at;
        row = at.take(S * 4, 16).at;
        zero = n = at.take(S * 8, 16).at;
        sum1 = at.take(S * 24, 16).at;
        fill = first = at.take(S * 8, 16).at;
        box = at.take(S * 24, 16).at;
        bytes = at.end(16) + 16;
    }
    ta::ComponentStats stats(char* p) const {
        ta::ComponentStats t;
        t.n = (unsigned long long*)(p + n); t.sum1 = (unsigned long long*)(p + sum1);
        t.first = (unsigned long long*)(p + first); t.box = (int32_t*)(p + box);
        return t;
    }
};

// the columns of ComponentState::rows, each from a multiple of 16 with S rows of room; the parts are the first R rows of each
struct ComponentTable {
    Part label, n, first, bbox, sum1;
    uint64_t bytes = 0;
    constexpr ComponentTable(uint64_t S, uint64_t R) {
        PartCursor at;
        const auto column = [&](uint64_t row_bytes) { return Part{at.take(S * row_bytes, 16).at, R * row_bytes}; };
        label = column(4); n = column(8); first = column(12); bbox = column(24); sum1 = column(24);
        bytes = at.end(16) + 16;
    }
};
static_assert(ComponentTable(3, 2).n.at == 16 && ComponentTable(3, 2).first.at == 48 && ComponentTable(3, 2).bbox.at == 96 && ComponentTable(3, 2).sum1.at == 176 &&
              ComponentTable(3, 2).bytes == 272 && ComponentTable(3, 2).first.bytes == 24, "label u32 | n u64 | first i32[3] | bbox i32[6] | sum1 u64[3]");

ta::ComponentArgs component_args(ta_ctx* c) {
    ta::ComponentArgs a = {};
    a.vol = c->vol;                // (the ids as the caller stored them, never the rank copy of a compacted context)
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.parent = (uint32_t*)c->cc.parent.p;
    return a;
}

// drain the stream, read the slot count, allocate, hand out the slots, run the statistics, sort, write the table
int components_settle(ta_ctx* c) {
    if (c->cc.state == 2) return TA_OK;
    if (c->cc.state != 1) return fail(TA_EINVAL, NO_TABLES);
    c->cc.state = 0;                               // (whatever fails below: no tables)
    int rc;
    const uint64_t nvox = voxels(c), W = c->cc.waves;
    const ScanBlock w(W);                          // ComponentState::work: the root counts of the waves
    uint64_t S = 0;
    TA_HIP(w.read_total(c->stream, c->cc.work.p, &S));
    TA_HIP(hipStreamSynchronize(c->stream));
    const ComponentSlots q(S);
    const SortLayout sl(S, 8);
    const ComponentTable tb(S, S);
    if ((rc = c->cc.slots.reserve(q.bytes)) != TA_OK) return rc;
    if ((rc = c->cc.sort.reserve(sl.end + 16)) != TA_OK) return rc;
    if ((rc = c->cc.rows.reserve(tb.bytes)) != TA_OK) return rc;
    char* sp = (char*)c->cc.slots.p;
    uint32_t* parent = (uint32_t*)c->cc.parent.p;
    uint32_t* root_of_slot = (uint32_t*)(sp + q.root);
    const ta::ComponentStats stats = q.stats(sp);
    unsigned long long* nonempty = (unsigned long long*)c->cc.small.p;
    TA_HIP(hipMemsetAsync(nonempty, 0, 16, c->stream));
    TA_HIP(hipMemsetAsync(sp + q.zero, 0, q.fill - q.zero, c->stream));
    TA_HIP(hipMemsetAsync(sp + q.fill, 0xFF, q.box - q.fill, c->stream));
    TA_HIP(hipMemsetAsync(sp + q.box, 0x7F, q.bytes - 16 - q.box, c->stream));
    TA_HIP(hipEventRecord(c->cc.ev[3], c->stream));
    ta::launch_component_emit(c->stream, parent, nvox, w.offsets(c->cc.work.p), root_of_slot);
    ta::ComponentGeometry g = {};
    g.nvox = nvox;
    g.own_begin = (uint64_t)c->first_owned * (uint64_t)c->mdims[1] * (uint64_t)c->mdims[2];
    g.n1 = (uint32_t)c->mdims[1]; g.n2 = (uint32_t)c->mdims[2];
    ta::ComponentRows rows = {};
    for (int k = 0; k < 3; ++k) { rows.axis[k] = c->perm[k]; rows.dims[c->perm[k]] = c->mdims[k]; }
    array_key_strides(c, g.key_stride);
    ta::launch_component_stats(c->stream, parent, g, stats);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->cc.ev[4], c->stream));
    // the slots sorted by (label, first); those without an owned voxel sort behind every row
    SortView<uint64_t> v(sl, c->cc.sort.p);
    c->cc.launched[3] = ta::launch_component_keys(c->stream, c->vol, c->itemsize, root_of_slot, stats, S, v.keys(), v.idx(), nonempty);
    TA_HIP(v.sort(c->stream, S, 64));
    char* tp = (char*)c->cc.rows.p;
    rows.label = (uint32_t*)(tp + tb.label.at); rows.n = (unsigned long long*)(tp + tb.n.at);
    rows.first = (int32_t*)(tp + tb.first.at); rows.bbox = (int32_t*)(tp + tb.bbox.at); rows.sum1 = (unsigned long long*)(tp + tb.sum1.at);
    rows.origin0 = c->a_origin - c->first_owned;
    ta::launch_component_rows(c->stream, c->vol, c->itemsize, root_of_slot, stats, v.idx(), S, nonempty, (uint32_t*)(sp + q.row), rows);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->cc.ev[5], c->stream));
    uint64_t R = 0;
    TA_HIP(hipMemcpyAsync(&R, nonempty, 8, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    c->cc.nslots = S;
    c->cc.nrows = R;
    c->cc.state = 2;
    return TA_OK;
}

// the checks every function behind the extract shares; settles
int components_ready(ta_ctx* c) {
    const int rc = results_ready(c, [](const ta_ctx* c) { return c->cc.state != 0; }, NO_TABLES);
    return rc != TA_OK ? rc : components_settle(c);
}

}  // namespace

// a new label volume (or new label values in it): the component tables and the row image are stale
void components_on_new_volume(ta_ctx* c) { c->cc.state = 0; }

extern "C" {

TA_API int ta_components_extract(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->vol) return fail(TA_EINVAL, "no label volume set");
    const uint64_t nvox = voxels(c);
    if (nvox > ta::CC_MAX_VOXELS)
        return fail(TA_ERANGE, "%llu voxels in the buffer: the component pass takes at most 2^31 (cut the volume into slabs)", (unsigned long long)nvox);
    // (an axis holds at most 2^30 voxels: ta_volume_set.  The bounds are int32 and their minima start at 0x7F7F7F7F)
    if (c->a_origin - c->first_owned + c->mdims[0] > (int64_t)0x7F7F7F7F)
        return fail(TA_ERANGE, "a0_origin %lld + %lld planes: the global coordinates of the component table are int32 below 2139062143",
                    (long long)c->a_origin, (long long)c->mdims[0]);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    c->cc.state = 0;
    c->cc.waves = ta::component_waves(nvox);
    const ScanBlock w(c->cc.waves);
    if ((rc = c->cc.parent.reserve(nvox * 4 + 16)) != TA_OK) return rc;
    if ((rc = c->cc.work.reserve(w.end + 16)) != TA_OK) return rc;
    if ((rc = c->cc.small.reserve(16)) != TA_OK) return rc;
    if ((rc = ensure_events(c->cc.ev)) != TA_OK) return rc;
    const ta::ComponentArgs a = component_args(c);
    TA_HIP(hipEventRecord(c->cc.ev[0], c->stream));
    ta::launch_component_local(c->stream, a, c->itemsize);
    c->cc.launched[0] = (uint32_t)std::min<uint64_t>(ta::component_tiles(a), 0xFFFFFFFFull);
    c->cc.launched[1] = ta::launch_component_seams(c->stream, a, c->itemsize);
    c->cc.launched[2] = c->cc.launched[3] = 0u;
    ta::launch_component_flatten(c->stream, a.parent, nvox, a.n1, a.n2, w.counts(c->cc.work.p));
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->cc.ev[1], c->stream));
    w.scan(c->stream, c->cc.work.p);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->cc.ev[2], c->stream));
    c->cc.state = 1;
    return TA_OK;
}

TA_API int ta_components_size(ta_ctx* c, uint64_t* nrows) {
    int rc = components_ready(c);
    if (rc != TA_OK) return rc;
    if (nrows) *nrows = c->cc.nrows;
    return TA_OK;
}

TA_API int ta_components_get(ta_ctx* c, uint32_t* label, uint64_t* n, int32_t* first, int32_t* bbox, uint64_t* sum1) {
    int rc = components_ready(c);
    if (rc != TA_OK) return rc;
    if (!c->cc.nrows) return TA_OK;
    const ComponentTable tb(c->cc.nslots, c->cc.nrows);
    return read_columns(c, c->cc.rows.p, {{label, tb.label}, {n, tb.n}, {first, tb.first}, {bbox, tb.bbox}, {sum1, tb.sum1}});
}

TA_API int ta_components_image(ta_ctx* c, int64_t first_plane, int64_t nplanes, uint32_t* rows) {
    int rc = components_ready(c);
    if (rc != TA_OK) return rc;
    if ((rc = check_planes(c, first_plane, nplanes)) != TA_OK || !nplanes) return rc;
    if (!rows) return fail(TA_EINVAL, "rows is NULL");
    const uint64_t plane = (uint64_t)c->mdims[1] * (uint64_t)c->mdims[2], count = (uint64_t)nplanes * plane;
    if ((rc = c->cc.image.reserve(count * 4)) != TA_OK) return rc;
    const ComponentSlots q(c->cc.nslots);
    c->cc.launched[2] = ta::launch_component_image(c->stream, (const uint32_t*)c->cc.parent.p, (const uint32_t*)((const char*)c->cc.slots.p + q.row),
                                                   (uint64_t)first_plane * plane, count, (uint32_t*)c->cc.image.p);
    TA_HIP(hipGetLastError());
    TA_HIP(hipMemcpyAsync(rows, c->cc.image.p, count * 4, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_components_relabel(ta_ctx* c, const uint32_t* new_label, uint64_t nrows) {
    int rc = components_ready(c);
    if (rc != TA_OK) return rc;
    if (nrows != c->cc.nrows)
        return fail(TA_EINVAL, "%llu new labels for a table of %llu rows", (unsigned long long)nrows, (unsigned long long)c->cc.nrows);
    if (!new_label && nrows) return fail(TA_EINVAL, "new_label is NULL");
    if (c->itemsize == 2)
        for (uint64_t r = 0; r < nrows; ++r)
            if (new_label[r] > 0xFFFFu)
                return fail(TA_ERANGE, "new_label[%llu]=%u does not fit the uint16 volume", (unsigned long long)r, new_label[r]);
    if (nrows) {
        if ((rc = c->cc.image.reserve(nrows * 4)) != TA_OK) return rc;
        const ComponentSlots q(c->cc.nslots);
        TA_HIP(hipMemcpyAsync(c->cc.image.p, new_label, nrows * 4, hipMemcpyHostToDevice, c->stream));
        c->cc.launched[2] = ta::launch_component_relabel(c->stream, (const uint32_t*)c->cc.parent.p, (const uint32_t*)((const char*)c->cc.slots.p + q.row),
                                                         voxels(c), (const uint32_t*)c->cc.image.p, const_cast<void*>(c->vol), c->itemsize);
        TA_HIP(hipGetLastError());
        TA_HIP(hipStreamSynchronize(c->stream));   // (the caller's table may be freed after return)
    }
    volume_labels_changed(c);
    return TA_OK;
}

TA_API int ta_components_debug(ta_ctx* c, uint32_t out[4]) {
    int rc = components_ready(c);
    if (rc != TA_OK) return rc;
    if (out) std::copy(c->cc.launched, c->cc.launched + 4, out);
    return TA_OK;
}

TA_API int ta_components_timing(ta_ctx* c, double* ms_pass, double* ms_after) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (c->cc.state != 2) return fail(TA_EINVAL, "no settled component tables (ask ta_components_size first)");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    hipEvent_t* ev = c->cc.ev;                     // union-find + statistics | scan + the rest
    double pass = 0.0, after = 0.0;
    TA_HIP(summed_ms(ev[5], {{ev[0], ev[1]}, {ev[3], ev[4]}}, &pass));
    TA_HIP(summed_ms(ev[5], {{ev[1], ev[2]}, {ev[4], ev[5]}}, &after));
    if (ms_pass) *ms_pass = pass;
    if (ms_after) *ms_after = after;
    return TA_OK;
}

}  // extern "C"
