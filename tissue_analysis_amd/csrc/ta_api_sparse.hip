// ta_api_sparse.hip -- sparse label ids (census, compaction into ranks, re-rank) and the max-label pass of include/tissue_scan.h
// on top of kernels_census.hip.
#include "ta_ctx.h"

namespace {
// census of `ids` (host, ascending, unique; NULL: of the resident volume itself) on the context; leaves census_n / census_ids
int build_census(ta_ctx* c, const uint32_t* ids, uint32_t n_ids) {
    int rc;
    const uint64_t nvox = (uint64_t)c->mdims[0] * c->mdims[1] * c->mdims[2];
    uint32_t top = 0, listed = 0;
    uint64_t cap = 0;
    bool have_list = false;
    DevBuf& list = c->ids.census_list;                      // (kept: allocating and freeing it costs more than the pass it saves)
    if (ids) {
        for (uint32_t i = 1; i < n_ids; ++i)
            if (ids[i] <= ids[i - 1]) return fail(TA_EINVAL, "ids must be ascending and unique (ids[%u]=%u after %u)", i, ids[i], ids[i - 1]);
        top = n_ids ? ids[n_ids - 1] : 0u;
    } else if (c->ids.vol_max >= 0 && c->vol == c->owned_vol.p) {
        top = (uint32_t)c->ids.vol_max;                     // (ta_volume_max_label has been here, and only this library writes
                                                        //  a volume it uploaded itself: no second pass)
    } else {
        // ONE pass over the voxels where the maximum is not known: the workgroups' label sets go to a list, the list gives the
        // maximum (the table's size) and is marked afterwards -- a few hundred thousand entries against a second read of the volume
        cap = ta::census_list_capacity(nvox);
        const uint32_t parts = ta::census_list_parts();
        if (list.reserve(ta::census_list_head_bytes() + (uint64_t)parts * cap * 4) == TA_OK) {
            TA_HIP(hipMemsetAsync(list.p, 0, ta::census_list_head_bytes(), c->stream));
            if (ta::launch_census_list(c->stream, c->vol, c->itemsize, nvox, c->mdims[2], list.p, (uint32_t)cap)) {
                std::vector<uint32_t> head;
                try { head.resize(2 * (size_t)parts); } catch (...) { return fail(TA_ENOMEM, "out of host memory"); }
                TA_HIP(hipMemcpyAsync(head.data(), list.p, ta::census_list_head_bytes(), hipMemcpyDeviceToHost, c->stream));
                TA_HIP(hipStreamSynchronize(c->stream));
                have_list = true;
                for (uint32_t p = 0; p < parts; ++p) {
                    if (head[2 * p] > cap) have_list = false;
                    if (head[2 * p] > listed) listed = head[2 * p];
                    if (head[2 * p + 1] > top) top = head[2 * p + 1];
                }
                if (have_list) c->ids.vol_max = top; else top = 0;
            }
        }
        if (!have_list) {                               // (rows that are not whole vectors, or a volume of noise: the two passes)
            ta::launch_max_label(c->stream, c->vol, c->itemsize, nvox, maxlab_dev(c));
            TA_HIP(hipMemcpyAsync(&top, maxlab_dev(c), sizeof(top), hipMemcpyDeviceToHost, c->stream));
            TA_HIP(hipStreamSynchronize(c->stream));
            c->ids.vol_max = top;
        }
    }
    c->ids.census_n = -1;
    if ((rc = c->ids.census.reserve(ta::census_bytes(top))) != TA_OK) return rc;
    DevBuf scratch, staged;
    if ((rc = scratch.reserve(ta::census_scratch_bytes(top))) != TA_OK) return rc;
    hipError_t e = hipMemsetAsync(c->ids.census.p, 0, ta::census_bytes(top), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(scratch.p, 0, ta::census_scratch_bytes(top), c->stream);
    if (e == hipSuccess && ids && n_ids) {
        if ((rc = staged.reserve((uint64_t)n_ids * 4)) != TA_OK) { scratch.release(); return rc; }
        e = hipMemcpyAsync(staged.p, ids, (uint64_t)n_ids * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) ta::launch_census_from_ids(c->stream, (const uint32_t*)staged.p, n_ids, c->ids.census.p, scratch.p, top);
    } else if (e == hipSuccess && !ids && have_list) {
        ta::launch_census_from_list(c->stream, list.p, (uint32_t)cap, listed, c->ids.census.p, scratch.p, top);
    } else if (e == hipSuccess && !ids) {
        ta::launch_census_mark(c->stream, c->vol, c->itemsize, nvox, c->mdims[2], c->ids.census.p, scratch.p, top);
    }
    uint32_t* total_dev = nullptr;
    uint32_t total = 0;
    if (e == hipSuccess) {
        ta::launch_census_scan(c->stream, c->ids.census.p, top, scratch.p, nullptr, &total_dev);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&total, total_dev, sizeof(total), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && total) {
        rc = c->ids.census_ids.reserve((uint64_t)total * 4);
        if (rc != TA_OK) { scratch.release(); staged.release(); return rc; }
        ta::launch_census_scan(c->stream, c->ids.census.p, top, scratch.p, (uint32_t*)c->ids.census_ids.p, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    scratch.release();
    staged.release();
    if (e != hipSuccess) return fail(TA_EHIP, "label census: %s", hipGetErrorString(e));
    c->ids.census_max = top;
    c->ids.census_n = (int64_t)total;
    c->ids.census_of_volume = ids == nullptr;
    return TA_OK;
}
}  // namespace

// whenever the voxels change: the census ends, and a compacted context goes back to dense rows until it is compacted again
void sparse_on_new_volume(ta_ctx* c) {
    c->ids.census_n = -1;
    c->ids.census_of_volume = false;
    c->ids.rerank_check = false;
    c->ids.vol_max = -1;
    if (c->ids.compact) { c->ids.compact = false; c->extracted = c->checked = false; }
}

int rerank_verdict(ta_ctx* c, uint32_t status) {
    if (!c->ids.rerank_check) return TA_OK;
    c->ids.rerank_check = false;
    if (status) { c->extracted = false; return fail(TA_ERANGE, "the refreshed volume holds a label id that is not in the list the context was compacted with"); }
    return TA_OK;
}

int settle_rerank(ta_ctx* c) {
    if (!c->ids.rerank_check) return TA_OK;
    uint32_t status = 0;
    TA_HIP(hipMemcpyAsync(&status, maxlab_dev(c), sizeof(status), hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return rerank_verdict(c, status);
}

extern "C" {

TA_API int ta_volume_max_label(ta_ctx* c, uint32_t* max_label) {
    if (!c || !max_label) return fail(TA_EINVAL, "NULL argument");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint64_t nvox = (uint64_t)c->mdims[0] * c->mdims[1] * c->mdims[2];
    if ((rc = settle_rerank(c)) != TA_OK) return rc;
    ta::launch_max_label(c->stream, c->vol, c->itemsize, nvox, maxlab_dev(c));
    uint32_t v = 0;
    TA_HIP(hipMemcpyAsync(&v, maxlab_dev(c), sizeof(v), hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    TA_HIP(hipGetLastError());
    *max_label = v;
    c->ids.vol_max = v;
    return TA_OK;
}

TA_API int ta_volume_label_census(ta_ctx* c, uint32_t* max_label, uint32_t* n_present) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if (c->ids.compact) return fail(TA_EINVAL, "the context is compacted: its census is the one it was compacted with");
    if ((rc = build_census(c, nullptr, 0)) != TA_OK) return rc;
    if (max_label) *max_label = c->ids.census_max;
    if (n_present) *n_present = (uint32_t)c->ids.census_n;
    return TA_OK;
}

TA_API int ta_label_census_get(ta_ctx* c, uint32_t* ids) {
    if (!c || !ids) return fail(TA_EINVAL, "NULL argument");
    if (c->ids.census_n < 0) return fail(TA_EINVAL, "no label census on this context");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if (c->ids.census_n == 0) return TA_OK;
    TA_HIP(hipMemcpyAsync(ids, c->ids.census_ids.p, (uint64_t)c->ids.census_n * 4, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_volume_compact_labels(ta_ctx* c, const uint32_t* ids, uint32_t n_ids, uint32_t* n_rows) {
    if (!c || (!ids && n_ids)) return fail(TA_EINVAL, "NULL argument");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    c->ids.compact = false;
    c->ids.rerank_check = false;
    c->extracted = c->checked = false;
    if (ids || c->ids.census_n < 0 || !c->ids.census_of_volume)          // (ids == NULL means THIS volume's census: never a caller's list left behind)
        if ((rc = build_census(c, ids, n_ids)) != TA_OK) return rc;
    if (c->ids.census_n >= (1ll << 28)) return fail(TA_ERANGE, "%lld label ids are present: too many for per-label rows", (long long)c->ids.census_n);
    const uint64_t nvox = (uint64_t)c->mdims[0] * c->mdims[1] * c->mdims[2];
    if ((rc = c->ids.compact_vol.reserve(nvox * c->itemsize + 64)) != TA_OK) return rc;
    uint32_t status = 0;
    hipError_t e = hipMemsetAsync(maxlab_dev(c), 0, sizeof(uint32_t), c->stream);       // (the word is free between max-label passes)
    if (e == hipSuccess) {
        ta::launch_census_rank(c->stream, c->vol, c->ids.compact_vol.p, c->itemsize, nvox, c->ids.census.p, c->ids.census_max, maxlab_dev(c));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&status, maxlab_dev(c), sizeof(status), hipMemcpyDeviceToHost, c->stream);
    try { c->ids.h_ids.resize((size_t)c->ids.census_n); } catch (...) { return fail(TA_ENOMEM, "out of host memory"); }
    if (e == hipSuccess && c->ids.census_n)
        e = hipMemcpyAsync(c->ids.h_ids.data(), c->ids.census_ids.p, (uint64_t)c->ids.census_n * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(TA_EHIP, "compact labels: %s", hipGetErrorString(e));
    if (status) return fail(TA_ERANGE, "the volume holds a label id that is not in the list it was to be compacted with");
    c->ids.compact = true;
    c->auto_tile_shift = 0;
    if (n_rows) *n_rows = (uint32_t)c->ids.census_n;
    return TA_OK;
}

TA_API int ta_volume_is_compact(ta_ctx* c, int* compact, uint32_t* n_rows) {
    if (!c || !compact) return fail(TA_EINVAL, "NULL argument");
    *compact = c->ids.compact ? 1 : 0;
    if (n_rows) *n_rows = c->ids.compact ? (uint32_t)c->ids.census_n : 0u;
    return TA_OK;
}

TA_API int ta_volume_rerank(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    if (!c->ids.compact) return fail(TA_EINVAL, "the context is not compacted");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint64_t nvox = (uint64_t)c->mdims[0] * c->mdims[1] * c->mdims[2];
    c->extracted = c->checked = false;
    // asynchronous on the context's stream: the "id not in the census" word travels to the host with the flags of the next
    // extraction, whose getters then answer TA_ERANGE
    hipError_t e = hipMemsetAsync(maxlab_dev(c), 0, sizeof(uint32_t), c->stream);
    if (e == hipSuccess) {
        ta::launch_census_rank(c->stream, c->vol, c->ids.compact_vol.p, c->itemsize, nvox, c->ids.census.p, c->ids.census_max, maxlab_dev(c));
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(TA_EHIP, "re-rank: %s", hipGetErrorString(e));
    c->ids.rerank_check = true;
    c->ids.vol_max = -1;
    junctions_on_new_volume(c);     // (the caller edited the labels in place)
    components_on_new_volume(c);
    return TA_OK;
}

TA_API int ta_volume_uncompact(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (c->ids.compact) {
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        c->ids.compact = false;
        c->ids.rerank_check = false;
        c->extracted = c->checked = false;
        c->ids.compact_vol.release();
        c->auto_tile_shift = 0;
    }
    return TA_OK;
}

}  // extern "C"
