// ta_api_exchange.hip -- the rank-exchange entry points of include/tissue_scan.h: the accumulators and the pair list of an extraction
// handed to, and merged from, other ranks.
#include "ta_ctx.h"

extern "C" {

TA_API int ta_accumulators_reduced(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->extracted) return fail(TA_EINVAL, "no extraction has been run on this context");
    c->reduced = true;
    return TA_OK;
}

TA_API int ta_accumulators_device(ta_ctx* c, void** sums_dev, void** boxes_dev, uint32_t* max_label) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->extracted) return fail(TA_EINVAL, "no extraction has been run on this context");
    if (sums_dev) *sums_dev = c->sums;
    if (boxes_dev) *boxes_dev = c->boxes;
    if (max_label) *max_label = c->max_label;
    return TA_OK;
}

TA_API int ta_adjacency_device(ta_ctx* c, void** keys_dev, void** faces_dev, int64_t* npairs) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = finish_extract(c)) != TA_OK) return rc;
    if (keys_dev) *keys_dev = c->out_keys.p;
    if (faces_dev) *faces_dev = c->out_faces.p;
    if (npairs) *npairs = c->npairs;
    return TA_OK;
}

TA_API int ta_adjacency_export(ta_ctx* c, void* keys_dst_dev, void* faces_dst_dev, int64_t capacity_pairs) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = finish_extract(c)) != TA_OK) return rc;
    if (capacity_pairs < c->npairs) return fail(TA_EINVAL, "export buffers hold %lld pairs, %lld needed", (long long)capacity_pairs, (long long)c->npairs);
    if (c->npairs > 0) {
        if (!keys_dst_dev || !faces_dst_dev) return fail(TA_EINVAL, "NULL export buffer");
        TA_HIP(hipMemcpyAsync(keys_dst_dev, c->out_keys.p, (uint64_t)c->npairs * 8, hipMemcpyDeviceToDevice, c->stream));
        TA_HIP(hipMemcpyAsync(faces_dst_dev, c->out_faces.p, (uint64_t)c->npairs * 24, hipMemcpyDeviceToDevice, c->stream));
    }
    return TA_OK;
}

TA_API int ta_adjacency_merge(ta_ctx* c, const void* keys_dev, const void* faces_dev, int64_t npairs) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (npairs < 0 || (npairs > 0 && (!keys_dev || !faces_dev))) return fail(TA_EINVAL, "bad pair list");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = finish_extract(c)) != TA_OK) return rc;
    if (!(c->feature_mask & TA_F_ADJACENCY)) return fail(TA_EINVAL, "the last extraction did not request adjacency");
    // local list (already collected, so the table is clean) + foreign list -> table -> collect again
    ta::PairTable pt = pair_table(c);
    DevBuf local_k, local_f;
    const uint64_t nl = (uint64_t)c->npairs;
    if ((rc = local_k.reserve(nl * 8 + 8)) != TA_OK) return rc;
    if ((rc = local_f.reserve(nl * 24 + 8)) != TA_OK) { local_k.release(); return rc; }
    hipError_t e = hipSuccess;
    if (nl) {
        e = hipMemcpyAsync(local_k.p, c->out_keys.p, nl * 8, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(local_f.p, c->out_faces.p, nl * 24, hipMemcpyDeviceToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipMemsetAsync(c->small.p, 0, SMALL_WORDS * sizeof(uint32_t), c->stream);
    if (e != hipSuccess) { local_k.release(); local_f.release(); return fail(TA_EHIP, "merge staging: %s", hipGetErrorString(e)); }
    ta::launch_pairs_insert(c->stream, pt, (const uint64_t*)local_k.p, (const uint64_t*)local_f.p, nl, flags_dev(c));
    ta::launch_pairs_insert(c->stream, pt, (const uint64_t*)keys_dev, (const uint64_t*)faces_dev, (uint64_t)npairs, flags_dev(c));
    ta::launch_pairs_collect(c->stream, pt, (uint64_t*)c->out_keys.p, (uint64_t*)c->out_faces.p, cursor_dev(c));
    e = hipMemcpyAsync(c->h_small, c->small.p, SMALL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    local_k.release(); local_f.release();
    if (e != hipSuccess) return fail(TA_EHIP, "merge: %s", hipGetErrorString(e));
    if (c->h_small[ta::FLAG_PAIR_OVERFLOW]) {
        // the collect has written the pairs that did fit over the local list: the extraction's adjacency is gone, and with it the
        // extraction (the getters, ta_adjacency_scope and the exchange calls answer TA_EINVAL until the next ta_extract)
        c->extracted = c->checked = false;
        c->host_pairs_ready = false;
        return fail(TA_ECAPACITY, "adjacency table overflow while merging (2^%d slots): the extraction is lost; raise TA_OPT_PAIR_SLOTS and run ta_extract again", c->pair_log2);
    }
    c->npairs = (int64_t)c->h_small[ta::NFLAGS];
    c->host_pairs_ready = false;
    return TA_OK;
}

TA_API int ta_adjacency_pack(ta_ctx* c, void* block_dev, int64_t capacity_pairs) {
    if (!c || !block_dev) return fail(TA_EINVAL, "NULL argument");
    if (capacity_pairs < 1) return fail(TA_EINVAL, "capacity_pairs must be >= 1");
    if (!c->extracted || !(c->feature_mask & TA_F_ADJACENCY))
        return fail(TA_EINVAL, "no extraction with adjacency has been run on this context");
    if (c->exchanged) return fail(TA_EINVAL, "the adjacency of this extraction was already exchanged");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    ta::launch_pairs_pack(c->stream, (const uint64_t*)c->out_keys.p, (const uint64_t*)c->out_faces.p, cursor_dev(c),
                          flags_dev(c), (uint64_t*)block_dev, (uint64_t)capacity_pairs);
    TA_HIP(hipGetLastError());
    return TA_OK;
}

TA_API int ta_adjacency_pack_shared(ta_ctx* c, void* block_dev, int64_t capacity_pairs) {
    if (!c || !block_dev) return fail(TA_EINVAL, "NULL argument");
    if (capacity_pairs < 1) return fail(TA_EINVAL, "capacity_pairs must be >= 1");
    if (!c->extracted || !(c->feature_mask & TA_F_ADJACENCY))
        return fail(TA_EINVAL, "no extraction with adjacency has been run on this context");
    if (c->exchanged) return fail(TA_EINVAL, "the adjacency of this extraction was already exchanged");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const int64_t lo = c->a_origin, hi = c->a_origin + (c->mdims[0] - c->first_owned);
    TA_HIP(hipMemsetAsync(block_dev, 0, 8, c->stream));          // the block's pair count: the kernel's append cursor
    // (the local list can hold no more pairs than the table has slots)
    ta::launch_pairs_pack_shared(c->stream, pair_table(c), (const uint64_t*)c->out_keys.p, (const uint64_t*)c->out_faces.p,
                                 cursor_dev(c), flags_dev(c), c->boxes, c->max_label, lo, hi, (uint64_t*)block_dev,
                                 (uint64_t)capacity_pairs, 1ull << c->pair_log2);
    TA_HIP(hipGetLastError());
    c->table_clean = false;          // holds this rank's private pairs until ta_adjacency_merge_blocks collects
    c->shared_packed = true;
    return TA_OK;
}

TA_API int ta_adjacency_merge_blocks(ta_ctx* c, const void* blocks_dev, int nblocks, int64_t capacity_pairs) {
    if (!c || !blocks_dev) return fail(TA_EINVAL, "NULL argument");
    if (nblocks < 1 || capacity_pairs < 1) return fail(TA_EINVAL, "nblocks and capacity_pairs must be >= 1");
    if (!c->extracted || !(c->feature_mask & TA_F_ADJACENCY))
        return fail(TA_EINVAL, "no extraction with adjacency has been run on this context");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    // the collect of the extraction left the table clean: rebuild it from every rank's block
    ta::PairTable pt = pair_table(c);
    TA_HIP(hipMemsetAsync(c->small.p, 0, SMALL_WORDS * sizeof(uint32_t), c->stream));
    ta::launch_pairs_insert_blocks(c->stream, pt, (const uint64_t*)blocks_dev, nblocks, (uint64_t)capacity_pairs,
                                   flags_dev(c));
    ta::launch_pairs_collect(c->stream, pt, (uint64_t*)c->out_keys.p, (uint64_t*)c->out_faces.p, cursor_dev(c));
    TA_HIP(hipMemcpyAsync(c->h_small, c->small.p, SMALL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipGetLastError());
    c->table_clean = true;
    c->exchanged = true;
    c->checked = false;
    c->host_pairs_ready = false;
    return TA_OK;
}

}  // extern "C"
