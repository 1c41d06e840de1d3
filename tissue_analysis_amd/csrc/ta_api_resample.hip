// ta_api_resample.hip -- the C ABI of include/tissue_scan_resample.h on top of kernels_resample.hip.
#include "../../include/tissue_scan_resample.h"
#include "../../include/tissue_scan_overlap.h"
#include "../../include/tissue_scan_signal.h"
#include "ta_ctx.h"
#include "ta_resample.h"

namespace {

const char* const NO_RESULT = "no resampled volume for the current grid (run ta_resample_extract)";

int check_source(const void* ptr, int itemsize, const int64_t dims[3]) {
    if (!ptr || !dims) return fail(TA_EINVAL, "NULL argument");
    if (itemsize != 1 && itemsize != 2 && itemsize != 4) return fail(TA_EINVAL, "the source: itemsize must be 1, 2 or 4 bytes, not %d", itemsize);
    for (int d = 0; d < 3; ++d)
        if (dims[d] <= 0 || dims[d] > (1ll << 30)) return fail(TA_EINVAL, "the source: dims[%d]=%lld out of range", d, (long long)dims[d]);
    return TA_OK;
}

void source_adopt(ta_ctx* c, const void* dev_ptr, int itemsize, const int64_t dims[3], const int64_t el[3]) {
    c->rs.src = dev_ptr;
    c->rs.src_itemsize = itemsize;
    for (int d = 0; d < 3; ++d) { c->rs.sdims[d] = dims[d]; c->rs.sel[d] = el[d]; }
    c->rs.valid = false;
}

// the result's voxels of a buffer plane
uint64_t plane_voxels(const ta_ctx* c) { return (uint64_t)c->rs.mdims[1] * (uint64_t)c->rs.mdims[2]; }

}  // namespace

// a new label volume: a result for another grid (dims, origin or halo) is stale; other dims drop source and result
void resample_on_new_volume(ta_ctx* c) {
    const bool same_dims = std::equal(c->rs.mdims, c->rs.mdims + 3, c->mdims);
    if (!same_dims || c->rs.a_origin != c->a_origin || c->rs.first_owned != c->first_owned) c->rs.valid = false;
    if (same_dims || (!c->rs.src && !c->rs.out.p)) return;
    c->rs.src = nullptr; c->rs.src_itemsize = 0;
    c->rs.owned_src.release();
    overlap_on_resampled(c, c->rs.out.p, nullptr, 0);      // (a B or a signal of other dims is dropped by its own file already)
    signal_on_resampled(c, c->rs.out.p, nullptr, 0);
    c->rs.out.release();
}

extern "C" {

TA_API int ta_resample_set_source(ta_ctx* c, const void* host_ptr, int itemsize, const int64_t dims[3], const int64_t strides_bytes[3]) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = check_source(host_ptr, itemsize, dims);
    if (rc != TA_OK) return rc;
    int64_t el[3] = {dims[1] * dims[2], dims[2], 1};
    if (strides_bytes) {                         // a dense axis permutation, as ta_volume_set: memory order = axes by decreasing stride
        int perm[3] = {0, 1, 2};
        std::stable_sort(perm, perm + 3, [&](int x, int y) {
            const int64_t sx = dims[x] == 1 ? INT64_MAX : strides_bytes[x];
            const int64_t sy = dims[y] == 1 ? INT64_MAX : strides_bytes[y];
            return sx > sy;
        });
        int64_t expect = itemsize;
        for (int k = 2; k >= 0; --k) {
            const int ax = perm[k];
            if (dims[ax] != 1 && strides_bytes[ax] != expect)
                return fail(TA_EINVAL, "the source: strides do not describe a dense permuted layout (axis %d: stride %lld, expected %lld)", ax,
                            (long long)strides_bytes[ax], (long long)expect);
            el[ax] = expect / itemsize;
            expect *= dims[ax];
        }
    }
    if ((rc = use_device(c)) != TA_OK) return rc;
    const uint64_t bytes = (uint64_t)dims[0] * dims[1] * dims[2] * itemsize;
    TA_HIP(hipStreamSynchronize(c->stream));     // (a pass in flight may still read the old one)
    c->rs.src = nullptr;
    if ((rc = c->rs.owned_src.reserve(bytes)) != TA_OK) return rc;
    TA_HIP(hipMemcpyAsync(c->rs.owned_src.p, host_ptr, bytes, hipMemcpyHostToDevice, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));     // the host buffer may be freed after return
    source_adopt(c, c->rs.owned_src.p, itemsize, dims, el);
    return TA_OK;
}

TA_API int ta_resample_set_source_device(ta_ctx* c, const void* dev_ptr, int itemsize, const int64_t dims[3]) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = check_source(dev_ptr, itemsize, dims);
    if (rc != TA_OK) return rc;
    if (((uintptr_t)dev_ptr % itemsize) != 0) return fail(TA_EINVAL, "the source: the device pointer is not aligned to its type");
    if ((rc = use_device(c)) != TA_OK) return rc;
    TA_HIP(hipStreamSynchronize(c->stream));
    c->rs.owned_src.release();
    const int64_t el[3] = {dims[1] * dims[2], dims[2], 1};
    source_adopt(c, dev_ptr, itemsize, dims, el);
    return TA_OK;
}

TA_API int ta_resample_extract(ta_ctx* c, const double A[12], int mode, uint32_t fill) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!A) return fail(TA_EINVAL, "NULL argument");
    if (mode != TA_RS_NEAREST && mode != TA_RS_LINEAR) return fail(TA_EINVAL, "bad resampling mode %d", mode);
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(A[k])) return fail(TA_EINVAL, "A[%d][%d]=%g is not finite", k / 4, k % 4, A[k]);
    if (!c->vol) return fail(TA_EINVAL, "no label volume set: the resampled volume takes its grid");
    if (!c->rs.src) return fail(TA_EINVAL, "no source volume set (ta_resample_set_source)");
    const int itemsize = c->rs.src_itemsize;
    if (mode == TA_RS_LINEAR && itemsize == 4) return fail(TA_EINVAL, "TA_RS_LINEAR takes a source of 1 or 2 bytes an item, not 4");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    c->rs.valid = false;
    const void* const was = c->rs.out.p;
    if (c->rs.out.bytes < voxels(c) * itemsize + 64) TA_HIP(hipStreamSynchronize(c->stream));      // (the buffer moves: a pass in flight may read it)
    rc = c->rs.out.reserve(voxels(c) * itemsize + 64);
    overlap_on_resampled(c, was, c->rs.out.p, itemsize);
    signal_on_resampled(c, was, c->rs.out.p, itemsize);
    if (rc != TA_OK) return rc;
    if ((rc = c->rs.small.reserve(16)) != TA_OK) return rc;
    if ((rc = ensure_events(c->rs.ev)) != TA_OK) return rc;
    ta::ResampleArgs a;
    a.src = c->rs.src;
    a.out = c->rs.out.p;
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.a_origin = c->a_origin;
    a.first_owned = c->first_owned;
    for (int k = 0; k < 3; ++k) a.mem_of[c->perm[k]] = k;
    for (int d = 0; d < 3; ++d) { a.m[d] = c->rs.sdims[d]; a.es[d] = c->rs.sel[d]; }
    for (int k = 0; k < 12; ++k) a.A[k] = A[k];
    a.fill = fill;
    a.outside = (unsigned long long*)c->rs.small.p;
    a.tiles_per_group = 0;
    TA_HIP(hipMemsetAsync(c->rs.small.p, 0, 16, c->stream));
    TA_HIP(hipEventRecord(c->rs.ev[0], c->stream));
    c->rs.plan = ta::launch_resample(c->stream, a, itemsize, mode == TA_RS_LINEAR ? ta::RS_LINEAR : ta::RS_NEAREST, &c->rs.vec);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->rs.ev[1], c->stream));
    c->rs.itemsize = itemsize;
    c->rs.mode = mode;
    for (int k = 0; k < 3; ++k) c->rs.mdims[k] = c->mdims[k];
    c->rs.a_origin = c->a_origin;
    c->rs.first_owned = c->first_owned;
    c->rs.valid = true;
    return TA_OK;
}

TA_API int ta_resample_get(ta_ctx* c, void* host_out, int64_t first_plane, int64_t nplanes) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->rs.valid) return fail(TA_EINVAL, NO_RESULT);
    int rc = check_planes(c, first_plane, nplanes);
    if (rc != TA_OK) return rc;
    if (!host_out && nplanes) return fail(TA_EINVAL, "NULL argument");
    if ((rc = use_device(c)) != TA_OK) return rc;
    const uint64_t plane = plane_voxels(c) * c->rs.itemsize;
    if (nplanes) TA_HIP(hipMemcpyAsync(host_out, (const char*)c->rs.out.p + (uint64_t)first_plane * plane, (uint64_t)nplanes * plane, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_resample_device(ta_ctx* c, void** dev_ptr, int* itemsize) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!dev_ptr) return fail(TA_EINVAL, "NULL argument");
    if (!c->rs.valid) return fail(TA_EINVAL, NO_RESULT);
    *dev_ptr = c->rs.out.p;
    if (itemsize) *itemsize = c->rs.itemsize;
    return TA_OK;
}

TA_API int ta_resample_outside(ta_ctx* c, uint64_t* outside) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!outside) return fail(TA_EINVAL, "NULL argument");
    if (!c->rs.valid) return fail(TA_EINVAL, NO_RESULT);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    TA_HIP(hipMemcpyAsync(outside, c->rs.small.p, 8, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_resample_timing(ta_ctx* c, double* ms) {
    return pass_timing(c, ms, [](ta_ctx* c) { return c->rs.valid && c->rs.ev[1] ? c->rs.ev : nullptr; }, "no resample pass has been run");
}

TA_API int ta_resample_debug(ta_ctx* c, uint32_t out[4]) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->rs.valid) return fail(TA_EINVAL, NO_RESULT);
    range_debug_words(out, c->rs.vec ? 1u : 0u, (uint32_t)c->rs.mode, c->rs.plan);
    return TA_OK;
}

TA_API int ta_resample_as_overlap(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->rs.valid) return fail(TA_EINVAL, NO_RESULT);
    if (c->rs.mode != TA_RS_NEAREST) return fail(TA_EINVAL, "labels are resampled with TA_RS_NEAREST: an interpolated volume is no label volume");
    return ta_overlap_set_device(c, c->rs.out.p, c->rs.itemsize);      // (refuses an itemsize of 1)
}

TA_API int ta_resample_as_signal(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->rs.valid) return fail(TA_EINVAL, NO_RESULT);
    return ta_signal_set_device(c, c->rs.out.p, c->rs.itemsize);       // (refuses an itemsize of 4)
}

}  // extern "C"
