// ta_api_walls.hip -- the wall-voxel and wall-median entry points of include/tissue_scan.h on top of kernels_walls.hip,
// kernels_wallsort.hip and kernels_wallmedian.hip.
#include "ta_ctx.h"

#include <cstdio>
#include <cstdlib>

namespace {
// layout of WallVoxelState::counts: counts u32[cells] | cell_base u32[cells] (each padded to 8 bytes) | offsets u64[cells] |
// block sums u64[scan_blocks] | total u64 + status u32[6] (the 32 bytes the host reads back) | cursors | todo u32[cells] |
// lane counts u8[cells][64]
uint64_t wall_bufs(void* base, const ta::WallPlan& p, ta::WallBuffers& b) {
    const uint64_t counts_bytes = (p.cells * 4 + 7) & ~7ull;
    char* at = (char*)base;
    b.counts = (uint32_t*)at; at += counts_bytes;
    b.cell_base = (uint32_t*)at; at += counts_bytes;
    b.offsets = (uint64_t*)at; at += p.cells * 8;
    b.block_sums = (uint64_t*)at; at += p.scan_blocks * 8;
    b.total = (uint64_t*)at; b.status = (uint32_t*)(b.total + 1); at += 32;
    b.cursors = (uint32_t*)at; at += ta::wall_cursor_bytes();
    b.todo = (uint32_t*)at; at += counts_bytes;
    b.lane_counts = (uint8_t*)at; at += p.cells * 64;
    return (uint64_t)(at - (char*)base);
}

// Room for the records the count pass stages: half a record per voxel (tissue: 0.1 - 0.25), split into regions; a
// volume with more takes the second walk for the cells that did not fit.  No memory for it: nothing is staged.
void wall_stage(ta_ctx* c, const ta::WallPlan& p, ta::WallBuffers& b) {
    const uint64_t nvox = (uint64_t)c->mdims[0] * c->mdims[1] * c->mdims[2];
    uint64_t records = std::min<uint64_t>(std::max<uint64_t>(nvox / 2, 1u << 16), 1ull << 31);
    // (tests: force the second walk / small regions.  Clamped: region_of_wave * region + got must stay below 2^32 in the kernel)
    if (const char* env = getenv("TA_WALL_STAGE_RECORDS")) records = std::min<uint64_t>(std::strtoull(env, nullptr, 10), 1ull << 31);
    const uint32_t regions = ta::wall_stage_regions();
    b.region = (uint32_t)(records / regions);
    b.stage = nullptr;
    (void)p;
    if (b.region == 0) return;
    const uint64_t need = ta::wall_stage_bytes(b.region, c->itemsize);
    if (c->walls.stage.bytes < need) {
        c->walls.stage.release();
        if (hipMalloc(&c->walls.stage.p, need) != hipSuccess) {
            (void)hipGetLastError();
            c->walls.stage.p = nullptr;
            b.region = 0;
            return;
        }
        c->walls.stage.bytes = need;
    }
    b.stage = c->walls.stage.p;
}
}  // namespace

// new label values: the staged records carry the OLD labels, a fetch must ask for a fresh count (the staging buffer itself is kept)
void walls_on_new_labels(ta_ctx* c) {
    c->walls.records = -1;
    c->walls.median_count = -1;
    c->walls.region = 0; c->walls.not_staged = 0;
}

// a new label volume: the same, and the staging buffer goes
void walls_on_new_volume(ta_ctx* c) {
    walls_on_new_labels(c);
    c->walls.stage.release();
}

extern "C" {

TA_API int ta_wall_voxels_count(ta_ctx* c, int64_t* nrecords) {
    if (!c || !nrecords) return fail(TA_EINVAL, "NULL argument");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    if (c->first_owned) return fail(TA_EINVAL, "wall voxels are not available on a slab that carries a halo plane");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const ta::WallPlan plan = ta::wall_plan(c->mdims[0], c->mdims[1], c->mdims[2]);
    if (plan.cells >= (1ull << 32)) return fail(TA_EINVAL, "volume too large for the wall voxel pass (%llu row strips)", (unsigned long long)plan.cells);
    ta::WallBuffers wb;
    if ((rc = c->walls.counts.reserve(wall_bufs(nullptr, plan, wb))) != TA_OK) return rc;
    (void)wall_bufs(c->walls.counts.p, plan, wb);
    wall_stage(c, plan, wb);
    c->walls.region = wb.region;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct { uint64_t total; uint32_t not_staged, wide_seen, label_or, unused[3]; } line = {0, 0, 0, 0, {0, 0, 0}};
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float ms_all = 0.f;
    bool wide = false;
    for (int attempt = 0; attempt < 2 && e == hipSuccess; ++attempt) {
        e = hipEventRecord(e0, c->stream);
        if (e == hipSuccess) {
            // count + stage per (row, strip), scan on the device: the only thing the host needs before the fetch is one line
            ta::launch_wall_count(c->stream, c->vol, c->itemsize, c->mdims[0], c->mdims[1], c->mdims[2], wb, wide);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&line, wb.total, 32, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        float ms = 0.f;
        if (e == hipSuccess) (void)hipEventElapsedTime(&ms, e0, e1);
        ms_all += ms;
        if (!line.wide_seen || wide) break;
        wide = true;                    // a label from 2^31 up: once more with the kernel that takes them
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(TA_EHIP, "wall voxel count: %s", hipGetErrorString(e));
    c->walls.records = (int64_t)line.total;
    c->walls.median_count = -1;
    c->walls.not_staged = line.not_staged;
    c->walls.wide = wide;
    c->walls.label_or = line.label_or;
    c->walls.ms = ms_all;
    if (getenv("TA_WALL_VERBOSE"))
        fprintf(stderr, "[tissue_scan] wall voxels: %llu records in %llu cells of 256 voxels, %u cells not staged (regions of %u records), wide=%d, %.3f ms\n",
                (unsigned long long)line.total, (unsigned long long)plan.cells, line.not_staged, wb.region, (int)wide, ms_all);
    *nrecords = c->walls.records;
    return TA_OK;
}

}  // extern "C"

namespace {
// The records of the last ta_wall_voxels_count on the DEVICE, in memory order or grouped by pair: `buf` owns them, *pairs_dev /
// *coords_dev point into it; the launches are bracketed by e0 / e1 when given.  Only enqueues work (and allocates).
int wall_records_device(ta_ctx* c, bool by_pair, DevBuf& buf, uint32_t** pairs_dev, int32_t** coords_dev, hipEvent_t e0, hipEvent_t e1) {
    const uint64_t n = (uint64_t)c->walls.records;
    int rc;
    const ta::WallPlan plan = ta::wall_plan(c->mdims[0], c->mdims[1], c->mdims[2]);
    ta::WallBuffers wb;
    (void)wall_bufs(c->walls.counts.p, plan, wb);
    wb.region = c->walls.region;
    wb.stage = c->walls.region ? c->walls.stage.p : nullptr;
    // one allocation: records in memory order | (grouped fetch) the same again grouped, sort keys / indices x 2, sort temp.
    // A volume of fewer than 2^32 voxels is grouped from KEYS: the fetch writes sort keys and linear voxel indices straight into
    // the sort's buffers (no records in memory order, no key pass, no gather of coordinates behind the last pass)
    const uint64_t nvox = (uint64_t)c->mdims[0] * (uint64_t)c->mdims[1] * (uint64_t)c->mdims[2];
    // (tests and same-call comparisons: TA_WALL_KEYED=0 sorts the records of the plain fetch, as volumes of 2^32 voxels and more do)
    const char* env_keyed = getenv("TA_WALL_KEYED");
    const bool keyed = by_pair && nvox < (1ull << 32) && !(env_keyed && env_keyed[0] == '0');
    const uint64_t temp_bytes = by_pair ? ta::wall_sort_temp_bytes(n) : 0;
    const uint64_t rec = n * 8, co = align16(n * 12), ix = align16(n * 4);
    if ((rc = buf.reserve(by_pair ? (keyed ? 0 : rec + co) + rec + co + 2 * rec + 2 * ix + temp_bytes + 64 : rec + co)) != TA_OK) return rc;
    char* p = (char*)buf.p;
    int label_bits = 1;                                             // bits a label of this volume takes
    while (label_bits < 32 && (c->walls.label_or >> label_bits) != 0u) ++label_bits;
    uint32_t* dpa = nullptr; int32_t* dco = nullptr;
    if (!keyed) { dpa = (uint32_t*)p; p += rec; dco = (int32_t*)p; p += co; }
    uint32_t* gpa = dpa; int32_t* gco = dco;
    uint64_t *k0 = nullptr, *k1 = nullptr; uint32_t *i0 = nullptr, *i1 = nullptr;
    if (by_pair) {
        gpa = (uint32_t*)p; p += rec;
        gco = (int32_t*)p; p += co;
        k0 = (uint64_t*)p; p += rec;
        k1 = (uint64_t*)p; p += rec;
        i0 = (uint32_t*)p; p += ix;
        i1 = (uint32_t*)p; p += ix;
    }
    hipError_t e = e0 ? hipEventRecord(e0, c->stream) : hipSuccess;
    if (e == hipSuccess) {
        // records leave the kernels as (lo, hi) / coordinates in ARRAY-axis order -- or as keys / linear indices for the sort
        ta::launch_wall_fetch(c->stream, c->vol, c->itemsize, c->mdims[0], c->mdims[1], c->mdims[2], wb, c->walls.wide,
                              c->walls.not_staged, keyed ? (uint32_t*)k0 : dpa, keyed ? (int32_t*)i0 : dco, c->perm, keyed ? label_bits : 0);
        e = hipGetLastError();
    }
    if (e == hipSuccess && keyed)
        e = ta::launch_wall_group_keyed(c->stream, n, k0, k1, i0, i1, p, label_bits, c->mdims, c->perm, gpa, gco);
    else if (e == hipSuccess && by_pair)
        e = ta::launch_wall_group_by_pair(c->stream, dpa, dco, n, k0, k1, i0, i1, p, temp_bytes, label_bits, gpa, gco);
    if (e == hipSuccess && e1) e = hipEventRecord(e1, c->stream);
    if (e != hipSuccess) return fail(TA_EHIP, "wall voxels: %s", hipGetErrorString(e));
    *pairs_dev = gpa; *coords_dev = gco;
    return TA_OK;
}

int wall_voxels_fetch(ta_ctx* c, uint32_t* pairs, int32_t* coords, double* ms_out, bool by_pair) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (c->walls.records < 0) return fail(TA_EINVAL, "call ta_wall_voxels_count first");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint64_t n = (uint64_t)c->walls.records;
    if (ms_out) *ms_out = c->walls.ms;
    if (n == 0) return TA_OK;
    if (!pairs || !coords) return fail(TA_EINVAL, "NULL output array");
    if (by_pair && n >= (1ull << 32)) return fail(TA_EINVAL, "too many records (%llu) for the grouped fetch", (unsigned long long)n);
    DevBuf buf;
    uint32_t* gpa = nullptr; int32_t* gco = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess && (rc = wall_records_device(c, by_pair, buf, &gpa, &gco, e0, e1)) != TA_OK) {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        buf.release();
        return rc;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(pairs, gpa, n * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(coords, gco, n * 12, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    float ms = 0.f;
    if (e == hipSuccess) (void)hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    buf.release();
    if (e != hipSuccess) return fail(TA_EHIP, "wall voxels: %s", hipGetErrorString(e));
    if (ms_out) *ms_out = c->walls.ms + ms;
    return TA_OK;
}
}  // namespace

extern "C" {

TA_API int ta_wall_medians(ta_ctx* c, int max_iter, int64_t* nwalls, double* ms_out) {
    if (!c || !nwalls) return fail(TA_EINVAL, "NULL argument");
    if (c->walls.records < 0) return fail(TA_EINVAL, "call ta_wall_voxels_count first");
    if (max_iter < 1) return fail(TA_EINVAL, "max_iter must be positive");
    if (c->perm[0] != 0 || c->perm[1] != 1 || c->perm[2] != 2)
        return fail(TA_EINVAL, "wall medians need a C-ordered volume (the order of a wall's voxels decides ties)");
    if ((uint64_t)c->walls.records >= (1ull << 31)) return fail(TA_EINVAL, "too many records for the wall medians");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint64_t n = (uint64_t)c->walls.records;
    c->walls.median_count = -1;
    *nwalls = 0;
    if (ms_out) *ms_out = 0.0;
    if (n == 0) { c->walls.median_count = 0; return TA_OK; }
    if (n >= (1ull << 32)) return fail(TA_EINVAL, "too many records (%llu) for the grouped fetch", (unsigned long long)n);
    DevBuf buf, scratch, starts;
    uint32_t* gpa = nullptr; int32_t* gco = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, c->stream);
    rc = e == hipSuccess ? wall_records_device(c, true, buf, &gpa, &gco, nullptr, nullptr) : TA_EHIP;
    if (rc == TA_OK) rc = scratch.reserve(ta::wall_median_scratch_bytes(n));
    if (rc == TA_OK) rc = starts.reserve(n * 4 + 16);
    uint64_t E = 0;
    uint32_t status = 0;
    if (rc == TA_OK) {
        e = ta::launch_wall_starts(c->stream, gpa, n, scratch.p, (uint32_t*)starts.p, &E);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) rc = c->walls.medians.reserve(E * 24 + 16);
        if (e == hipSuccess && rc == TA_OK) {
            uint32_t* op = (uint32_t*)c->walls.medians.p;
            uint32_t* os = op + 2 * E;
            int32_t* om = (int32_t*)(os + E);
            uint32_t* st = ScanBlock(n).counts(scratch.p);                // (the flags are dead: their first word takes the status)
            e = hipMemsetAsync(st, 0, 4, c->stream);
            if (e == hipSuccess) {
                ta::launch_wall_medians(c->stream, gpa, gco, (const uint32_t*)starts.p, (uint32_t)E, n, max_iter, op, os, om, st);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&status, st, 4, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        }
    }
    float ms = 0.f;
    if (rc == TA_OK && e == hipSuccess) (void)hipEventElapsedTime(&ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    buf.release(); scratch.release(); starts.release();
    if (rc != TA_OK) return rc;
    if (e != hipSuccess) return fail(TA_EHIP, "wall medians: %s", hipGetErrorString(e));
    // (walls still moving after max_iter passes are MARKED -- bit 31 of their size word -- not refused: a caller asks for
    //  some walls, and one that nobody asks for -- the background's, say -- must not fail the rest)
    c->walls.median_count = (int64_t)E;
    *nwalls = (int64_t)E;
    if (ms_out) *ms_out = ms;
    return TA_OK;
}

TA_API int ta_wall_medians_get(ta_ctx* c, uint32_t* pairs, uint32_t* sizes, int32_t* medians) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (c->walls.median_count < 0) return fail(TA_EINVAL, "call ta_wall_medians first");
    const uint64_t E = (uint64_t)c->walls.median_count;
    if (E == 0) return TA_OK;
    if (!pairs || !sizes || !medians) return fail(TA_EINVAL, "NULL output array");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint32_t* op = (const uint32_t*)c->walls.medians.p;
    TA_HIP(hipMemcpyAsync(pairs, op, E * 8, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipMemcpyAsync(sizes, op + 2 * E, E * 4, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipMemcpyAsync(medians, op + 3 * E, E * 12, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_wall_voxels_get(ta_ctx* c, uint32_t* pairs, int32_t* coords, double* ms_out) {
    return wall_voxels_fetch(c, pairs, coords, ms_out, false);
}

TA_API int ta_wall_voxels_get_by_pair(ta_ctx* c, uint32_t* pairs, int32_t* coords, double* ms_out) {
    return wall_voxels_fetch(c, pairs, coords, ms_out, true);
}

}  // extern "C"
