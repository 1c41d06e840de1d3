// ta_api.hip -- the core C ABI of include/tissue_scan.h on top of the gfx950 kernels: the context, its options and stream, the volume,
// the sweep and its results, timing and memory helpers.  (Wall voxels: ta_api_walls.hip; sparse ids: ta_api_sparse.hip; rank exchange:
// ta_api_exchange.hip; the features: ta_api_<feature>.hip.)
#include "ta_ctx.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <new>

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {

int ensure_pair_table(ta_ctx* c, int log2cap) {
    if (c->pair_log2 == log2cap && c->pslots.p) return TA_OK;
    const uint64_t cap = 1ull << log2cap;
    int rc;
    if ((rc = c->pslots.reserve(cap * sizeof(ta::PairSlot))) != TA_OK) return rc;
    if ((rc = c->out_keys.reserve(cap * 8)) != TA_OK) return rc;
    if ((rc = c->out_faces.reserve(cap * 24)) != TA_OK) return rc;
    c->pair_log2 = log2cap;
    c->table_clean = false;
    return TA_OK;
}

int auto_pair_log2(uint32_t max_label) {
    uint64_t want = 16ull * ((uint64_t)max_label + 1);
    int l = 16;
    while ((1ull << l) < want && l < 28) ++l;
    return l;
}

// Label changes per voxel along the fast axis, from a SAMPLE of the owned planes (eight planes spread over the slab, one small
// kernel each, one 64-byte read-back): what predicts which tile shape of the uint32 adjacency sweep is faster.  One stream
// synchronisation, once per resident volume.  < 0: could not be measured.
double sampled_event_density(ta_ctx* c) {
    const int64_t owned = c->mdims[0] - c->first_owned;
    if (owned <= 0 || c->mdims[1] <= 0 || c->mdims[2] <= 0 || !c->vol) return -1.0;
    const int nsample = (int)std::min<int64_t>(8, owned);
    DevBuf d;
    if (d.reserve((uint64_t)nsample * sizeof(uint64_t)) != TA_OK) return -1.0;
    const size_t plane_bytes = (size_t)c->mdims[1] * c->mdims[2] * c->itemsize;
    for (int k = 0; k < nsample; ++k) {
        const int64_t p = c->first_owned + ((2 * k + 1) * owned) / (2 * nsample);
        ta::launch_plane_events(c->stream, (const char*)c->vol + (size_t)p * plane_bytes, c->itemsize, 1, c->mdims[1], c->mdims[2], (uint64_t*)d.p + k);
    }
    uint64_t ev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ev, d.p, (size_t)nsample * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    d.release();
    if (e != hipSuccess) { (void)hipGetLastError(); return -1.0; }
    uint64_t tot = 0;
    for (int k = 0; k < nsample; ++k) tot += ev[k];
    return (double)tot / ((double)nsample * (double)c->mdims[1] * (double)c->mdims[2]);
}

// Above this many label changes per voxel the narrow tiles win (five waves a SIMD where every plane step is full of records),
// below it the wide ones (fewer plane steps where most steps are background).  Same box, same call, round 5: C4 (0.023 changes a
// voxel) wide 0.98 vs narrow 1.01 ms; the same cells without the ellipsoid (0.054) 1.38 vs 1.28 ms.
constexpr double SHAPE_DENSITY_NARROW = 0.032;
constexpr double WIDE_SHORTER_TILES_DENSITY = 0.02;       // (see run_extract: the default tile height of the wide tiles)

// The sweep shape of this launch; *tune = the measuring slot (0 .. 3) whose events bracket it, or -1.
int sweep_shape(ta_ctx* c, bool adjacency, int* tune) {
    *tune = -1;
    if (c->itemsize != 4 || !adjacency) return 0;
    if (c->shape.opt >= 0) return c->shape.opt;
    // the wide tiles want whole 512-column tiles: the partial ones run a kernel with three waves per SIMD (1000^3: 1.24
    // against 1.05 ms), and a volume narrower than a tile has nothing else
    if (c->mdims[2] % 512 != 0) return 0;
    if (c->shape.pick >= 0) return c->shape.pick;
    if (c->shape.opt == -1) {
        // decided BEFORE the first sweep, from the density of label changes in a sample of planes (a caller that sweeps a volume
        // once -- SpatialImageAnalysis(image) -- gets the faster shape on that sweep)
        const double density = sampled_event_density(c);
        c->shape.density = density;
        c->shape.pick = (density >= 0.0 && density > SHAPE_DENSITY_NARROW) ? 0 : 1;
        return c->shape.pick;
    }
    // TA_OPT_SWEEP_SHAPE = -2: the first four sweeps of the volume take turns (wide, narrow, wide, narrow), each between two
    // events of its own, and the faster shape keeps the volume
    bool all = c->shape.tune_launched == 4;
    for (int k = 0; k < c->shape.tune_launched; ++k) {
        if (!c->shape.tune_done[k]) {
            if (hipEventQuery(c->shape.tune_ev[2 * k + 1]) == hipSuccess &&
                hipEventElapsedTime(&c->shape.tune_ms[k], c->shape.tune_ev[2 * k], c->shape.tune_ev[2 * k + 1]) == hipSuccess) c->shape.tune_done[k] = true;
            else (void)hipGetLastError();             // (not ready: asked again by the next sweep)
        }
        all = all && c->shape.tune_done[k];
    }
    if (all) {
        c->shape.pick = std::min(c->shape.tune_ms[0], c->shape.tune_ms[2]) <= std::min(c->shape.tune_ms[1], c->shape.tune_ms[3]) ? 1 : 0;
        return c->shape.pick;
    }
    if (c->shape.tune_launched < 4 && c->shape.tune_ev[7]) {
        *tune = c->shape.tune_launched;                     // (counted as launched by run_extract once BOTH its events are on the stream)
        return (*tune & 1) ^ 1;                       // wide, narrow, wide, narrow
    }
    return 1;                                         // (measured sweeps still in flight)
}

// One full extraction pass on the stream (no host sync).
int run_extract(ta_ctx* c) {
    const uint64_t nlabels = (uint64_t)c->max_label + 1;
    ta::SweepArgs a;
    a.vol = sweep_vol(c);
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.a_origin = c->a_origin;
    a.first_owned = c->first_owned;
    int tune = -1;
    a.shape = sweep_shape(c, c->feature_mask & TA_F_ADJACENCY, &tune);
    c->shape.last = a.shape;
    a.tile_planes = c->tile_planes > 0 ? c->tile_planes : ta::sweep_default_tile_planes(c->feature_mask & TA_F_ADJACENCY, c->itemsize, a.shape);
    if (c->tile_planes <= 0) {
        // the wide tiles of a volume whose sampled planes change label often hold more labels and pairs a plane: a little shorter
        // (C4, 0.023 changes a voxel: 28 planes 0.948 against 0.954 ms at 32; C5, 0.014: 32 planes 6.546 against 6.562 at 28 --
        // profiles/r05_tile_planes.txt; without a measured density -- a forced shape -- the default stays)
        if (a.shape == 1 && c->shape.density >= WIDE_SHORTER_TILES_DENSITY && a.tile_planes > 28) a.tile_planes = 28;
        // automatic: small volumes get shorter tiles until the launch has >= 2048 workgroups (8 per CU)
        while (a.tile_planes > 8 && ta::sweep_grid_size(a, c->itemsize, c->feature_mask & TA_F_ADJACENCY) < 2048) a.tile_planes /= 2;
        // volumes whose cells are so small that a tile holds more labels than the workgroup tables (the contributions
        // then spill to global atomics, ~100x dearer) get shorter tiles still: see finish_extract
        for (int k = 0; k < c->auto_tile_shift && a.tile_planes > 1; ++k) a.tile_planes /= 2;
    }
    {   // packed LDS moment words: each kernel is built for tiles up to this height
        const int cap = ta::sweep_max_tile_planes(c->feature_mask & TA_F_ADJACENCY, c->itemsize, a.shape);
        if (a.tile_planes > cap) a.tile_planes = cap;
    }
    c->tile_planes_used = a.tile_planes;
    // 16-byte loads: rows that are 16-byte aligned, or ANY rows of a volume the library uploaded itself (unaligned 16-byte
    // global loads are legal on gfx950 -- 6.2 TB/s from dword-aligned, 4.8 TB/s from odd addresses, measured -- and the
    // strip that straddles the end of the very last row reads into the slack ta_volume_set leaves behind the buffer)
    a.vec_ok = ((((uintptr_t)a.vol & 15) == 0) && ((a.n2 * c->itemsize) % 16 == 0)) || (a.vol == c->owned_vol.p && c->owned_vol.p) ||
               c->ids.compact || c->volume_slack >= 16;       // (an adopted buffer whose owner promises readable bytes behind it: TA_OPT_VOLUME_SLACK)
    a.max_label = c->max_label;
    a.sums = c->sums;
    a.boxes = c->boxes;
    a.pairs = pair_table(c);
    a.flags = flags_dev(c);
    uint64_t* hot_rows = nullptr;
    uint64_t nwg = 0;
    if (c->impl == 0) {           // the sweep keeps a private row per workgroup for the hot label
        nwg = ta::sweep_grid_size(a, c->itemsize, c->feature_mask & TA_F_ADJACENCY);
        int rc0 = c->hot_rows.reserve(nwg * ta::HOTW * 8);
        if (rc0 != TA_OK) return rc0;
        hot_rows = (uint64_t*)c->hot_rows.p;
    }

    const bool adj = c->feature_mask & TA_F_ADJACENCY;
    c->last_grid = ta::sweep_grid_size(a, c->itemsize, c->feature_mask & TA_F_ADJACENCY);
    // A hipEventRecord costs ~4 us of queue time: by default only the sweep kernel is bracketed (TA_OPT_TIMING)
    const size_t nslots = c->ring.size() / 2;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    if (c->timing >= 1 && nslots) {
        ev_a = c->ring[2 * (c->extract_seq % nslots)];
        ev_b = c->ring[2 * (c->extract_seq % nslots) + 1];
        if (c->extract_seq - c->ring_since >= nslots) c->ring_since = c->extract_seq - nslots + 1;
    } else {
        c->ring_since = c->extract_seq + 1;
    }
    ++c->extract_seq;
    if (c->timing >= 2) TA_HIP(hipEventRecord(c->ev[0], c->stream));
    if (adj && !c->table_clean) {
        ta::launch_pairs_clear(c->stream, a.pairs);
        c->table_clean = true;
    }
    ta::launch_init_accumulators(c->stream, c->sums, c->boxes, nlabels, flags_dev(c), cursor_dev(c), hot_rows);
    // the sweep kernel alone (what the roofline is quoted on): the two events ride on the sweep's own launches
    // (begin / end timestamps of the dispatch, no event-record packets on the queue); the naive kernel gets plain records
    const bool own_dims = c->mdims[0] - c->first_owned > 0 && c->mdims[1] > 0 && c->mdims[2] > 0;
    if (tune >= 0) TA_HIP(hipEventRecord(c->shape.tune_ev[2 * tune], c->stream));
    if (c->impl == 1 || !own_dims) {
        if (ev_a) TA_HIP(hipEventRecord(ev_a, c->stream));
        if (c->impl == 1) ta::launch_naive(c->stream, a, c->itemsize, c->feature_mask);
        if (ev_b) TA_HIP(hipEventRecord(ev_b, c->stream));
    } else {
        ta::launch_scan(c->stream, a, c->itemsize, c->feature_mask, ev_a, ev_b);
    }
    if (tune >= 0) {
        TA_HIP(hipEventRecord(c->shape.tune_ev[2 * tune + 1], c->stream));
        c->shape.tune_launched = tune + 1;                  // (a slot counts only with both of its events recorded: an early return above leaves it to be measured again)
    }
    // Without adjacency the LAST kernel of the step (the hot-row fold) mirrors the flag words into host-mapped memory
    // itself: no device-to-host copy (a blit kernel and a queue barrier) at the end of the step.  With adjacency the pair
    // count is final only when the collect kernel has ended; letting its last block publish it was measured and costs
    // more (every block then waits for its own stores before it can count itself done: 29 -> 44 us) than the copy.
    uint32_t* mirror = c->h_small_dev;
    bool published = false;
    if (hot_rows && !adj) {
        ta::launch_hot_reduce(c->stream, a, c->itemsize, hot_rows, (uint32_t)nwg, mirror, SMALL_WORDS);
        published = mirror != nullptr;
    }
    if (adj && hot_rows)             // the fold of the hot-label rows rides along with the collect: one launch
        ta::launch_pairs_collect_hot(c->stream, a.pairs, (uint64_t*)c->out_keys.p, (uint64_t*)c->out_faces.p, cursor_dev(c),
                                     a, c->itemsize, hot_rows, (uint32_t)nwg);
    else if (adj)
        ta::launch_pairs_collect(c->stream, a.pairs, (uint64_t*)c->out_keys.p, (uint64_t*)c->out_faces.p, cursor_dev(c));
    if (c->timing >= 2) TA_HIP(hipEventRecord(c->ev[3], c->stream));
    if (!published)
        TA_HIP(hipMemcpyAsync(c->h_small, c->small.p, SMALL_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost,
                              c->stream));
    TA_HIP(hipGetLastError());
    return TA_OK;
}

}  // namespace

// Drain the stream and validate the flags of the last pass; grows the adjacency table and
// re-runs when it overflowed.
int finish_extract(ta_ctx* c) {
    if (!c->extracted) return fail(TA_EINVAL, "no extraction has been run on this context");
    if (c->checked) return TA_OK;
    if (c->exchanged) {       // the list came from other ranks too: a re-run is the host's call
        TA_HIP(hipStreamSynchronize(c->stream));
        int rc = rerank_verdict(c, c->h_small[ta::NFLAGS + 1]);
        if (rc != TA_OK) return rc;
        if (c->h_small[ta::FLAG_RANGE])
            return fail(TA_ERANGE, "a rank saw a label above max_label=%u", c->max_label);
        if (c->h_small[ta::FLAG_EXCHANGE_OVERFLOW])
            return fail(TA_ECAPACITY, "an exchange block was too small for a rank's pair list");
        if (c->h_small[ta::FLAG_PAIR_OVERFLOW])
            return fail(TA_ECAPACITY, "adjacency table overflow on some rank (2^%d slots here)", c->pair_log2);
        c->npairs = (int64_t)c->h_small[ta::NFLAGS];
        c->checked = true;
        return TA_OK;
    }
    for (int attempt = 0; attempt < 8; ++attempt) {
        TA_HIP(hipStreamSynchronize(c->stream));
        int rc = rerank_verdict(c, c->h_small[ta::NFLAGS + 1]);      // (the word ta_volume_rerank left behind came back with this extraction's flags)
        if (rc != TA_OK) return rc;
        if (c->h_small[ta::FLAG_RANGE])
            return fail(TA_ERANGE, "the volume holds a label above max_label=%u", c->max_label);
        if (!c->h_small[ta::FLAG_PAIR_OVERFLOW]) {
            c->npairs = (c->feature_mask & TA_F_ADJACENCY) ? (int64_t)c->h_small[ta::NFLAGS] : 0;
            c->checked = true;
            // more than a handful of table spills per workgroup: the next sweeps of this context use shorter tiles
            // (results do not depend on the tile height; only the automatic height adapts, an explicit one is kept)
            const uint64_t spills = (uint64_t)c->h_small[ta::FLAG_LDS_LABEL_SPILL] + c->h_small[ta::FLAG_LDS_PAIR_SPILL];
            if (c->impl == 0 && c->tile_planes <= 0 && c->auto_tile_shift < 4 && spills > 8 * c->last_grid) ++c->auto_tile_shift;
            return TA_OK;
        }
        if (c->pair_log2 >= 30) break;
        if ((rc = ensure_pair_table(c, c->pair_log2 + 2)) != TA_OK) return rc;
        if (c->reduced)       // a local re-run would replace the reduced (global) rows by this rank's: the host redoes the step
            return fail(TA_ECAPACITY, "adjacency table overflow (grown to 2^%d slots): repeat the extraction on every rank", c->pair_log2);
        if ((rc = run_extract(c)) != TA_OK) return rc;
    }
    return fail(TA_ECAPACITY, "adjacency table overflow at 2^%d slots", c->pair_log2);
}

// ---- companion volumes (ta_ctx.h) ------------------------------------------------------------------------------------------

static void companion_adopt(const ta_ctx* c, Companion& v, const void* dev_ptr, int itemsize) {
    v.p = dev_ptr;
    v.itemsize = itemsize;
    for (int m = 0; m < 3; ++m) v.mdims[m] = c->mdims[m];
}

int companion_set_host(ta_ctx* c, Companion& v, const CompanionKind& k, const void* host_ptr, int itemsize, const int64_t dims[3],
                       const int64_t strides_bytes[3]) {
    if (!host_ptr || !dims) return fail(TA_EINVAL, "NULL argument");
    if (itemsize != k.size_a && itemsize != k.size_b) return fail(TA_EINVAL, "%s: itemsize must be %d or %d bytes, not %d", k.noun, k.size_a, k.size_b, itemsize);
    if (!c->vol) return fail(TA_EINVAL, "no label volume set: %s takes its dims and layout", k.noun);
    int64_t adims[3], el[3];                     // the label volume's dims and element strides, in array-axis order
    int64_t e = 1;
    for (int m = 2; m >= 0; --m) { adims[c->perm[m]] = c->mdims[m]; el[c->perm[m]] = e; e *= c->mdims[m]; }
    for (int d = 0; d < 3; ++d) {
        if (dims[d] != adims[d])
            return fail(TA_EINVAL, "%s: dims (%lld, %lld, %lld) differ from the label volume's (%lld, %lld, %lld)", k.noun, (long long)dims[0],
                        (long long)dims[1], (long long)dims[2], (long long)adims[0], (long long)adims[1], (long long)adims[2]);
        const int64_t st = strides_bytes ? strides_bytes[d] : (d == 2 ? 1 : (d == 1 ? dims[2] : dims[1] * dims[2])) * itemsize;
        if (dims[d] != 1 && st != el[d] * itemsize)
            return fail(TA_EINVAL, "%s: the layout differs from the label volume's (axis %d: stride %lld bytes, expected %lld)", k.noun, d,
                        (long long)st, (long long)(el[d] * itemsize));
    }
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint64_t bytes = (uint64_t)e * itemsize;
    TA_HIP(hipStreamSynchronize(c->stream));     // (a pass in flight may still read the old one)
    v.p = nullptr;
    if ((rc = v.owned.reserve(bytes + 64)) != TA_OK) return rc;
    TA_HIP(hipMemcpyAsync(v.owned.p, host_ptr, bytes, hipMemcpyHostToDevice, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));     // the host buffer may be freed after return
    companion_adopt(c, v, v.owned.p, itemsize);
    return TA_OK;
}

int companion_set_device(ta_ctx* c, Companion& v, const CompanionKind& k, const void* dev_ptr, int itemsize) {
    if (!dev_ptr) return fail(TA_EINVAL, "NULL argument");
    if (itemsize != k.size_a && itemsize != k.size_b) return fail(TA_EINVAL, "%s: itemsize must be %d or %d bytes, not %d", k.noun, k.size_a, k.size_b, itemsize);
    if (!c->vol) return fail(TA_EINVAL, "no label volume set: %s takes its buffer dims", k.noun);
    if (((uintptr_t)dev_ptr % itemsize) != 0) return fail(TA_EINVAL, "%s: the device pointer is not aligned to its type", k.noun);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    TA_HIP(hipStreamSynchronize(c->stream));
    v.owned.release();
    companion_adopt(c, v, dev_ptr, itemsize);
    return TA_OK;
}

void companion_on_new_volume(const ta_ctx* c, Companion& v) {
    if (v.p && !companion_matches(c, v)) { v.p = nullptr; v.owned.release(); v.itemsize = 0; }
}

// ---- the one invalidation path (ta_ctx.h) -----------------------------------------------------------------------------------

static void voxels_changed(ta_ctx* c) {          // what every change of the voxels ends, whoever made it
    sparse_on_new_volume(c);
    c->shape.forget_choice();
    c->extracted = c->checked = false;
    overlap_on_new_volume(c);
    junctions_on_new_volume(c);
    components_on_new_volume(c);
    distance_on_new_volume(c);
    nearest_on_new_volume(c);
    profile_on_new_volume(c);
    sighist_on_new_volume(c);
    sigmom_on_new_volume(c);
    cosig_on_new_volume(c);
    topology_on_new_volume(c);
    extents_on_new_volume(c);
}

void volume_labels_changed(ta_ctx* c) {
    voxels_changed(c);
    walls_on_new_labels(c);
}

void volume_replaced(ta_ctx* c) {
    voxels_changed(c);
    c->auto_tile_shift = 0;
    walls_on_new_volume(c);
    signal_on_new_volume(c);         // (these two are keyed by the extraction, which is gone; a signal of other dims is dropped)
    wallgeo_on_new_volume(c);
    resample_on_new_volume(c);       // (reads the grid only: new label values leave it alone)
}

// A result of `bytes` that lives on the device only while it is read back: `enqueue(dev)` launches what writes it and answers
// with hipGetLastError (or an upload's error before it); then the copy to `host_dst` and one drain.  The scratch is released on
// every path; `what` names the result in the TA_EHIP message.
template <class Enqueue> static int run_and_read_back(ta_ctx* c, const char* what, uint64_t bytes, void* host_dst, Enqueue enqueue) {
    DevBuf out;
    const int rc = out.reserve(bytes);
    if (rc != TA_OK) return rc;
    hipError_t e = enqueue(out.p);
    if (e == hipSuccess) e = hipMemcpyAsync(host_dst, out.p, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    out.release();
    if (e != hipSuccess) return fail(TA_EHIP, "%s: %s", what, hipGetErrorString(e));
    return TA_OK;
}

extern "C" {

TA_API int ta_version(void) { return TA_ABI_VERSION; }

TA_API const char* ta_last_error(void) { return g_err.c_str(); }

TA_API int ta_device_count(int* count) {
    if (!count) return fail(TA_EINVAL, "count is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *count = n;
    return TA_OK;
}

TA_API int ta_ctx_destroy(ta_ctx* c);

TA_API int ta_ctx_create(int device_id, ta_ctx** out) {
    if (!out) return fail(TA_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(TA_ENODEVICE, "no HIP device visible (libtissue_scan needs an MI355X / gfx950 GPU)");
    }
    if (device_id < 0 || device_id >= n) return fail(TA_EINVAL, "device_id %d out of range [0,%d)", device_id, n);
    ta_ctx* c = new (std::nothrow) ta_ctx();
    if (!c) return fail(TA_ENOMEM, "out of host memory");
    c->device = device_id;
    // every failure below goes through ta_ctx_destroy: it releases whatever was created so far
    int rc = TA_OK;
    hipError_t e = hipSetDevice(device_id);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) c->own_stream = true;
    for (auto& ev : c->ev) if (e == hipSuccess) e = hipEventCreate(&ev);
    try { c->ring.assign(2, nullptr); } catch (...) { rc = fail(TA_ENOMEM, "out of host memory"); }
    for (auto& ev : c->ring) if (e == hipSuccess && rc == TA_OK) e = hipEventCreate(&ev);
    for (auto& ev : c->shape.tune_ev) if (e == hipSuccess && rc == TA_OK) e = hipEventCreate(&ev);
    if (e == hipSuccess) rc = c->small.reserve(SMALL_WORDS * sizeof(uint32_t));
    if (e == hipSuccess && rc == TA_OK) e = hipHostMalloc((void**)&c->h_small, SMALL_WORDS * sizeof(uint32_t), hipHostMallocMapped);
    if (e == hipSuccess && rc == TA_OK) {
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, c->h_small, 0) == hipSuccess) c->h_small_dev = (uint32_t*)dp;
        else (void)hipGetLastError();          // no mapping: the steps fall back to the device-to-host copy
    }
    if (e != hipSuccess || rc != TA_OK) {
        if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? TA_ENOMEM : TA_EHIP, "ta_ctx_create: %s", hipGetErrorString(e));
        const std::string keep = g_err;
        (void)ta_ctx_destroy(c);
        g_err = keep;
        return rc;
    }
    memset(c->h_small, 0, SMALL_WORDS * sizeof(uint32_t));
    *out = c;
    return TA_OK;
}

TA_API int ta_ctx_destroy(ta_ctx* c) {
    if (!c) return TA_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->owned_vol.release(); c->own_sums.release(); c->own_boxes.release();
    c->pslots.release(); c->out_keys.release(); c->out_faces.release();
    c->small.release();
    c->hot_rows.release(); c->sort_buf.release(); c->h_pairs.release();
    c->walls.release(); c->ids.release(); c->shape.release();
    c->sig.release(); c->mesh.release(); c->ov.release(); c->jn.release(); c->wg.release(); c->cc.release(); c->dist.release(); c->near.release(); c->prof.release(); c->sh.release(); c->sm.release(); c->co.release(); c->tp.release(); c->ex.release(); c->rs.release();
    if (c->h_small) (void)hipHostFree(c->h_small);
    destroy_events(c->ev);
    for (auto& e : c->ring) if (e) (void)hipEventDestroy(e);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return TA_OK;
}

TA_API int ta_ctx_set_stream(ta_ctx* c, void* hip_stream) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if (c->stream) TA_HIP(hipStreamSynchronize(c->stream));
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    c->stream = nullptr;
    if (hip_stream == TA_STREAM_LEGACY_DEFAULT) {
        c->stream = hipStreamLegacy;              // the null stream: ordered with every blocking stream of the device
        c->own_stream = false;
    } else if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
        c->own_stream = false;
    } else {
        TA_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    return TA_OK;
}

TA_API int ta_ctx_set_option(ta_ctx* c, int key, int64_t value) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    switch (key) {
        case TA_OPT_IMPL:
            if (value < 0 || value > 1) return fail(TA_EINVAL, "TA_OPT_IMPL must be 0 (sweep) or 1 (per-voxel atomics)");
            c->impl = (int)value; return TA_OK;
        case TA_OPT_TILE_PLANES:
            if (value < 0 || value > ta::sweep_tile_planes_limit()) return fail(TA_EINVAL, "TA_OPT_TILE_PLANES must be in [0,%d]", ta::sweep_tile_planes_limit());
            c->tile_planes = (int)value; return TA_OK;
        case TA_OPT_PAIR_SLOTS:
            if (value != 0 && (value < 4 || value > 30)) return fail(TA_EINVAL, "TA_OPT_PAIR_SLOTS must be 0 or in [4,30]");
            c->opt_pair_log2 = (int)value; return TA_OK;
        case TA_OPT_SWEEP_SHAPE:
            if (value < -2 || value > 1) return fail(TA_EINVAL, "TA_OPT_SWEEP_SHAPE is -1 (by label-change density), -2 (by four timed sweeps), 0 or 1");
            c->shape.opt = (int)value;
            c->auto_tile_shift = 0;
            c->shape.forget_choice();              // (decided again, by the new rule, at the next sweep)
            return TA_OK;
        case TA_OPT_VOLUME_SLACK:
            if (value < 0) return fail(TA_EINVAL, "TA_OPT_VOLUME_SLACK must be >= 0");
            c->volume_slack = value; return TA_OK;
        case TA_OPT_TIMING:
            if (value < 0 || value > 2) return fail(TA_EINVAL, "TA_OPT_TIMING must be 0, 1 or 2");
            c->timing = (int)value; return TA_OK;
        case TA_OPT_TIMING_RING: {
            if (value < 1 || value > 4096) return fail(TA_EINVAL, "TA_OPT_TIMING_RING must be in [1,4096]");
            int rc = use_device(c);
            if (rc != TA_OK) return rc;
            if (c->stream) TA_HIP(hipStreamSynchronize(c->stream));
            const size_t want = 2 * (size_t)value;
            while (c->ring.size() > want) { (void)hipEventDestroy(c->ring.back()); c->ring.pop_back(); }
            while (c->ring.size() < want) {
                hipEvent_t ev = nullptr;
                TA_HIP(hipEventCreate(&ev));
                try { c->ring.push_back(ev); } catch (...) { (void)hipEventDestroy(ev); return fail(TA_ENOMEM, "out of host memory"); }
            }
            c->ring_since = c->extract_seq;          // the kept durations start with the next extraction
            return TA_OK;
        }
        case TA_OPT_SWEEP_SHAPE_USED:
        case TA_OPT_TILE_PLANES_USED:
            return fail(TA_EINVAL, "option key %d is read only", key);
        default:
            return fail(TA_EINVAL, "unknown option key %d", key);
    }
}

TA_API int ta_ctx_get_option(ta_ctx* c, int key, int64_t* value) {
    if (!c || !value) return fail(TA_EINVAL, "NULL argument");
    switch (key) {
        case TA_OPT_IMPL: *value = c->impl; return TA_OK;
        case TA_OPT_VOLUME_SLACK: *value = c->volume_slack; return TA_OK;
        case TA_OPT_SWEEP_SHAPE: *value = c->shape.opt; return TA_OK;
        case TA_OPT_SWEEP_SHAPE_USED: *value = c->shape.last; return TA_OK;
        case TA_OPT_TILE_PLANES_USED: *value = c->tile_planes_used; return TA_OK;
        case TA_OPT_TIMING: *value = c->timing; return TA_OK;
        case TA_OPT_TIMING_RING: *value = (int64_t)(c->ring.size() / 2); return TA_OK;
        case TA_OPT_TILE_PLANES: {
            const int shape = c->shape.opt >= 0 ? c->shape.opt : (c->shape.pick >= 0 ? c->shape.pick : 1);
            int planes = c->tile_planes > 0 ? c->tile_planes : ta::sweep_default_tile_planes(c->feature_mask & TA_F_ADJACENCY, c->itemsize, shape);
            if (c->tile_planes <= 0 && c->itemsize == 4 && (c->feature_mask & TA_F_ADJACENCY) && shape == 1 &&
                c->shape.density >= WIDE_SHORTER_TILES_DENSITY && planes > 28) planes = 28;      // (the rule of run_extract)
            *value = planes; return TA_OK;
        }
        case TA_OPT_PAIR_SLOTS: *value = c->pslots.p ? c->pair_log2 : c->opt_pair_log2; return TA_OK;
        default: return fail(TA_EINVAL, "unknown option key %d", key);
    }
}

TA_API int ta_ctx_synchronize(ta_ctx* c) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_volume_set(ta_ctx* c, const void* host_ptr, int itemsize, const int64_t dims[3],
                  const int64_t strides_bytes[3]) {
    if (!c || !host_ptr || !dims) return fail(TA_EINVAL, "NULL argument");
    if (itemsize != 2 && itemsize != 4) return fail(TA_EINVAL, "itemsize must be 2 (uint16) or 4 (uint32)");
    for (int d = 0; d < 3; ++d)
        if (dims[d] <= 0 || dims[d] > (1ll << 30)) return fail(TA_EINVAL, "dims[%d]=%lld out of range", d, (long long)dims[d]);
    int perm[3] = {0, 1, 2};
    if (strides_bytes) {
        // memory order = axes by decreasing stride (size-1 axes are layout-neutral: keep them first)
        std::stable_sort(perm, perm + 3, [&](int x, int y) {
            const int64_t sx = dims[x] == 1 ? INT64_MAX : strides_bytes[x];
            const int64_t sy = dims[y] == 1 ? INT64_MAX : strides_bytes[y];
            return sx > sy;
        });
        int64_t expect = itemsize;
        for (int k = 2; k >= 0; --k) {
            const int ax = perm[k];
            if (dims[ax] != 1 && strides_bytes[ax] != expect)
                return fail(TA_EINVAL, "strides do not describe a dense permuted layout (axis %d: stride %lld, expected %lld)",
                            ax, (long long)strides_bytes[ax], (long long)expect);
            expect *= dims[ax];
        }
    }
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint64_t bytes = (uint64_t)dims[0] * dims[1] * dims[2] * itemsize;
    TA_HIP(hipStreamSynchronize(c->stream));
    if ((rc = c->owned_vol.reserve(bytes + 64)) != TA_OK) return rc;      // (+ slack: see run_extract, vec_ok)
    TA_HIP(hipMemcpyAsync(c->owned_vol.p, host_ptr, bytes, hipMemcpyHostToDevice, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));   // the host buffer may be freed after return
    c->vol = c->owned_vol.p;
    c->itemsize = itemsize;
    for (int k = 0; k < 3; ++k) { c->perm[k] = perm[k]; c->mdims[k] = dims[perm[k]]; }
    c->a_origin = 0;
    c->first_owned = 0;
    volume_replaced(c);              // (volume_slack stays as it is: the library's own upload never looks at it)
    return TA_OK;
}

TA_API int ta_volume_set_device(ta_ctx* c, const void* dev_ptr, int itemsize, const int64_t buf_dims[3],
                         int64_t a0_origin, int has_low_halo) {
    if (!c || !dev_ptr || !buf_dims) return fail(TA_EINVAL, "NULL argument");
    if (itemsize != 2 && itemsize != 4) return fail(TA_EINVAL, "itemsize must be 2 (uint16) or 4 (uint32)");
    for (int d = 0; d < 3; ++d)
        if (buf_dims[d] <= 0 || buf_dims[d] > (1ll << 30)) return fail(TA_EINVAL, "buf_dims[%d]=%lld out of range", d, (long long)buf_dims[d]);
    if (has_low_halo && buf_dims[0] < 2) return fail(TA_EINVAL, "a slab with a halo needs at least 2 planes");
    if (a0_origin < 0) return fail(TA_EINVAL, "a0_origin must be >= 0");
    if (((uintptr_t)dev_ptr % itemsize) != 0) return fail(TA_EINVAL, "device pointer is not aligned to the label type");
    c->vol = dev_ptr;
    c->volume_slack = 0;             // (told again by the owner of the new buffer)
    c->itemsize = itemsize;
    for (int k = 0; k < 3; ++k) { c->perm[k] = k; c->mdims[k] = buf_dims[k]; }
    c->a_origin = a0_origin;
    c->first_owned = has_low_halo ? 1 : 0;
    volume_replaced(c);
    return TA_OK;
}

TA_API int ta_volume_relabel(ta_ctx* c, const uint32_t* lut, uint32_t lut_len) {
    if (!c || (!lut && lut_len)) return fail(TA_EINVAL, "NULL argument");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    if (c->first_owned) return fail(TA_EINVAL, "cannot relabel a slab that carries a halo plane");
    if (compact_rows(c) >= 0 && lut_len != (uint32_t)compact_rows(c))
        return fail(TA_EINVAL, "a compacted context relabels through one entry per rank: %u entries for %lld ranks", lut_len, (long long)compact_rows(c));
    if (c->itemsize == 2)
        for (uint32_t i = 0; i < lut_len; ++i)
            if (lut[i] > 0xFFFFu) return fail(TA_ERANGE, "lut[%u]=%u does not fit the uint16 volume", i, lut[i]);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if (lut_len == 0) return TA_OK;
    DevBuf d;
    if ((rc = d.reserve((uint64_t)lut_len * 4)) != TA_OK) return rc;
    hipError_t e = hipMemcpyAsync(d.p, lut, (uint64_t)lut_len * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        ta::launch_relabel(c->stream, sweep_vol(c), const_cast<void*>(c->vol), c->itemsize,
                           (uint64_t)c->mdims[0] * c->mdims[1] * c->mdims[2], (const uint32_t*)d.p, lut_len);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    d.release();
    if (e != hipSuccess) return fail(TA_EHIP, "relabel: %s", hipGetErrorString(e));
    volume_labels_changed(c);
    return TA_OK;
}

TA_API int ta_volume_get(ta_ctx* c, void* host_dst) {
    if (!c || !host_dst) return fail(TA_EINVAL, "NULL argument");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint64_t bytes = (uint64_t)c->mdims[0] * c->mdims[1] * c->mdims[2] * c->itemsize;
    TA_HIP(hipMemcpyAsync(host_dst, c->vol, bytes, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_volume_map(ta_ctx* c, const void* lut, uint32_t lut_len, const void* fill, int out_itemsize,
                         void* host_dst) {
    if (!c || !fill || !host_dst || (!lut && lut_len)) return fail(TA_EINVAL, "NULL argument");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    if (out_itemsize != 1 && out_itemsize != 2 && out_itemsize != 4 && out_itemsize != 8)
        return fail(TA_EINVAL, "out_itemsize must be 1, 2, 4 or 8");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint64_t n = (uint64_t)c->mdims[0] * c->mdims[1] * c->mdims[2];
    uint64_t fillw = 0;
    memcpy(&fillw, fill, (size_t)out_itemsize);
    DevBuf dl;
    if ((rc = dl.reserve((uint64_t)lut_len * out_itemsize + 8)) != TA_OK) return rc;
    rc = run_and_read_back(c, "map", n * out_itemsize, host_dst, [&](void* dout) {
        if (lut_len)
            if (const hipError_t e = hipMemcpyAsync(dl.p, lut, (uint64_t)lut_len * out_itemsize, hipMemcpyHostToDevice, c->stream); e != hipSuccess) return e;
        ta::launch_map(c->stream, sweep_vol(c), c->itemsize, dout, out_itemsize, n, dl.p, lut_len, fillw);     // (compacted: lut[rank])
        return hipGetLastError();
    });
    dl.release();
    return rc;
}

TA_API int ta_volume_first_layer(ta_ctx* c, uint32_t background, int keep_background, void* host_dst) {
    if (!c || !host_dst) return fail(TA_EINVAL, "NULL argument");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    if (c->first_owned) return fail(TA_EINVAL, "the first voxel layer is not available on a slab that carries a halo plane");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint64_t bytes = (uint64_t)c->mdims[0] * c->mdims[1] * c->mdims[2] * c->itemsize;
    return run_and_read_back(c, "first voxel layer", bytes, host_dst, [&](void* dout) {
        ta::launch_first_layer(c->stream, c->vol, c->itemsize, dout, c->mdims[0], c->mdims[1], c->mdims[2], background, keep_background ? 1 : 0);
        return hipGetLastError();
    });
}

TA_API int ta_volume_hollow(ta_ctx* c, uint32_t background, int remove_background, int label_bits, void* host_dst) {
    if (!c || !host_dst) return fail(TA_EINVAL, "NULL argument");
    if (label_bits == 0) label_bits = 8 * c->itemsize;
    if (label_bits != 8 && label_bits != 16 && label_bits != 32 && label_bits != 64) return fail(TA_EINVAL, "label_bits must be 0, 8, 16, 32 or 64");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    if (c->first_owned) return fail(TA_EINVAL, "hollowed-out cells are not available on a slab that carries a halo plane");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint64_t bytes = (uint64_t)c->mdims[0] * c->mdims[1] * c->mdims[2] * c->itemsize;
    return run_and_read_back(c, "hollowed-out cells", bytes, host_dst, [&](void* dout) {
        ta::launch_hollow(c->stream, c->vol, c->itemsize, dout, c->mdims[0], c->mdims[1], c->mdims[2], background, remove_background ? 1 : 0, label_bits);
        return hipGetLastError();
    });
}

TA_API int ta_volume_layer18(ta_ctx* c, uint8_t* host_dst) {
    if (!c || !host_dst) return fail(TA_EINVAL, "NULL argument");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    if (c->first_owned) return fail(TA_EINVAL, "the voxel layers are not available on a slab that carries a halo plane");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const uint64_t bytes = (uint64_t)c->mdims[0] * c->mdims[1] * c->mdims[2];
    return run_and_read_back(c, "voxel layers", bytes, host_dst, [&](void* dout) {
        ta::launch_layer18(c->stream, c->vol, c->itemsize, (uint8_t*)dout, c->mdims[0], c->mdims[1], c->mdims[2]);
        return hipGetLastError();
    });
}

TA_API int ta_volume_owned_planes(ta_ctx* c, int64_t* planes) {
    if (!c || !planes) return fail(TA_EINVAL, "NULL argument");
    *planes = c->vol ? c->mdims[0] - c->first_owned : 0;
    return TA_OK;
}

TA_API int ta_volume_plane_events(ta_ctx* c, uint64_t* events) {
    if (!c || !events) return fail(TA_EINVAL, "NULL argument");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const int64_t owned = c->mdims[0] - c->first_owned;
    if (owned <= 0) return TA_OK;
    const char* first = (const char*)c->vol + (size_t)c->first_owned * c->mdims[1] * c->mdims[2] * c->itemsize;
    return run_and_read_back(c, "plane events", (uint64_t)owned * sizeof(uint64_t), events, [&](void* d) {
        ta::launch_plane_events(c->stream, first, c->itemsize, owned, c->mdims[1], c->mdims[2], (uint64_t*)d);
        return hipGetLastError();
    });
}

TA_API int ta_bind_accumulators(ta_ctx* c, void* sums_dev, void* boxes_dev, uint32_t max_label) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if ((sums_dev == nullptr) != (boxes_dev == nullptr)) return fail(TA_EINVAL, "bind both buffers or neither");
    if (sums_dev && (((uintptr_t)sums_dev & 15) || ((uintptr_t)boxes_dev & 7)))
        return fail(TA_EINVAL, "bound accumulators must be 16-byte (sums) / 8-byte (boxes) aligned");
    c->bound = sums_dev != nullptr;
    c->bound_max_label = max_label;
    if (c->bound) { c->sums = (uint64_t*)sums_dev; c->boxes = (int32_t*)boxes_dev; }
    else { c->sums = nullptr; c->boxes = nullptr; }
    c->extracted = c->checked = false;
    return TA_OK;
}

TA_API int ta_extract(ta_ctx* c, uint32_t feature_mask, uint32_t max_label) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    if (feature_mask == 0 || (feature_mask & ~TA_F_ALL)) return fail(TA_EINVAL, "bad feature mask 0x%x", feature_mask);
    if (max_label >= (1u << 28)) return fail(TA_EINVAL, "max_label %u too large for dense per-label rows", max_label);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    {   // exactness guard: every u64 sum must stay below 2^64
        const long double g0 = (long double)(c->a_origin + c->mdims[0]), nv = (long double)c->mdims[0] * c->mdims[1] * c->mdims[2];
        const long double gm = std::max(g0, std::max((long double)c->mdims[1], (long double)c->mdims[2]));
        if (nv * gm * gm >= 1.8e19L) return fail(TA_EINVAL, "volume too large for exact 64-bit second moments");
    }
    const uint64_t nlabels = (uint64_t)max_label + 1;
    if (c->bound) {
        if (c->bound_max_label != max_label)
            return fail(TA_EINVAL, "bound accumulators are sized for max_label=%u, not %u", c->bound_max_label, max_label);
    } else {
        if ((rc = c->own_sums.reserve(nlabels * ta::NSUM * 8)) != TA_OK) return rc;
        if ((rc = c->own_boxes.reserve(nlabels * ta::NBOX * 4)) != TA_OK) return rc;
        c->sums = (uint64_t*)c->own_sums.p;
        c->boxes = (int32_t*)c->own_boxes.p;
    }
    c->max_label = max_label;
    c->feature_mask = feature_mask;
    {
        const bool adj = feature_mask & TA_F_ADJACENCY;
        // never below a size the table has already grown to (a fixed TA_OPT_PAIR_SLOTS is a starting size)
        int want = c->opt_pair_log2 ? std::max(c->opt_pair_log2, c->pslots.p ? c->pair_log2 : 0)
                                    : std::max(c->pslots.p ? c->pair_log2 : 4, adj ? auto_pair_log2(max_label) : 4);
        if ((rc = ensure_pair_table(c, want)) != TA_OK) return rc;
    }
    c->extracted = true;
    c->checked = false;
    c->exchanged = false;
    c->shared_packed = false;
    c->reduced = false;
    c->host_pairs_ready = false;
    return run_extract(c);
}

TA_API int ta_get_labels(ta_ctx* c, uint64_t* count, int32_t* bbox, uint64_t* sum1, uint64_t* sum2) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = finish_extract(c)) != TA_OK) return rc;
    const uint64_t n = (uint64_t)c->max_label + 1;
    std::vector<uint64_t> hs;
    std::vector<int32_t> hb;
    try {
        if (count || sum1 || sum2) hs.resize(n * ta::NSUM);
        if (bbox) hb.resize(n * ta::NBOX);
    } catch (...) { return fail(TA_ENOMEM, "out of host memory"); }
    if (!hs.empty()) TA_HIP(hipMemcpyAsync(hs.data(), c->sums, hs.size() * 8, hipMemcpyDeviceToHost, c->stream));
    if (!hb.empty()) TA_HIP(hipMemcpyAsync(hb.data(), c->boxes, hb.size() * 4, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    int slot[6];
    moment_slots(c, slot);
    const bool mom2 = c->feature_mask & TA_F_MOMENT2;
    if (c->perm[0] == 0 && c->perm[1] == 1 && c->perm[2] == 2) {
        // C-ordered input (array axes = memory axes): no permutation, one tight loop per output
        if (count) for (uint64_t l = 0; l < n; ++l) count[l] = hs[l * ta::NSUM];
        if (sum1) for (uint64_t l = 0; l < n; ++l) { sum1[3 * l] = hs[l * ta::NSUM + 1]; sum1[3 * l + 1] = hs[l * ta::NSUM + 2]; sum1[3 * l + 2] = hs[l * ta::NSUM + 3]; }
        if (sum2) {
            if (mom2) for (uint64_t l = 0; l < n; ++l) memcpy(sum2 + 6 * l, &hs[l * ta::NSUM + 4], 6 * sizeof(uint64_t));
            else memset(sum2, 0, n * 6 * sizeof(uint64_t));
        }
        if (bbox) for (uint64_t l = 0; l < n; ++l) {
            const bool present = hb[l * 6] != INT32_MAX;
            for (int k = 0; k < 3; ++k) { bbox[l * 6 + k] = present ? hb[l * 6 + k] : -1; bbox[l * 6 + 3 + k] = present ? (-hb[l * 6 + 3 + k] + 1) : -1; }
        }
        return TA_OK;
    }
    for (uint64_t l = 0; l < n; ++l) {
        if (count) count[l] = hs[l * ta::NSUM];
        if (sum1) for (int k = 0; k < 3; ++k) sum1[l * 3 + c->perm[k]] = hs[l * ta::NSUM + 1 + k];
        // (without TA_F_MOMENT2 the device columns are not defined -- the rare table-spill path writes cross terms there --
        //  and the getter answers zero)
        if (sum2) for (int q = 0; q < 6; ++q) sum2[l * 6 + slot[q]] = mom2 ? hs[l * ta::NSUM + 4 + q] : 0ull;
        if (bbox) {
            const bool present = hb[l * 6] != INT32_MAX;
            for (int k = 0; k < 3; ++k) {
                bbox[l * 6 + c->perm[k]] = present ? hb[l * 6 + k] : -1;
                bbox[l * 6 + 3 + c->perm[k]] = present ? (-hb[l * 6 + 3 + k] + 1) : -1;
            }
        }
    }
    return TA_OK;
}

TA_API int ta_adjacency_scope(ta_ctx* c, int* scope) {
    if (!c || !scope) return fail(TA_EINVAL, "NULL argument");
    if (!c->extracted || !(c->feature_mask & TA_F_ADJACENCY))
        return fail(TA_EINVAL, "no extraction with adjacency has been run on this context");
    *scope = !c->exchanged ? TA_ADJ_LOCAL : (c->shared_packed ? TA_ADJ_PARTIAL : TA_ADJ_MERGED);
    return TA_OK;
}

TA_API int ta_adjacency_size(ta_ctx* c, int64_t* npairs) {
    if (!c || !npairs) return fail(TA_EINVAL, "NULL argument");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = finish_extract(c)) != TA_OK) return rc;
    *npairs = c->npairs;
    return TA_OK;
}

TA_API int ta_adjacency_get(ta_ctx* c, uint32_t* lo, uint32_t* hi, uint64_t* faces) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = finish_extract(c)) != TA_OK) return rc;
    const uint64_t n = (uint64_t)c->npairs;
    if (!c->host_pairs_ready) {
        if ((rc = c->h_pairs.reserve(n * 32 + 16)) != TA_OK) return rc;
        if (n) {
            // sorted by (lo, hi) on the device (kernels_pairsort.hip: counting sort over the label rows, rank inside a bucket;
            // a std::sort of ~10^5 records used to cost more than the sweep, a 64-bit library radix sort 0.45 ms)
            if (n >= (1ull << 32)) return fail(TA_EINVAL, "too many pairs (%llu)", (unsigned long long)n);
            const uint64_t kb = n * 8;
            DevBuf& buf = c->sort_buf;
            if ((rc = buf.reserve(kb + n * 24 + ta::pairs_sort_scratch_bytes(n, c->max_label) + 64)) != TA_OK) return rc;
            char* p = (char*)buf.p;
            uint64_t* ks = (uint64_t*)p; p += kb;
            uint64_t* fo = (uint64_t*)p; p += n * 24;
            const bool has_voxel = sweep_vol(c) && c->mdims[0] - c->first_owned > 0 && c->mdims[1] > 0 && c->mdims[2] > 0;
            hipError_t e = ta::launch_pairs_sort(c->stream, (const uint64_t*)c->out_keys.p, (const uint64_t*)c->out_faces.p, n, c->max_label,
                                                 p, ks, fo, has_voxel ? sweep_vol(c) : nullptr, c->itemsize,
                                                 (int64_t)c->first_owned * c->mdims[1] * c->mdims[2]);
            // (keys and faces sit back to back in the sort's output: one copy)
            if (e == hipSuccess) e = hipMemcpyAsync(c->h_pairs.p, ks, n * 32, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return fail(TA_EHIP, "adjacency sort: %s", hipGetErrorString(e));
        }
        c->host_pairs_ready = true;
    }
    const bool identity = c->perm[0] == 0 && c->perm[1] == 1 && c->perm[2] == 2;
    const uint64_t* h_keys = (const uint64_t*)c->h_pairs.p;
    const uint64_t* h_faces = h_keys + n;
    if (c->ids.compact) {               // rows are ranks, label values are ids (order-preserving: the list stays sorted)
        const uint64_t nid = c->ids.h_ids.size();
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t a = h_keys[i] >> 32, b = h_keys[i] & 0xffffffffu;
            if (a >= nid || b >= nid) return fail(TA_ERANGE, "adjacency holds rank %llu, the census has %llu ids", (unsigned long long)std::max(a, b), (unsigned long long)nid);
            if (lo) lo[i] = c->ids.h_ids[a];
            if (hi) hi[i] = c->ids.h_ids[b];
        }
    } else {
        if (lo) for (uint64_t i = 0; i < n; ++i) lo[i] = (uint32_t)(h_keys[i] >> 32);
        if (hi) for (uint64_t i = 0; i < n; ++i) hi[i] = (uint32_t)(h_keys[i] & 0xffffffffu);
    }
    if (faces && identity && n) memcpy(faces, h_faces, n * 3 * sizeof(uint64_t));      // C-ordered input: a plain copy
    else if (faces) for (uint64_t i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) faces[3 * i + c->perm[k]] = h_faces[3 * i + k];
    return TA_OK;
}

TA_API int ta_timing(ta_ctx* c, double* ms_sweep, double* ms_adjacency, double* ms_total, uint64_t* bytes_read) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!c->extracted) return fail(TA_EINVAL, "no extraction has been run on this context");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const size_t nslots = c->ring.size() / 2;
    // (durations no event recorded are NaN, not 0: "not measured" must not read as "took no time" in a bandwidth figure)
    float a = NAN, b = NAN, t = NAN;
    if (c->extract_seq > c->ring_since && nslots) {          // the last extraction recorded its sweep events
        hipEvent_t ev_a = c->ring[2 * ((c->extract_seq - 1) % nslots)], ev_b = c->ring[2 * ((c->extract_seq - 1) % nslots) + 1];
        TA_HIP(hipEventSynchronize(ev_b));
        TA_HIP(hipEventElapsedTime(&a, ev_a, ev_b));
        if (c->timing >= 2) {
            TA_HIP(hipEventSynchronize(c->ev[3]));
            TA_HIP(hipEventElapsedTime(&b, ev_b, c->ev[3]));
            TA_HIP(hipEventElapsedTime(&t, c->ev[0], c->ev[3]));
        }
    }      // (else: the last extraction recorded no events -- TA_OPT_TIMING is 0)
    if (ms_sweep) *ms_sweep = a;
    if (ms_adjacency) *ms_adjacency = b;
    if (ms_total) *ms_total = t;
    if (bytes_read)
        *bytes_read = (uint64_t)(c->mdims[0] - c->first_owned) * c->mdims[1] * c->mdims[2] * c->itemsize;
    return TA_OK;
}

TA_API int ta_timing_series(ta_ctx* c, double* ms_sweep, int capacity, int* count) {
    if (!c || !count || (capacity > 0 && !ms_sweep) || capacity < 0) return fail(TA_EINVAL, "NULL ctx / output or negative capacity");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    const size_t nslots = c->ring.size() / 2;
    uint64_t first = c->ring_since, last = c->extract_seq;          // extractions [first, last) have valid events
    if (last - first > (uint64_t)capacity) first = last - (uint64_t)capacity;
    *count = 0;
    if (c->stream) TA_HIP(hipStreamSynchronize(c->stream));
    for (uint64_t q = first; q < last && nslots; ++q) {
        float ms = 0;
        TA_HIP(hipEventElapsedTime(&ms, c->ring[2 * (q % nslots)], c->ring[2 * (q % nslots) + 1]));
        ms_sweep[(*count)++] = ms;
    }
    return TA_OK;
}

TA_API int ta_read_probe(ta_ctx* c, const void* dev_ptr, uint64_t bytes, int repeats, double* ms_best) {
    if (!c || !dev_ptr || !ms_best) return fail(TA_EINVAL, "NULL argument");
    if (((uintptr_t)dev_ptr & 15) || bytes < 16) return fail(TA_EINVAL, "the probe needs a 16-byte aligned buffer of at least 16 bytes");
    if (repeats < 1) repeats = 1;
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if ((rc = settle_rerank(c)) != TA_OK) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    double best = -1.0;
    for (int r = 0; r < repeats + 1 && e == hipSuccess; ++r) {            // the first launch is a warm-up
        e = hipEventRecord(e0, c->stream);
        if (e == hipSuccess) { ta::launch_read_probe(c->stream, dev_ptr, bytes, maxlab_dev(c)); e = hipGetLastError(); }
        if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess && r > 0 && (best < 0 || ms < best)) best = ms;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return fail(TA_EHIP, "read probe: %s", hipGetErrorString(e));
    *ms_best = best;
    return TA_OK;
}

TA_API int ta_debug_counters(ta_ctx* c, uint32_t out[16]) {
    if (!c || !out) return fail(TA_EINVAL, "NULL argument");
    if (!c->extracted) return fail(TA_EINVAL, "no extraction has been run on this context");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    TA_HIP(hipStreamSynchronize(c->stream));
    for (int i = 0; i < 16; ++i) out[i] = i < ta::NFLAGS ? c->h_small[i] : 0u;
    return TA_OK;
}

TA_API int ta_synth_voronoi(ta_ctx* c, void* dev_out, int itemsize, const int64_t dims[3], int64_t a_begin,
                     int64_t a_count, const int32_t* seeds, const int32_t grid[3], const int64_t* ell) {
    if (!c || !dev_out || !dims || !seeds || !grid) return fail(TA_EINVAL, "NULL argument");
    if (itemsize != 2 && itemsize != 4) return fail(TA_EINVAL, "itemsize must be 2 or 4");
    if (a_begin < 0 || a_count < 0 || a_begin + a_count > dims[0]) return fail(TA_EINVAL, "plane range out of bounds");
    const int64_t ncell = (int64_t)grid[0] * grid[1] * grid[2];
    if (ncell <= 0) return fail(TA_EINVAL, "empty seed grid");
    if (itemsize == 2 && ncell + 1 > 65535) return fail(TA_EINVAL, "uint16 cannot hold %lld labels", (long long)ncell + 1);
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    DevBuf dseeds, dell;
    if ((rc = dseeds.reserve((uint64_t)ncell * 12)) != TA_OK) return rc;
    hipError_t e = hipMemcpyAsync(dseeds.p, seeds, (uint64_t)ncell * 12, hipMemcpyHostToDevice, c->stream);
    const uint64_t nell = (uint64_t)(dims[0] + dims[1] + dims[2]);
    if (e == hipSuccess && ell) {
        if ((rc = dell.reserve(nell * 8)) != TA_OK) { dseeds.release(); return rc; }
        e = hipMemcpyAsync(dell.p, ell, nell * 8, hipMemcpyHostToDevice, c->stream);
    }
    if (e == hipSuccess) {
        ta::launch_synth(c->stream, dev_out, itemsize, dims, a_begin, a_count, (const int32_t*)dseeds.p, grid,
                         ell ? (const int64_t*)dell.p : nullptr);
        e = hipStreamSynchronize(c->stream);
    }
    dseeds.release(); dell.release();
    if (e != hipSuccess) return fail(TA_EHIP, "ta_synth_voronoi: %s", hipGetErrorString(e));
    TA_HIP(hipGetLastError());
    return TA_OK;
}

TA_API int ta_device_malloc(ta_ctx* c, uint64_t bytes, void** dev_ptr) {
    if (!c || !dev_ptr) return fail(TA_EINVAL, "NULL argument");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    *dev_ptr = nullptr;
    if (hipMalloc(dev_ptr, bytes ? bytes : 16) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TA_ENOMEM, "hipMalloc of %llu bytes failed", (unsigned long long)bytes);
    }
    return TA_OK;
}

TA_API int ta_device_free(ta_ctx* c, void* dev_ptr) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    TA_HIP(hipStreamSynchronize(c->stream));
    if (dev_ptr) TA_HIP(hipFree(dev_ptr));
    return TA_OK;
}

TA_API int ta_memcpy_d2h(ta_ctx* c, void* host_dst, const void* dev_src, uint64_t bytes) {
    if (!c || (bytes && (!host_dst || !dev_src))) return fail(TA_EINVAL, "NULL argument");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    TA_HIP(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

TA_API int ta_memcpy_h2d(ta_ctx* c, void* dev_dst, const void* host_src, uint64_t bytes) {
    if (!c || (bytes && (!dev_dst || !host_src))) return fail(TA_EINVAL, "NULL argument");
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    TA_HIP(hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}

}  // extern "C"
