// ta_ctx.h -- the context behind the C ABI and what the ta_api*.hip files share (host only, private to csrc/).  Every concern has one
// struct of state below and its entry points in a file of its own: ta_api.hip holds the core (context, volume, sweep, extraction)
// and the sweep's tile shape; ta_api_walls.hip, ta_api_sparse.hip and ta_api_exchange.hip the wall voxels, the sparse label ids and
// the rank exchange; ta_api_<feature>.hip a feature.  What crosses files is declared here, with the file that defines it; the small
// checks that several features repeat are inline here: a feature's timed intervals above the state structs; what the passes over a
// settled extraction, the getters and the two separable transforms share below the context.  The formats that have a header of
// their own: the parts of a buffer (ta_parts.h), the count/scan block and the sort workspace of the count-then-emit passes
// (ta_counted.h), the launch plan of the range passes (ta_range_plan.h), the column passes and batches (ta_separable.h).
#pragma once
#include "../../include/tissue_scan.h"
#include "ta_counted.h"
#include "ta_kernels.h"
#include "ta_nearest.h"
#include "ta_parts.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

// sets the calling thread's ta_last_error and returns `code`
int fail(int code, const char* fmt, ...);

#define TA_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(e_ == hipErrorOutOfMemory ? TA_ENOMEM : TA_EHIP, "%s: %s (%s:%d)",  \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                   \
    } while (0)

// grow-only device memory (DevBuf), or page-locked host memory (PinnedBuf): device-to-host copies into it run at PCIe speed, into a
// std::vector they are staged
template <bool PINNED> struct Buf {
    void* p = nullptr;
    uint64_t bytes = 0;
    int reserve(uint64_t need) {
        if (need <= bytes) return TA_OK;
        release();
        if ((PINNED ? hipHostMalloc(&p, need ? need : 16, hipHostMallocDefault) : hipMalloc(&p, need ? need : 16)) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return fail(TA_ENOMEM, "%s of %llu bytes failed", PINNED ? "hipHostMalloc" : "hipMalloc", (unsigned long long)need);
        }
        bytes = need;
        return TA_OK;
    }
    void release() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; bytes = 0; }
};
using DevBuf = Buf<false>;
using PinnedBuf = Buf<true>;

inline uint64_t align16(uint64_t b) { return (b + 15) & ~15ull; }

// the events of a feature: created at its first pass, destroyed by its release()
template <size_t N> int ensure_events(hipEvent_t (&ev)[N]) {
    for (auto& e : ev) if (!e) TA_HIP(hipEventCreate(&e));
    return TA_OK;
}
template <size_t N> void destroy_events(hipEvent_t (&ev)[N]) { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }
inline int elapsed_ms(hipEvent_t a, hipEvent_t b, double* ms) {       // (both recorded and complete)
    float t = 0.f;
    TA_HIP(hipEventElapsedTime(&t, a, b));
    *ms = (double)t;
    return TA_OK;
}
inline int interval_ms(hipEvent_t a, hipEvent_t b, double* ms) {      // (both recorded: waits for b)
    TA_HIP(hipEventSynchronize(b));
    return elapsed_ms(a, b, ms);
}

// A companion volume: a second volume with the buffer dims and layout of the label volume (the signal image, the overlap's B).
struct Companion {
    const void* p = nullptr;                            // device pointer (owned.p or adopted), NULL = none
    DevBuf owned;
    int itemsize = 0;
    int64_t mdims[3] = {0, 0, 0};                       // the label buffer dims it was set for
};
struct CompanionKind { const char* noun; int size_a, size_b; };      // what the messages call it; the item sizes it takes

// signal image (include/tissue_scan_signal.h)
struct SignalState {
    Companion img;
    DevBuf out;                                         // flags u32[4] | n | sum | sumsq[2] | min | max | side_lo | side_hi
    DevBuf hash;                                        // pair -> row table of the sorted pair list: keys u64[cap] | rows u32[cap]
    uint64_t seq = 0;                                   // extract_seq of the extraction the results belong to, 0 = none
    uint32_t what = 0;
    uint32_t rows = 0;                                  // max_label + 1 of that extraction
    int64_t npairs = 0;
    ta::RangePlan plan;                                 // what the last pass was launched with (ta_signal_debug)
    hipEvent_t ev[2] = {nullptr, nullptr};
    void release() { img.owned.release(); out.release(); hash.release(); destroy_events(ev); }
};

// cell meshes (include/tissue_scan_mesh.h)
struct MeshState {
    DevBuf small;                                       // flags u32[4] | wanted u8[R] | count/scan block of the faces | of the corners
    DevBuf work;                                        // face records u64[F] | neighbours u32[F] | corners u64[V] | sort keys, values x 2 | sort temp
    DevBuf out;                                         // vertex corners u64[V] | vbeg, vend, fbeg, fend u64[R] | triangles u32[2F][3] | cell, neighbour u32[2F]
    uint64_t seq = 0;                                   // extract_seq of the extraction the mesh belongs to, 0 = none
    uint64_t faces = 0, verts = 0;
    uint32_t rows = 0;
    int64_t m[3] = {0, 0, 0};                           // dims of the meshed image, memory order
    bool host_ready = false;                            // cells and CSR offsets below are read back
    std::vector<uint32_t> cells;
    std::vector<uint64_t> voff, toff;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    void release() { small.release(); work.release(); out.release(); destroy_events(ev); }
};

// label overlap with a second label volume B (include/tissue_scan_overlap.h)
struct OverlapState {
    Companion b;
    DevBuf table;                                       // the device-global pair table: keys u64[slots] | counts u64[slots]
    DevBuf small;                                       // flags u32[4] | voxels of the pair (2^32 - 1, 2^32 - 1) u64
    DevBuf work;                                        // compaction: the count/scan block of the blocks of the table
    DevBuf sort;                                        // sort keys u64[P] x 2 | slots u32[P] x 2 | radix temp
    DevBuf rows;                                        // the sorted table: a u32[P] | b u32[P] | n u64[P]
    int opt_log2 = 0;                                   // ta_overlap_set_capacity: 0 = automatic
    int grown_log2 = 0;                                 // what an automatic table of this volume had to grow to
    int log2 = 0;                                       // slots of the table of the pass in flight
    int state = 0;                                      // 0 = no table, 1 = pass enqueued, 2 = settled (rows holds npairs rows)
    int passes = 0;                                     // runs of the pass kernel for this table
    ta::RangePlan plan;                                 // what the last run was launched with (ta_overlap_debug)
    uint32_t lds_spills = 0;                            // OV_FLAG_LDS_SPILL of the last run, kept by overlap_settle
    uint64_t npairs = 0;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // pass begin, end | count + scan end | emit begin, rows end
    void release() { b.owned.release(); table.release(); small.release(); work.release(); sort.release(); rows.release(); destroy_events(ev); }
};

// cell junctions (include/tissue_scan_junctions.h): index 0 = edges (3 labels), 1 = vertices (4 labels)
struct JunctionState {
    DevBuf small;                                       // blocks of order >= 5 u64
    DevBuf work;                                        // per wave: the count/scan block of the edge records | of the vertex records
    DevBuf rec;                                         // records: origins u64[N3] | origins u64[N4] | labels u32[N3][3] | labels u32[N4][4]
    DevBuf sort[2];                                     // sort keys u64[N] x 2 | order u32[N] x 2 | radix temp | count/scan block of the row heads
    DevBuf rows[2];                                     // the table: n u64[R] | sums u64[R][3] | labels u32[R][K]
    int state = 0;                                      // 0 = no tables, 1 = counting walk enqueued, 2 = settled
    uint64_t waves = 0;                                 // waves (= tasks) of a walk
    uint64_t nrows[2] = {0, 0}, degenerate = 0;
    uint32_t key_groups[2] = {0, 0};                    // workgroups of the key kernel of the last settle (ta_junctions_debug), 0 = no records
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // count begin, end | scans end | emit begin, end | tables end
    void release() { small.release(); work.release(); rec.release(); for (int k = 0; k < 2; ++k) { sort[k].release(); rows[k].release(); } destroy_events(ev); }
};

// wall geometry (include/tissue_scan_wallgeo.h)
struct WallGeoState {
    DevBuf out;                                         // flags u32[4] | rows u64[P][15]: fwd | rev | sum1 | sum2, memory-axis order
    DevBuf hash;                                        // pair -> row table of the sorted pair list: keys u64[cap] | sorted keys | rows u32[cap]
    uint64_t seq = 0;                                   // extract_seq of the extraction the rows belong to, 0 = none
    int64_t npairs = 0;
    ta::RangePlan plan;                                 // what the last pass was launched with; 0, 0 when it had no pair and was not launched
    hipEvent_t ev[2] = {nullptr, nullptr};
    void release() { out.release(); hash.release(); destroy_events(ev); }
};

// connected components of the labels (include/tissue_scan_components.h)
struct ComponentState {
    DevBuf parent;                                      // u32[voxels]: the union-find forest, then root / flagged slot: the row image's source
    DevBuf work;                                        // per wave: the count/scan block of the roots (offsets: the first slot of a wave)
    DevBuf slots;                                       // per slot: root u32[S] | row u32[S] | n u64[S] | sum1 u64[S][3] | first u64[S] | box i32[S][6]
    DevBuf sort;                                        // sort keys u64[S] x 2 | order u32[S] x 2 | radix temp
    DevBuf rows;                                        // the table, S rows of room: label u32 | n u64 | first i32[3] | bbox i32[6] | sum1 u64[3]
    DevBuf small;                                       // slots with owned voxels u64
    DevBuf image;                                       // staging of ta_components_image and of ta_components_relabel's table
    int state = 0;                                      // 0 = no tables, 1 = union-find and count enqueued, 2 = settled
    uint64_t waves = 0, nslots = 0, nrows = 0;
    uint32_t launched[4] = {0, 0, 0, 0};                // what the last pass launched (ta_components_debug): local tiles | seam groups | last image or relabel groups | key groups
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // union-find begin, end | scan end | emit begin, statistics end | table end
    void release() { parent.release(); work.release(); slots.release(); sort.release(); rows.release(); small.release(); image.release(); destroy_events(ev); }
};

// distance maps (include/tissue_scan_distance.h)
struct DistanceState {
    DevBuf d2;                                          // f64[voxels]: the image
    DevBuf work;                                        // envelope stacks of a batch of columns: f f64[len][B] | boundaries f64[len][B] | positions i32[len][B]
    DevBuf table;                                       // min2 u64[R] | max2 u64[R] | pole u64[R] | flags u32[4]
    uint64_t seq = 0;                                   // extract_seq of the extraction the results belong to, 0 = none
    uint32_t rows = 0;                                  // max_label + 1 of that extraction
    int64_t opt_batch = 0;                              // ta_distance_set_batch: 0 = automatic
    ta::DistanceLaunch launched;                        // what the last pass launched (ta_distance_debug)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};     // passes begin, end | table end
    void release() { d2.release(); work.release(); table.release(); destroy_events(ev); }
};

// nearest-label maps (include/tissue_scan_nearest.h)
struct NearestState {
    DevBuf f;                                           // f64[voxels]: D2
    DevBuf lab;                                         // u32[voxels]: N, as the volume the passes read stores labels
    DevBuf work;                                        // envelope stacks of a batch of columns: f f64[len][B] | boundaries f64 | positions i32 | labels u32 | boundary labels u32
    DevBuf table;                                       // gained u64[R] | totals u64[2] | flags u32[4]
    uint64_t seq = 0;                                   // extract_seq of the extraction the results belong to, 0 = none
    uint32_t rows = 0;                                  // max_label + 1 of that extraction
    int64_t opt_batch = 0;                              // ta_nearest_set_batch: 0 = automatic
    ta::NearestArgs args = {};                          // what the last pass ran with: ta_nearest_apply fills by the same rule
    uint32_t launched[4] = {0, 0, 0, 0};                // what the last pass launched (ta_nearest_debug)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};     // passes begin, end | counts end
    void release() { f.release(); lab.release(); work.release(); table.release(); destroy_events(ev); }
};

// distance-shell profiles (include/tissue_scan_profile.h)
struct ProfileState {
    DevBuf out;                                         // flags u32[4] | edges f64[65] | n u64[R][K] | with a signal: sum | sumsq[2] | min u32 | max u32
    double edges[65] = {0.0};                           // what the last pass's edges were copied to the device from: edges2[0 .. K], +inf behind
    uint64_t seq = 0;                                   // extract_seq of the extraction (and of the distance map) the table belongs to, 0 = none
    uint32_t rows = 0, bins = 0;                        // R = max_label + 1 of that extraction, K
    bool with_signal = false;                           // the pass read the signal: a new signal makes the table stale
    ta::RangePlan plan;                                 // what the last pass was launched with (ta_profile_debug)
    hipEvent_t ev[2] = {nullptr, nullptr};
    void release() { out.release(); destroy_events(ev); }
};

// signal histograms and order statistics (include/tissue_scan_sighist.h)
struct SigHistState {
    DevBuf out;                                         // flags u32[4] | counts u64[R][B]
    DevBuf rank;                                        // flags u32[2][4] | ranks u64[R][n] | rem u64[R][n] | hi, sel, map, values u32[R][n] | counts u64[R][256] | uint16: counts u64[R][n][256]
    std::vector<uint64_t> h_ranks;                      // what the last ta_sigrank_extract's ranks were copied to the device from
    uint64_t hist_seq = 0, rank_seq = 0;                // extract_seq of the extraction each table belongs to, 0 = none
    uint32_t rows = 0, bins = 0;                        // R = max_label + 1 of the histogram's extraction, B
    uint32_t rank_rows = 0, nranks = 0;                 // R and n of the order statistics
    int rank_passes = 0;                                // digit passes of the last ta_sigrank_extract: 1 (uint8) or 2 (uint16)
    int last = 0;                                       // whose digit pass ran last (ta_sighist_debug): 1 = histogram, 2 = order statistics
    ta::RangePlan plan;                                 // what that pass was launched with
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};       // histogram begin, end | order statistics begin, end
    void release() { out.release(); rank.release(); destroy_events(ev); }
};

// signal-weighted moments (include/tissue_scan_sigmoments.h)
struct SigMomentState {
    DevBuf out;                                         // flags u32[4] | n u64[R] | w u64[R] | m1 u64[R][3] | m2 u64[R][6][2]
    uint64_t seq = 0;                                   // extract_seq of the extraction the rows belong to, 0 = none
    uint32_t rows = 0;                                  // max_label + 1 of that extraction
    ta::RangePlan plan;                                 // what the last pass was launched with (ta_sigmom_debug)
    hipEvent_t ev[2] = {nullptr, nullptr};
    void release() { out.release(); destroy_events(ev); }
};

// two-channel statistics (include/tissue_scan_cosignal.h): channel A is SignalState::img
struct CoSignalState {
    Companion b;                                        // channel B
    DevBuf out;                                         // flags u32[4] | n | sum_a | sum_b u64[R] | sq_aa | sq_bb | sq_ab u64[R][2] | n_a | n_b | n_ab | over_a | over_b u64[R]
    uint64_t seq = 0;                                   // extract_seq of the extraction the rows belong to, 0 = none
    uint32_t rows = 0;                                  // max_label + 1 of that extraction
    uint32_t thr[2] = {0, 0};                           // the thresholds of the last pass (ta_cosignal_thresholds)
    ta::RangePlan plan;                                 // what the last pass was launched with (ta_cosignal_debug)
    hipEvent_t ev[2] = {nullptr, nullptr};
    void release() { b.owned.release(); out.release(); destroy_events(ev); }
};

// Euler numbers (include/tissue_scan_topology.h)
struct TopologyState {
    DevBuf out;                                         // flags u32[4] | mixed blocks u64 | n0 u64[R] | n1 u64[R][3] | n2 u64[R][3] | n3 u64[R] | v u64[R] | e u64[R][3]
    uint64_t seq = 0;                                   // extract_seq of the extraction the rows belong to, 0 = none
    uint32_t rows = 0;                                  // max_label + 1 of that extraction
    ta::RangePlan plan;                                 // what the last pass was launched with (ta_topology_debug)
    hipEvent_t ev[2] = {nullptr, nullptr};
    void release() { out.release(); destroy_events(ev); }
};

// oriented extents (include/tissue_scan_extents.h)
struct ExtentState {
    DevBuf out;                                         // flags u32[4] | keys of lo u64[R][3] | keys of hi u64[R][3]
    DevBuf weights;                                     // f64[R][3][3]: the table of the last pass
    std::vector<double> h_weights;                      // what that table was copied to the device from
    uint64_t seq = 0;                                   // extract_seq of the extraction the rows belong to, 0 = none
    uint32_t rows = 0;                                  // max_label + 1 of that extraction
    ta::RangePlan plan;                                 // what the last pass was launched with (ta_extents_debug)
    hipEvent_t ev[2] = {nullptr, nullptr};
    void release() { out.release(); weights.release(); destroy_events(ev); }
};

// resampling a second volume onto the label grid (include/tissue_scan_resample.h)
struct ResampleState {
    const void* src = nullptr;                          // device pointer (owned_src.p or adopted), NULL = none
    DevBuf owned_src;
    int src_itemsize = 0;
    int64_t sdims[3] = {0, 0, 0}, sel[3] = {0, 0, 0};   // source dims and element strides, array-axis order
    DevBuf out;                                         // the result: the label volume's buffer dims and layout, the source's type
    DevBuf small;                                       // outside u64
    bool valid = false;                                 // out holds the result of a pass over the current grid
    int itemsize = 0, mode = 0;                         // of that result
    bool vec = false;                                   // that pass wrote whole strips (ta_resample_debug)
    int64_t mdims[3] = {0, 0, 0}, a_origin = 0;         // the grid it was computed for
    int first_owned = 0;
    ta::RangePlan plan;                                 // what the last pass was launched with (ta_resample_debug)
    hipEvent_t ev[2] = {nullptr, nullptr};
    void release() { owned_src.release(); out.release(); small.release(); destroy_events(ev); }
};

// wall voxels and wall medians (ta_api_walls.hip)
struct WallVoxelState {
    DevBuf counts;                                      // per-chunk record counts, then offsets
    DevBuf stage;                                       // the records the count pass staged (kept until the volume is replaced)
    DevBuf medians;                                     // ta_wall_medians: pairs u32[E][2] | sizes u32[E] | medians i32[E][3]
    int64_t records = -1;                               // result of the last ta_wall_voxels_count, -1 = none
    uint32_t region = 0, not_staged = 0;                // records per staging region of that call (0 = nothing staged); cells left to the second walk
    int64_t median_count = -1;                          // E of the last ta_wall_medians, -1 = none
    bool wide = false;                                  // that call met a label >= 2^31
    uint32_t label_or = 0;                              // OR of all labels of the volume (that call): the bits a label takes
    double ms = 0.0;
    void release() { counts.release(); stage.release(); medians.release(); }
};

// sparse label ids (ta_api_sparse.hip): the census of the volume's ids and the copy of the volume in their ranks (what the sweep then reads)
struct SparseIdState {
    DevBuf census, census_ids, compact_vol, census_list;      // (census_list: the label list of the one-pass census, ~n / 256 entries)
    uint32_t census_max = 0;            // ids 0 .. census_max have a bit
    int64_t census_n = -1;              // ids present, -1 = no census
    int64_t vol_max = -1;               // largest label of the resident buffer (halo included), -1 = not known
    bool compact = false;               // per-label ROWS are ranks 0 .. census_n - 1; every label VALUE handed out is an id
    bool census_of_volume = false;      // the census on the context was taken from THIS volume (not a caller's id list)
    bool rerank_check = false;          // ta_volume_rerank's "id not in the list" word has not been looked at yet
    std::vector<uint32_t> h_ids;        // rank -> id (host copy, compact mode)
    void release() { census.release(); census_ids.release(); compact_vol.release(); census_list.release(); }
};

// the tile shape of the sweep of a uint32 volume with adjacency (kernels_scan.hip; state of ta_api.hip's sweep_shape): both give the
// same results; which one is faster depends on the tissue (background around it: the wide one; cells everywhere: the narrow one), so
// the first four sweeps of a volume take turns (wide, narrow, wide, narrow) between two events each, and the faster shape keeps the volume
struct SweepShapeState {
    int opt = -1;                                       // TA_OPT_SWEEP_SHAPE: -1 = measure, 0 / 1 = as told
    int pick = -1;                                      // choice for this volume, -1 = not yet
    double density = -1.0;                              // label changes per voxel in the sampled planes (what decided it), -1 = not measured
    int last = 0;                                       // TA_OPT_SWEEP_SHAPE_USED: the shape of the last sweep
    int tune_launched = 0;                              // measuring sweeps launched (0 .. 4)
    hipEvent_t tune_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool tune_done[4] = {false, false, false, false};
    float tune_ms[4] = {0.f, 0.f, 0.f, 0.f};
    void forget_choice() {                              // decided again at the next sweep (new voxels, or a new rule)
        pick = -1;
        density = -1.0;
        tune_launched = 0;
        for (bool& d : tune_done) d = false;
    }
    void release() { destroy_events(tune_ev); }
};

struct ta_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // [0] step begin, [3] step end (TA_OPT_TIMING = 2 only)
    std::vector<hipEvent_t> ring;                       // 2 events per slot around the sweep kernel of the last `ring.size()/2` extractions
    int timing = 1;                                     // TA_OPT_TIMING
    uint64_t extract_seq = 0, ring_since = 0;           // extractions run; the one the ring's oldest valid slot belongs to

    // resident volume
    const void* vol = nullptr;       // device pointer (owned_vol.p or adopted)
    DevBuf owned_vol;
    int itemsize = 0;
    int64_t mdims[3] = {0, 0, 0};    // buffer dims in memory-axis order
    int perm[3] = {0, 1, 2};         // perm[k] = array axis of memory axis k
    int64_t a_origin = 0;
    int first_owned = 0;

    // accumulators
    DevBuf own_sums, own_boxes;
    uint64_t* sums = nullptr;
    int32_t* boxes = nullptr;
    bool bound = false;
    uint32_t bound_max_label = 0;
    uint32_t max_label = 0;

    // adjacency
    DevBuf pslots, out_keys, out_faces, small;         // small: flags[NFLAGS] | cursor | maxlabel
    DevBuf hot_rows;                                    // [workgroups][16] private rows of the hot label
    DevBuf sort_buf;                                    // scratch of ta_adjacency_get's device sort (kept between calls)
    int pair_log2 = 0;                                  // current table log2 capacity
    int opt_pair_log2 = 0;
    bool table_clean = false;
    uint32_t* h_small = nullptr;                        // pinned, device-mapped mirror of `small`
    uint32_t* h_small_dev = nullptr;                    // its device address: the last kernel of a step writes it

    // options / state
    int impl = 0;
    int tile_planes = 0;
    int tile_planes_used = 0;                           // TA_OPT_TILE_PLANES_USED: the height the last sweep was launched with
    int64_t volume_slack = 0;                           // TA_OPT_VOLUME_SLACK: bytes readable behind an adopted volume
    int auto_tile_shift = 0;                            // automatic tile height halved this many times (table spills seen)
    uint64_t last_grid = 0;                             // workgroups of the last sweep
    uint32_t feature_mask = 0;
    bool extracted = false, checked = false;
    bool exchanged = false;                             // adjacency rebuilt by ta_adjacency_merge_blocks
    bool shared_packed = false;                         // ... from ta_adjacency_pack_shared blocks: the list is PARTIAL
    bool reduced = false;                               // the bound accumulators hold other ranks' contributions too
    int64_t npairs = 0;
    PinnedBuf h_pairs;                                  // sorted host copy for ta_adjacency_get: keys u64[n], then faces u64[n][3]
    bool host_pairs_ready = false;

    // one struct per concern: each one's state is written by its own file only (the core reads ids.compact / h_ids for the sweep)
    WallVoxelState walls;
    SparseIdState ids;
    SweepShapeState shape;
    SignalState sig;
    MeshState mesh;
    OverlapState ov;
    JunctionState jn;
    WallGeoState wg;
    ComponentState cc;
    DistanceState dist;
    NearestState near;
    ProfileState prof;
    SigHistState sh;
    SigMomentState sm;
    CoSignalState co;
    TopologyState tp;
    ExtentState ex;
    ResampleState rs;
};

inline int use_device(ta_ctx* c) {
    TA_HIP(hipSetDevice(c->device));
    return TA_OK;
}

// the volume the sweep reads: the rank copy in compact mode
inline const void* sweep_vol(const ta_ctx* c) { return c->ids.compact ? c->ids.compact_vol.p : c->vol; }
inline int64_t compact_rows(const ta_ctx* c) { return c->ids.compact ? c->ids.census_n : -1; }      // rows of a compacted context, -1 = dense

// Drain the stream and validate the flags of the last pass; grows the adjacency table and re-runs when it overflowed.  ta_api.hip.
int finish_extract(ta_ctx* c);

// What the passes over a settled extraction share.  pass_current: results tagged `seq` belong to the extraction the context holds.
inline bool pass_current(const ta_ctx* c, uint64_t seq) { return seq != 0 && c->extracted && seq == c->extract_seq; }
// the entry checks behind a pass's own (`noun` is what its messages call it, "signal pass"): the device, an extraction, its flags settled
inline int extraction_preflight(ta_ctx* c, const char* noun) {
    int rc = use_device(c);
    if (rc != TA_OK) return rc;
    if (!c->extracted) return fail(TA_EINVAL, "the %s needs a ta_extract of the current volume first", noun);
    return finish_extract(c);
}
// the N flag words a pass left at `dev`, once the stream has drained; each feature reads its own meaning into them
template <int N> int read_pass_flags(ta_ctx* c, const void* dev, uint32_t* flags) {
    TA_HIP(hipMemcpyAsync(flags, dev, N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}
// ... of a range pass whose words are RANGE = 0 (a label above max_label), SPILL = 1 (records that missed a workgroup's LDS table),
// of `sets` (1 or 2) passes in a row at `dev`; `noun` is what the message calls the pass; spills: those of the last set
constexpr int RANGE_NFLAGS = 4, RANGE_FLAG_RANGE = 0, RANGE_FLAG_SPILL = 1;
inline int range_pass_finish(ta_ctx* c, const void* dev, const char* noun, uint32_t* spills = nullptr, int sets = 1) {
    uint32_t f[2 * RANGE_NFLAGS] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int rc = sets == 2 ? read_pass_flags<2 * RANGE_NFLAGS>(c, dev, f) : read_pass_flags<RANGE_NFLAGS>(c, dev, f);
    if (rc != TA_OK) return rc;
    if (f[RANGE_FLAG_RANGE] || f[RANGE_NFLAGS + RANGE_FLAG_RANGE])
        return fail(TA_ERANGE, "the %s met a label above max_label=%u (the volume changed since ta_extract)", noun, c->max_label);
    if (spills) *spills = f[(sets - 1) * RANGE_NFLAGS + RANGE_FLAG_SPILL];
    return TA_OK;
}
// the four words of a range pass's ta_*_debug: two of its own (spills first, where it counts them), then the launch plan
inline void range_debug_words(uint32_t out[4], uint32_t first, uint32_t second, const ta::RangePlan& plan) {
    if (out) { out[0] = first; out[1] = second; out[2] = plan.tiles_per_group; out[3] = plan.groups; }
}

// What the getters share.  results_ready: the entry checks of a getter whose results are tagged with an extraction (or a volume);
// `current(c)` is the table's own predicate, asked only of a context that is there; `no_results` the feature's own message.
template <class Current> int results_ready(ta_ctx* c, Current current, const char* no_results) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!current(c)) return fail(TA_EINVAL, "%s", no_results);
    return use_device(c);
}
// read_columns: the parts of the buffer at `base` into the host arrays that want them (a NULL destination, an empty part: skipped),
// in list order, then one drain of the stream
struct Column { void* dst; Part part; };
inline int read_columns(ta_ctx* c, const void* base, std::initializer_list<Column> columns) {
    for (const Column& col : columns)
        if (col.dst && col.part.bytes)
            TA_HIP(hipMemcpyAsync(col.dst, (const char*)base + col.part.at, col.part.bytes, hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    return TA_OK;
}
// pass_timing: a ta_*_timing of one interval; `events(c)` gives the two events of a pass that "has run" by the feature's own
// rule, NULL otherwise (`none` is its message then)
template <class Events> int pass_timing(ta_ctx* c, double* ms, Events events, const char* none) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!ms) return fail(TA_EINVAL, "NULL argument");
    hipEvent_t* ev = events(c);
    if (!ev) return fail(TA_EINVAL, "%s", none);
    const int rc = use_device(c);
    return rc != TA_OK ? rc : interval_ms(ev[0], ev[1], ms);
}
// host_alloc: host allocations of an entry point run inside it, so that no exception leaves an extern "C" function
template <class Allocate> int host_alloc(Allocate allocate) {
    try { allocate(); } catch (...) { return fail(TA_ENOMEM, "out of host memory"); }
    return TA_OK;
}

// Axis arithmetic.  moment_slots: second moments come in the order 00 01 02 11 12 22 of their axis pair; slot[q] is where the
// q-th pair of MEMORY axes lies among the pairs of ARRAY axes.  array_key_strides: the stride of memory axis k in a key that
// counts voxels in the C order of the ARRAY axes.
inline void moment_slots(const ta_ctx* c, int slot[6]) {
    auto pair_slot = [](int x, int y) { if (x > y) std::swap(x, y); return x == 0 ? y : (x == 1 ? 2 + y : 5); };
    static const int mem_pair[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    for (int q = 0; q < 6; ++q) slot[q] = pair_slot(c->perm[mem_pair[q][0]], c->perm[mem_pair[q][1]]);
}
inline void array_dims(const ta_ctx* c, int64_t dims[3]) { for (int k = 0; k < 3; ++k) dims[c->perm[k]] = c->mdims[k]; }
inline void array_key_strides(const ta_ctx* c, uint64_t key_stride[3]) {
    int64_t dims[3];
    array_dims(c, dims);
    const uint64_t array_stride[3] = {(uint64_t)dims[1] * (uint64_t)dims[2], (uint64_t)dims[2], 1ull};
    for (int k = 0; k < 3; ++k) key_stride[k] = array_stride[c->perm[k]];
}

inline uint64_t voxels(const ta_ctx* c) { return (uint64_t)c->mdims[0] * (uint64_t)c->mdims[1] * (uint64_t)c->mdims[2]; }

// an id as the volume the passes read stores it; false when no voxel can hold it
inline bool stored_label(const ta_ctx* c, uint32_t id, uint32_t* stored) {
    *stored = id;
    if (!c->ids.compact) return c->itemsize == 4 || id <= 0xFFFFu;
    const auto& ids = c->ids.h_ids;                 // the passes read ranks: the id's rank, if the volume holds it
    const auto it = std::lower_bound(ids.begin(), ids.end(), id);
    *stored = (uint32_t)(it - ids.begin());
    return it != ids.end() && *it == id;
}

// the plane range of a ta_*_image call lies inside the buffer
inline int check_planes(const ta_ctx* c, int64_t first_plane, int64_t nplanes) {
    if (first_plane < 0 || nplanes < 0 || first_plane > c->mdims[0] || nplanes > c->mdims[0] - first_plane)
        return fail(TA_EINVAL, "planes %lld .. %lld are not inside the buffer's %lld", (long long)first_plane, (long long)(first_plane + nplanes),
                    (long long)c->mdims[0]);
    return TA_OK;
}

// the two intervals between three recorded events of a feature, once the last one is complete; either output may be NULL
inline int two_intervals_ms(hipEvent_t (&ev)[3], double* ms_first, double* ms_second) {
    TA_HIP(hipEventSynchronize(ev[2]));
    double first = 0.0, second = 0.0;
    int rc;
    if ((rc = elapsed_ms(ev[0], ev[1], &first)) != TA_OK || (rc = elapsed_ms(ev[1], ev[2], &second)) != TA_OK) return rc;
    if (ms_first) *ms_first = first;
    if (ms_second) *ms_second = second;
    return TA_OK;
}

// The whole-volume separable transforms (ta_api_distance.hip, ta_api_nearest.hip; `noun` is what their messages call the pass, "distance pass").
// Their entry checks run in this order: check_spacing, then transform_preflight, which settles the extraction the pass reads and
// fills w, the spacing of memory axis k.
inline int check_spacing(const double spacing[3]) {
    if (!spacing) return fail(TA_EINVAL, "spacing is NULL");
    for (int k = 0; k < 3; ++k)
        if (!(spacing[k] > 0.0) || !std::isfinite(spacing[k])) return fail(TA_EINVAL, "spacing[%d]=%g is not positive and finite", k, spacing[k]);
    return TA_OK;
}
inline int transform_preflight(ta_ctx* c, const char* noun, const double spacing[3], double w[3]) {
    if (!c->vol) return fail(TA_EINVAL, "no label volume set");
    if (c->first_owned != 0 || c->a_origin != 0)
        return fail(TA_EINVAL, "the %s does not take a slab (an exact transform needs halos of unbounded depth)", noun);
    const int rc = extraction_preflight(c, noun);
    if (rc != TA_OK) return rc;
    for (int k = 0; k < 3; ++k) w[k] = spacing[c->perm[k]];
    return TA_OK;
}
inline int check_batch_option(const ta_ctx* c, int64_t columns) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (columns < 0 || columns > (1ll << 30)) return fail(TA_EINVAL, "the columns of a batch must be 0 (automatic) or in [1, 2^30]");
    return TA_OK;
}

// ta_ctx::small and its host mirror h_small: flags, cursor, max label, parked hot-row pointer (2 words)
constexpr int SMALL_WORDS = ta::SMALL_WORDS_DEV;
inline uint32_t* flags_dev(ta_ctx* c) { return (uint32_t*)c->small.p; }
inline uint32_t* cursor_dev(ta_ctx* c) { return (uint32_t*)c->small.p + ta::NFLAGS; }
inline uint32_t* maxlab_dev(ta_ctx* c) { return (uint32_t*)c->small.p + ta::NFLAGS + 1; }
inline ta::PairTable pair_table(ta_ctx* c) {
    ta::PairTable pt;
    pt.slots = (ta::PairSlot*)c->pslots.p;       // (device allocations are aligned far beyond a slot's 32 bytes)
    pt.unused = 0;
    pt.mask = (uint32_t)((1ull << c->pair_log2) - 1);
    return pt;
}

// A new label volume (for the sparse ids, the overlap, the junctions, the components, the distance maps and their profiles, the nearest-label maps also: new label values in it).  Defined by
// the file of each concern, called by the core's volume_replaced / volume_labels_changed (the junctions' and the components' also by
// ta_volume_rerank: the caller edited the labels in place).
void walls_on_new_volume(ta_ctx* c);
void sparse_on_new_volume(ta_ctx* c);
void signal_on_new_volume(ta_ctx* c);
void overlap_on_new_volume(ta_ctx* c);
void junctions_on_new_volume(ta_ctx* c);
void wallgeo_on_new_volume(ta_ctx* c);
void components_on_new_volume(ta_ctx* c);
void distance_on_new_volume(ta_ctx* c);
void nearest_on_new_volume(ta_ctx* c);
void profile_on_new_volume(ta_ctx* c);
void profile_on_new_distance(ta_ctx* c);              // a new ta_distance_extract: the image the table was read from is gone.  ta_api_profile.hip
void profile_on_new_signal(ta_ctx* c);                // a new signal image: stale when the pass read the old one.  ta_api_profile.hip
void sighist_on_new_volume(ta_ctx* c);
void sighist_on_new_signal(ta_ctx* c);                // a new signal image: both tables read the old one.  ta_api_sighist.hip
void sigmom_on_new_volume(ta_ctx* c);
void sigmom_on_new_signal(ta_ctx* c);                 // a new signal image: the rows read the old one.  ta_api_sigmoments.hip
void cosig_on_new_volume(ta_ctx* c);                  // ... and a B of other dims is dropped.  ta_api_cosignal.hip
void cosig_on_new_signal(ta_ctx* c);                  // a new signal image: the rows read the old one as their channel A.  ta_api_cosignal.hip
void topology_on_new_volume(ta_ctx* c);
void extents_on_new_volume(ta_ctx* c);
void resample_on_new_volume(ta_ctx* c);               // a grid of other dims drops source and result.  ta_api_resample.hip
// ta_resample_extract is about to write into `buf` (or, now == NULL, has let go of it): a B / a signal adopted from it by
// ta_resample_as_overlap / _as_signal holds new contents -- its tables are stale -- and is dropped when the buffer moved to `now`
// or changed its item size.  ta_api_overlap.hip, ta_api_signal.hip.
void overlap_on_resampled(ta_ctx* c, const void* buf, const void* now, int itemsize);
void signal_on_resampled(ta_ctx* c, const void* buf, const void* now, int itemsize);
void walls_on_new_labels(ta_ctx* c);                  // new label values in the same volume: the staging buffer is kept.  ta_api_walls.hip

// The two ways the voxels change (ta_api.hip).  volume_replaced: the tail of ta_volume_set / ta_volume_set_device, called once vol,
// itemsize, dims and layout are in place.  volume_labels_changed: new label values written by the library itself (ta_volume_relabel,
// ta_components_relabel): the census and a compacted state end, the extraction and everything keyed by the old labels is stale.
void volume_replaced(ta_ctx* c);
void volume_labels_changed(ta_ctx* c);

// The word ta_volume_rerank leaves on the device shares its place with the max-label passes.  rerank_verdict takes the word wherever
// it was read (nothing to do unless a rerank is unchecked): clears the check, and on an id that is not in the list ends the extraction
// and fails.  settle_rerank reads the word from the device first: for whoever is about to reuse its place.  ta_api_sparse.hip.
int rerank_verdict(ta_ctx* c, uint32_t status);
int settle_rerank(ta_ctx* c);

// The pair -> row hash of the sorted pair list of the settled extraction (c->npairs > 0 pairs), built into `into` on the stream:
// keys u64[cap] | sorted keys u64[P] | rows u32[cap].  Each caller keeps a buffer of its own.  ta_api_signal.hip.
int build_pair_index(ta_ctx* c, DevBuf& into, const uint64_t** hkeys, const uint32_t** hrows, uint32_t* hmask);

// Companions: these touch the companion's own fields only.  The setters check the arguments against the label volume and drain the
// stream (a pass in flight may still read the old companion) before they change anything; a failure later leaves no companion set.
int companion_set_host(ta_ctx* c, Companion& v, const CompanionKind& kind, const void* host_ptr, int itemsize, const int64_t dims[3],
                       const int64_t strides_bytes[3]);
int companion_set_device(ta_ctx* c, Companion& v, const CompanionKind& kind, const void* dev_ptr, int itemsize);
inline bool companion_matches(const ta_ctx* c, const Companion& v) { return std::equal(v.mdims, v.mdims + 3, c->mdims); }   // set for these dims
void companion_on_new_volume(const ta_ctx* c, Companion& v);      // ... or dropped

// the entry checks of a pass over labels + signal: a signal set for this volume, then extraction_preflight
inline int signal_pass_preflight(ta_ctx* c, const char* noun) {
    if (!c->sig.img.p) return fail(TA_EINVAL, "no signal set");
    if (!c->vol || !companion_matches(c, c->sig.img)) return fail(TA_EINVAL, "the signal does not match the label volume");
    return extraction_preflight(c, noun);
}
