// kernels_components.hip -- connected components of equal label (include/tissue_scan_components.h): a block-based union-find over
// the resident label volume, the statistics of every component, and the row image.
//
// parent[v] is the buffer-linear index of a voxel of v's component, never a larger one than v: a forest whose roots are the
// smallest voxel of every set.  Links only ever go from a root to a smaller index of the set it is united with.
// 1. Local pass.  One workgroup per tile of CC_TILE_PLANES x CC_TILE_ROWS x CC_TILE_COLS voxels.  A lane holds a 16-byte strip of
//    a row (4 uint32 or 8 uint16 labels; rows that are not whole strips take the scalar loads).  The runs of equal labels inside a
//    strip are resolved in registers; the last label of the strip goes to the next lane by __shfl_up, and a run that spans
//    several lanes takes the start of its first strip (one ballot: the lane where the run begins).  Links across rows and planes:
//    union-find on an LDS parent array with LDS atomicMin, one union per pair of overlapping runs.  Then every voxel finds its
//    root in LDS and parent[v] is written as the buffer index of that root: components that meet only through another tile stay
//    apart here.
// 2. Seam pass.  Only the pairs of equal label across tile faces.  Workgroups on different XCDs write the same words of `parent`
//    within the launch and the L2s of the XCDs are not coherent with each other, so EVERY access to `parent` in this kernel is an
//    agent-scope atomic: relaxed loads to walk, atomicMin to link the larger root under the smaller one, again from the returned
//    old value when the linked word was no longer a root.  A stale read is harmless: it names a voxel of the same set that is
//    not smaller than the current parent.  The launch boundary publishes the local pass's plain stores to this kernel and this
//    kernel's links to the next one; nothing waits for another workgroup.
// 3. Flatten and count: first the voxels that the seam pass linked out of their tile name their root (component_hoist_kernel: the
//    former roots of the tiles' sets, few), then parent[v] = root of v (a word only ever changes from an ancestor to the root,
//    and roots do not change in these kernels, so the plain loads may see either); every wave counts its roots.  The counts are
//    scanned, the host
//    allocates one slot per root, and the emit kernel hands the slots out in voxel order: parent[root] = CC_SLOT_FLAG | slot.
// 4. Statistics over the owned voxels: a lane takes four consecutive voxels, the runs of one slot among them by closed forms.
//    Lanes whose four voxels are one run are folded across the wave (segments of neighbouring lanes of one slot) and the
//    segment's first lane issues one set of integer atomics; the other lanes issue theirs per run.  A wave walks 32 such chunks
//    of 256 voxels and keeps what whole chunks of one component add in registers until another component follows.  The minima
//    are looked at before they are sent (a value read too old is only larger: one atomic too many, never one too few).
// 5. Sort keys label << 32 | first, the existing radix sort, and a kernel that writes the rows in that order and the slot -> row
//    table.  6. Row image and relabel: streaming gathers through parent and that table.
// All integers: bit-exact whatever the order.
#include "ta_components.h"

#include <algorithm>

namespace ta {
namespace {

constexpr int CC_TILE = CC_TILE_PLANES * CC_TILE_ROWS * CC_TILE_COLS;
constexpr int CC_THREADS = 256;

#define CC_RELAXED_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define CC_RELAXED_GROUP __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

template <typename E, int VPL>
__device__ __forceinline__ void unpack16(const uint4 q, uint32_t (&out)[VPL]) {
    static_assert(VPL * (int)sizeof(E) == 16, "a strip is 16 bytes");
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < VPL; ++j) out[j] = sizeof(E) == 4 ? w[j] : ((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
}

__device__ __forceinline__ uint64_t lanes_upto(int lane) { return lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// exclusive prefix sum of v across the wave
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t v, int lane) {
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= d) inc += t;
    }
    return inc - v;
}

// ---- 1. local pass --------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t lds_find(uint32_t* par, uint32_t x) {
    uint32_t y;
    while ((y = __hip_atomic_load(par + x, CC_RELAXED_GROUP)) != x) x = y;
    return x;
}

__device__ __forceinline__ void lds_union(uint32_t* par, uint32_t a, uint32_t b) {
    for (;;) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = __hip_atomic_fetch_min(par + a, b, CC_RELAXED_GROUP);
        if (old == a) return;                      // a was a root: linked
        a = old;                                   // it was not: what it pointed to and b are still to be united
    }
}

// the voxels of a strip (nv of them inside the volume) that share their label with the voxel `back` tile indices before them
template <typename E, int VPL>
__device__ __forceinline__ void link_back(uint32_t* par, const E* lab, int base, int back, int nv, const uint32_t (&v)[VPL]) {
    uint32_t u[VPL];
    unpack16<E, VPL>(*reinterpret_cast<const uint4*>(lab + base - back), u);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        // one union per pair of overlapping runs: where either run begins
        const bool fresh = j == 0 || v[j] != v[j - 1] || u[j] != u[j - 1];
        if (j < nv && v[j] == u[j] && fresh) lds_union(par, (uint32_t)(base + j), (uint32_t)(base - back + j));
    }
}

template <typename E, bool VEC>
__global__ __launch_bounds__(CC_THREADS) void component_local_kernel(const ComponentArgs A, int64_t ntc, int64_t ntr) {
    constexpr int VPL = 16 / (int)sizeof(E);
    constexpr int LPR = CC_TILE_COLS / VPL;        // lanes of a row of the tile: 64 or 32
    constexpr int ITER = CC_TILE / VPL / CC_THREADS;
    __shared__ uint32_t par[CC_TILE];
    __shared__ __attribute__((aligned(16))) E lab[CC_TILE];
    const int lane = threadIdx.x & 63;
    const int64_t tile = blockIdx.x;
    const int64_t q0 = (tile / (ntc * ntr)) * CC_TILE_PLANES, r0 = ((tile / ntc) % ntr) * CC_TILE_ROWS, c0 = (tile % ntc) * CC_TILE_COLS;
    const E* vol = (const E*)A.vol;

    // strips: tile index of the strip's first voxel = 16-byte strip number * VPL; row = plane * CC_TILE_ROWS + row in the plane
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int base = (it * CC_THREADS + (int)threadIdx.x) * VPL;
        const int row = base / CC_TILE_COLS, cs = base % CC_TILE_COLS;
        const int64_t q = q0 + row / CC_TILE_ROWS, r = r0 + row % CC_TILE_ROWS, c = c0 + cs;
        int nv = 0;
        if (q < A.n0 && r < A.n1 && c < A.n2) nv = A.n2 - c < VPL ? (int)(A.n2 - c) : VPL;
        uint32_t v[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j) v[j] = 0u;
        if (nv > 0) {
            const E* src = vol + (q * A.n1 + r) * A.n2 + c;
            if (VEC) {
                unpack16<E, VPL>(*reinterpret_cast<const uint4*>(src), v);     // (n2 is a multiple of VPL: nv == VPL)
            } else {
#pragma unroll
                for (int j = 0; j < VPL; ++j)
                    if (j < nv) v[j] = (uint32_t)src[j];
            }
        }
        // the runs of the strip: rs[j] = where the run of voxel j begins
        int rs[VPL];
        rs[0] = 0;
        bool uniform = nv == VPL;
#pragma unroll
        for (int j = 1; j < VPL; ++j) {
            rs[j] = v[j] == v[j - 1] ? rs[j - 1] : j;
            uniform = uniform && v[j] == v[0];
        }
        // the lane before: its last label, and where that label's run begins
        const uint32_t prev_last = (uint32_t)__shfl_up((int)v[VPL - 1], 1);
        const int prev_full = __shfl_up(nv == VPL ? 1 : 0, 1);
        const int prev_uniform = __shfl_up(uniform ? 1 : 0, 1);
        const uint32_t prev_start = (uint32_t)__shfl_up(base + rs[VPL - 1], 1);
        const bool link = (lane % LPR) != 0 && nv > 0 && prev_full && prev_last == v[0];
        // a run that fills whole lanes begins where the first of them says: the nearest lane at or before this one that does not
        // hand the question on (lane 0 of a row never does)
        const bool settles = !(link && prev_uniform);
        const uint32_t mine = link ? prev_start : (uint32_t)base;
        const uint64_t m = __ballot(settles) & lanes_upto(lane);
        const uint32_t head = (uint32_t)__shfl((int)mine, 63 - __clzll((long long)m));
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            par[base + j] = j >= nv ? (uint32_t)(base + j) : (rs[j] == 0 ? head : (uint32_t)(base + rs[j]));
            lab[base + j] = (E)v[j];
        }
    }
    __syncthreads();

    // rows and planes: the strip one row and one plane back, inside the tile
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int base = (it * CC_THREADS + (int)threadIdx.x) * VPL;
        const int row = base / CC_TILE_COLS, cs = base % CC_TILE_COLS;
        const int64_t q = q0 + row / CC_TILE_ROWS, r = r0 + row % CC_TILE_ROWS, c = c0 + cs;
        int nv = 0;
        if (q < A.n0 && r < A.n1 && c < A.n2) nv = A.n2 - c < VPL ? (int)(A.n2 - c) : VPL;
        if (nv > 0) {
            uint32_t v[VPL];
            unpack16<E, VPL>(*reinterpret_cast<const uint4*>(lab + base), v);
            if (row % CC_TILE_ROWS != 0) link_back<E, VPL>(par, lab, base, CC_TILE_COLS, nv, v);
            if (row / CC_TILE_ROWS != 0) link_back<E, VPL>(par, lab, base, CC_TILE_ROWS * CC_TILE_COLS, nv, v);
        }
    }
    __syncthreads();

    // flatten (reads only) and write the buffer index of the root
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int base = (it * CC_THREADS + (int)threadIdx.x) * VPL;
        const int row = base / CC_TILE_COLS, cs = base % CC_TILE_COLS;
        const int64_t q = q0 + row / CC_TILE_ROWS, r = r0 + row % CC_TILE_ROWS, c = c0 + cs;
        int nv = 0;
        if (q < A.n0 && r < A.n1 && c < A.n2) nv = A.n2 - c < VPL ? (int)(A.n2 - c) : VPL;
        if (nv > 0) {
            uint32_t v[VPL], g[VPL];
            unpack16<E, VPL>(*reinterpret_cast<const uint4*>(lab + base), v);
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                if (j > 0 && v[j] == v[j - 1]) { g[j] = g[j - 1]; continue; }      // (the same run: the same root)
                uint32_t x = (uint32_t)(base + j), y;
                while ((y = par[x]) != x) x = y;
                const int xr = (int)x / CC_TILE_COLS;
                g[j] = (uint32_t)(((q0 + xr / CC_TILE_ROWS) * A.n1 + r0 + xr % CC_TILE_ROWS) * A.n2 + c0 + (int)x % CC_TILE_COLS);
            }
            uint32_t* dst = A.parent + (q * A.n1 + r) * A.n2 + c;
            if (VEC) {
#pragma unroll
                for (int j = 0; j < VPL; j += 4) *reinterpret_cast<uint4*>(dst + j) = make_uint4(g[j], g[j + 1], g[j + 2], g[j + 3]);
            } else {
#pragma unroll
                for (int j = 0; j < VPL; ++j)
                    if (j < nv) dst[j] = g[j];
            }
        }
    }
}

// ---- 2. seam pass ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t seam_find(uint32_t* parent, uint32_t x) {
    uint32_t y;
    while ((y = __hip_atomic_load(parent + x, CC_RELAXED_AGENT)) != x) x = y;
    return x;
}

__device__ __forceinline__ void seam_union(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = seam_find(parent, a);
        b = seam_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = __hip_atomic_fetch_min(parent + a, b, CC_RELAXED_AGENT);
        if (old == a) return;
        a = old;
    }
}

// voxel x and voxel y (wanted: they share a label across a tile face): unite their sets.  Neighbouring lanes mostly hold the same
// two roots: a lane whose pair is that of the lane before it leaves the link to that lane.  Called by whole waves.
__device__ __forceinline__ void seam_link(uint32_t* parent, bool wanted, uint32_t x, uint32_t y, int lane) {
    uint32_t a = 0u, b = 0u;
    if (wanted) {
        a = seam_find(parent, x);
        b = seam_find(parent, y);
        wanted = a != b;
    }
    const uint32_t pa = (uint32_t)__shfl_up((int)a, 1), pb = (uint32_t)__shfl_up((int)b, 1);
    const int pw = __shfl_up(wanted ? 1 : 0, 1);
    if (wanted && !(lane > 0 && pw && pa == a && pb == b)) seam_union(parent, a, b);
}

template <typename E>
__global__ __launch_bounds__(CC_THREADS) void component_seam_kernel(const ComponentArgs A) {
    const E* vol = (const E*)A.vol;
    const int lane = threadIdx.x & 63;
    const int64_t rows = A.n0 * A.n1, plane = A.n1 * A.n2;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t q = row / A.n1, r = row % A.n1, base = row * A.n2;
        const bool face0 = q > 0 && q % CC_TILE_PLANES == 0, face1 = r > 0 && r % CC_TILE_ROWS == 0;
        if (face0 || face1) {                      // (uniform over the workgroup, and so is the loop)
            for (int64_t cb = 0; cb < A.n2; cb += CC_THREADS) {
                const int64_t c = cb + threadIdx.x;
                const bool live = c < A.n2;
                const int64_t v = base + (live ? c : 0);
                const E l = vol[v];
                // the pair one column back, inside the same tiles: where it holds this label on both sides too, the local pass
                // has joined it to this pair on either side of the face, and its union serves both
                const int64_t back = !live || c % CC_TILE_COLS == 0 ? 0 : 1;
                const bool begins = back == 0 || vol[v - 1] != l;
                const int64_t d0 = face0 ? plane : 0, d1 = face1 ? A.n2 : 0;
                seam_link(A.parent, live && face0 && vol[v - d0] == l && (begins || vol[v - d0 - back] != l), (uint32_t)v, (uint32_t)(v - plane), lane);
                seam_link(A.parent, live && face1 && vol[v - d1] == l && (begins || vol[v - d1 - back] != l), (uint32_t)v, (uint32_t)(v - A.n2), lane);
            }
        }
        for (int64_t c = ((int64_t)threadIdx.x + 1) * CC_TILE_COLS; c < A.n2; c += (int64_t)CC_THREADS * CC_TILE_COLS)
            if (vol[base + c] == vol[base + c - 1]) seam_union(A.parent, (uint32_t)(base + c), (uint32_t)(base + c - 1));
    }
}

// ---- 3. flatten, count, emit ------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t root_from(const uint32_t* parent, uint32_t x) {
    uint32_t y;
    while ((y = parent[x]) != x) x = y;
    return x;
}

// Before the flatten: a voxel whose word names a voxel of ANOTHER tile was the root of its tile's set until the seam pass linked
// it; every voxel of that set is about to walk through it.  Such voxels (few) walk to their root first and name it, so that the
// walks of the flatten are two steps long instead of one per tile the component crosses.  A voxel wrongly taken or left (a root
// linked inside its own tile) only costs or saves a walk: any word that names an ancestor is valid.
__global__ __launch_bounds__(CC_THREADS) void component_hoist_kernel(uint32_t* parent, uint64_t nvox, uint32_t n1, uint32_t n2) {
    const uint64_t v0 = ((uint64_t)blockIdx.x * CC_THREADS + threadIdx.x) * 4;
    if (v0 >= nvox) return;
    const uint32_t row0 = (uint32_t)v0 / n2;
    uint32_t c = (uint32_t)v0 - row0 * n2, q = row0 / n1, r = row0 - (row0 / n1) * n1;      // of voxel v0 + j
    for (int j = 0; j < 4 && v0 + j < nvox; ++j) {
        const uint32_t v = (uint32_t)(v0 + j), p = parent[v];
        if (p != v) {
            const uint32_t prow = p / n2, pc = p - prow * n2, pq = prow / n1, pr = prow - pq * n1;
            if (pc / CC_TILE_COLS != c / CC_TILE_COLS || pr / CC_TILE_ROWS != r / CC_TILE_ROWS || pq / CC_TILE_PLANES != q / CC_TILE_PLANES)
                parent[v] = root_from(parent, p);
        }
        if (++c == n2) { c = 0u; if (++r == n1) { r = 0u; ++q; } }
    }
}

__global__ __launch_bounds__(CC_THREADS) void component_flatten_kernel(uint32_t* parent, uint64_t nvox, uint32_t* wave_counts) {
    const uint64_t t = (uint64_t)blockIdx.x * CC_THREADS + threadIdx.x, v0 = t * 4;
    uint32_t cnt = 0u;
    if (v0 + 3 < nvox) {
        const uint4 p = *reinterpret_cast<const uint4*>(parent + v0);
        const uint32_t in[4] = {p.x, p.y, p.z, p.w};
        uint32_t out[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            out[j] = j > 0 && in[j] == in[j - 1] ? out[j - 1] : root_from(parent, in[j]);
            cnt += out[j] == (uint32_t)(v0 + j) ? 1u : 0u;
        }
        *reinterpret_cast<uint4*>(parent + v0) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
        for (uint64_t v = v0; v < nvox; ++v) {
            const uint32_t root = root_from(parent, parent[v]);
            parent[v] = root;
            cnt += root == (uint32_t)v ? 1u : 0u;
        }
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) wave_counts[t >> 6] = cnt;
}

__global__ __launch_bounds__(CC_THREADS) void component_emit_kernel(uint32_t* parent, uint64_t nvox, const uint64_t* wave_offsets,
                                                                    uint32_t* root_of_slot) {
    const int lane = threadIdx.x & 63;
    const uint64_t t = (uint64_t)blockIdx.x * CC_THREADS + threadIdx.x, v0 = t * 4;
    uint32_t in[4] = {0u, 0u, 0u, 0u};
    bool root[4] = {false, false, false, false};
    if (v0 + 3 < nvox) {
        const uint4 p = *reinterpret_cast<const uint4*>(parent + v0);
        in[0] = p.x; in[1] = p.y; in[2] = p.z; in[3] = p.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (v0 + j < nvox) in[j] = parent[v0 + j];
    }
    uint32_t mine = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        root[j] = v0 + j < nvox && in[j] == (uint32_t)(v0 + j);
        mine += root[j] ? 1u : 0u;
    }
    uint64_t at = wave_offsets[t >> 6] + wave_exclusive(mine, lane);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (root[j]) {
            parent[v0 + j] = CC_SLOT_FLAG | (uint32_t)at;
            root_of_slot[at] = (uint32_t)(v0 + j);
            ++at;
        }
}

// the slot of a voxel from its word p of `parent`: a root carries its own, any other voxel names its root
__device__ __forceinline__ uint32_t slot_from(const uint32_t* parent, uint32_t p) {
    return (p & CC_SLOT_FLAG) ? (p & ~CC_SLOT_FLAG) : (parent[p] & ~CC_SLOT_FLAG);
}

// ---- 4. statistics --------------------------------------------------------------------------------------------------------------

struct Fold {
    uint32_t n;
    uint64_t s[3];
    int32_t lo[3], hi[3];
    uint64_t key;
};

__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d), hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ void stats_send(const ComponentStats& T, uint32_t slot, const Fold& f) {
    flush_add(T.n + slot, (unsigned long long)f.n);
    int32_t* box = T.box + 6ull * slot;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (f.s[k]) flush_add(T.sum1 + 3ull * slot + k, (unsigned long long)f.s[k]);
        if (f.lo[k] < box[k]) flush_min(box + k, f.lo[k]);
        if (-f.hi[k] < box[3 + k]) flush_min(box + 3 + k, -f.hi[k]);
    }
    if (f.key < T.first[slot]) (void)__hip_atomic_fetch_min(T.first + slot, (unsigned long long)f.key, CC_RELAXED_AGENT);
}

// a run of len voxels (q, r, c .. c + len - 1)
__device__ __forceinline__ Fold run_fold(const ComponentGeometry& G, uint32_t q, uint32_t r, uint32_t c, uint32_t len) {
    Fold f;
    f.n = len;
    f.s[0] = (uint64_t)len * q; f.s[1] = (uint64_t)len * r; f.s[2] = (uint64_t)len * c + (uint64_t)len * (len - 1) / 2;
    f.lo[0] = f.hi[0] = (int32_t)q; f.lo[1] = f.hi[1] = (int32_t)r;
    f.lo[2] = (int32_t)c; f.hi[2] = (int32_t)(c + len - 1);
    f.key = q * G.key_stride[0] + r * G.key_stride[1] + c * G.key_stride[2];      // (every stride is positive: the run's smallest)
    return f;
}

// a wave walks CC_STATS_CHUNKS chunks of 256 consecutive voxels; what a chunk of ONE component adds stays in lane 0's registers
// for as long as the chunks that follow belong to the same component
constexpr int CC_STATS_CHUNKS = 32;

__device__ __forceinline__ void fold_add(Fold& f, const Fold& o) {
    f.n += o.n;
    f.key = o.key < f.key ? o.key : f.key;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f.s[k] += o.s[k];
        f.lo[k] = o.lo[k] < f.lo[k] ? o.lo[k] : f.lo[k];
        f.hi[k] = o.hi[k] > f.hi[k] ? o.hi[k] : f.hi[k];
    }
}

__global__ __launch_bounds__(CC_THREADS) void component_stats_kernel(const uint32_t* parent, const ComponentGeometry G, const ComponentStats T) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (CC_THREADS / 64) + (threadIdx.x >> 6);
    Fold kept = {};                                // lane 0: the chunks of one component so far, of slot kept_slot
    uint32_t kept_slot = CC_NO_ROW;
    for (int chunk = 0; chunk < CC_STATS_CHUNKS; ++chunk) {
        const uint64_t v0 = ((wave * CC_STATS_CHUNKS + chunk) * 64 + lane) * 4;
        if ((wave * CC_STATS_CHUNKS + chunk) * 256 >= G.nvox) break;      // (wave-uniform)
        uint32_t p[4] = {0u, 0u, 0u, 0u};
        int have = 0;                              // voxels of the lane inside the buffer
        if (v0 + 3 < G.nvox) {
            const uint4 w = *reinterpret_cast<const uint4*>(parent + v0);
            p[0] = w.x; p[1] = w.y; p[2] = w.z; p[3] = w.w;
            have = 4;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v0 + j < G.nvox) { p[j] = parent[v0 + j]; have = j + 1; }
        }
        uint32_t q = 0u, r = 0u, c = 0u;           // of voxel v0 (nvox <= 2^31: 32-bit divisions)
        if (have) {
            const uint32_t row = (uint32_t)v0 / G.n2;
            c = (uint32_t)v0 - row * G.n2;
            q = row / G.n1;
            r = row - q * G.n1;
        }
        uint32_t slot[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            slot[j] = j >= have ? CC_NO_ROW : (j > 0 && p[j] == p[j - 1] ? slot[j - 1] : slot_from(parent, p[j]));
        // four owned voxels of one row and one component: the lane's part goes through the wave
        const bool whole = have == 4 && v0 >= G.own_begin && c + 3 < G.n2 && slot[1] == slot[0] && slot[2] == slot[0] && slot[3] == slot[0];
        if (!whole) {
            uint32_t qq = q, rr = r, cc = c;       // of voxel j
            uint32_t cur = 0u, len = 0u, sq = 0u, sr = 0u, sc = 0u;
            bool owned = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool live = j < have;
                if (live && len > 0u && slot[j] == cur && cc != 0u) {
                    ++len;
                } else {
                    if (len > 0u && owned) stats_send(T, cur, run_fold(G, sq, sr, sc, len));
                    len = 0u;
                    if (live) { cur = slot[j]; len = 1u; sq = qq; sr = rr; sc = cc; owned = v0 + j >= G.own_begin; }
                }
                if (++cc == G.n2) { cc = 0u; if (++rr == G.n1) { rr = 0u; ++qq; } }
            }
            if (len > 0u && owned) stats_send(T, cur, run_fold(G, sq, sr, sc, len));
        }
        // segments: neighbouring whole lanes of one slot; every other lane is a segment of its own that adds nothing
        const int prev_whole = __shfl_up(whole ? 1 : 0, 1);
        const uint32_t prev_slot = (uint32_t)__shfl_up((int)slot[0], 1);
        const bool head = !(whole && lane > 0 && prev_whole && prev_slot == slot[0]);
        const uint64_t heads = __ballot(head);
        if (__ballot(whole) == 0ull) continue;     // (wave-uniform)
        const uint32_t seg = (uint32_t)__popcll(heads & lanes_upto(lane));
        Fold f = run_fold(G, q, r, c, 4u);
        if (!whole) {
            f.n = 0u; f.key = ~0ull;
#pragma unroll
            for (int k = 0; k < 3; ++k) { f.s[k] = 0ull; f.lo[k] = 0x7fffffff; f.hi[k] = -0x7fffffff; }
        }
        // segments ascend along the wave: after the step of distance d a lane holds its segment's lanes in [lane, lane + 2d)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            Fold o;
            const uint32_t oseg = (uint32_t)__shfl_down((int)seg, d);
            o.n = (uint32_t)__shfl_down((int)f.n, d);
            o.key = shfl_down_u64(f.key, d);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                o.s[k] = shfl_down_u64(f.s[k], d);
                o.lo[k] = __shfl_down(f.lo[k], d);
                o.hi[k] = __shfl_down(f.hi[k], d);
            }
            if (lane + d < 64 && oseg == seg) fold_add(f, o);
        }
        if (heads == 1ull && __ballot(whole) == ~0ull) {
            // the whole chunk is one segment (lane 0 holds it): kept back, and sent when another component follows
            if (lane == 0) {
                if (kept_slot == slot[0]) {
                    fold_add(kept, f);
                } else {
                    if (kept_slot != CC_NO_ROW) stats_send(T, kept_slot, kept);
                    kept = f;
                    kept_slot = slot[0];
                }
            }
        } else if (whole && head) {
            stats_send(T, slot[0], f);
        }
    }
    if (lane == 0 && kept_slot != CC_NO_ROW) stats_send(T, kept_slot, kept);
}

// ---- 5. keys and rows -----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t label_at(const void* vol, int itemsize, uint64_t v) {
    return itemsize == 2 ? (uint32_t)((const uint16_t*)vol)[v] : ((const uint32_t*)vol)[v];
}

__global__ __launch_bounds__(256) void component_keys_kernel(const void* vol, int itemsize, const uint32_t* root_of_slot, const ComponentStats T,
                                                             uint64_t nslots, uint64_t* keys_out, uint32_t* index_out, unsigned long long* nonempty) {
    // (the loop is uniform over the wave: one add per wave to the one word, of the wave's slots with owned voxels)
    for (uint64_t at = (uint64_t)blockIdx.x * blockDim.x; at < nslots; at += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = at + threadIdx.x;
        const bool rowed = i < nslots && T.n[i] != 0ull;
        if (i < nslots) {
            keys_out[i] = rowed ? ((uint64_t)label_at(vol, itemsize, root_of_slot[i]) << 32) | (uint32_t)T.first[i] : ~0ull;
            index_out[i] = (uint32_t)i;
        }
        const uint64_t m = __ballot(rowed);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(nonempty, (unsigned long long)__popcll(m));
    }
}

__global__ __launch_bounds__(256) void component_rows_kernel(const void* vol, int itemsize, const uint32_t* root_of_slot, const ComponentStats T,
                                                             const uint32_t* order, uint64_t nslots, const unsigned long long* nonempty,
                                                             uint32_t* row_of_slot, const ComponentRows R) {
    const uint64_t nrows = *nonempty;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t slot = order[i];
        if (i >= nrows) { row_of_slot[slot] = CC_NO_ROW; continue; }
        row_of_slot[slot] = (uint32_t)i;
        const int64_t n = (int64_t)T.n[slot];
        R.label[i] = label_at(vol, itemsize, root_of_slot[slot]);
        R.n[i] = (unsigned long long)n;
        const int64_t key = (int64_t)T.first[slot];
        const int64_t x[3] = {key / (R.dims[1] * R.dims[2]), (key / R.dims[2]) % R.dims[1], key % R.dims[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) R.first[3 * i + a] = (int32_t)(x[a] + (R.axis[0] == a ? R.origin0 : 0));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int64_t shift = k == 0 ? R.origin0 : 0;
            R.bbox[6 * i + R.axis[k]] = (int32_t)(T.box[6ull * slot + k] + shift);
            R.bbox[6 * i + 3 + R.axis[k]] = (int32_t)(-(int64_t)T.box[6ull * slot + 3 + k] + 1 + shift);
            R.sum1[3 * i + R.axis[k]] = (unsigned long long)((int64_t)T.sum1[3ull * slot + k] + n * shift);
        }
    }
}

// ---- 6. row image and relabel ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void component_image_kernel(const uint32_t* parent, const uint32_t* row_of_slot, uint64_t first, uint64_t count,
                                                              uint32_t* rows_out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x)
        rows_out[i] = row_of_slot[slot_from(parent, parent[first + i])];
}

template <typename E>
__global__ __launch_bounds__(256) void component_relabel_kernel(const uint32_t* parent, const uint32_t* row_of_slot, uint64_t nvox,
                                                                const uint32_t* new_label, E* vol) {
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvox; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t row = row_of_slot[slot_from(parent, parent[v])];
        if (row != CC_NO_ROW) vol[v] = (E)new_label[row];
    }
}

unsigned grid_for(uint64_t n) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), CC_STREAM_MAX_GROUPS); }

}  // namespace

uint64_t component_tiles(const ComponentArgs& a) {
    return (uint64_t)((a.n0 + CC_TILE_PLANES - 1) / CC_TILE_PLANES) * (uint64_t)((a.n1 + CC_TILE_ROWS - 1) / CC_TILE_ROWS) *
           (uint64_t)((a.n2 + CC_TILE_COLS - 1) / CC_TILE_COLS);
}

void launch_component_local(hipStream_t s, const ComponentArgs& a, int itemsize) {
    const uint64_t tiles = component_tiles(a);
    if (!tiles) return;
    const int64_t ntc = (a.n2 + CC_TILE_COLS - 1) / CC_TILE_COLS, ntr = (a.n1 + CC_TILE_ROWS - 1) / CC_TILE_ROWS;
    const bool vec = a.n2 % (16 / itemsize) == 0 && ((uintptr_t)a.vol % 16) == 0;
    const dim3 grid((unsigned)tiles), block(CC_THREADS);
    if (itemsize == 2) {
        if (vec) hipLaunchKernelGGL((component_local_kernel<uint16_t, true>), grid, block, 0, s, a, ntc, ntr);
        else hipLaunchKernelGGL((component_local_kernel<uint16_t, false>), grid, block, 0, s, a, ntc, ntr);
    } else {
        if (vec) hipLaunchKernelGGL((component_local_kernel<uint32_t, true>), grid, block, 0, s, a, ntc, ntr);
        else hipLaunchKernelGGL((component_local_kernel<uint32_t, false>), grid, block, 0, s, a, ntc, ntr);
    }
}

uint32_t launch_component_seams(hipStream_t s, const ComponentArgs& a, int itemsize) {
    const uint64_t rows = (uint64_t)a.n0 * (uint64_t)a.n1;
    if (!rows) return 0u;
    const dim3 grid((unsigned)std::min<uint64_t>(rows, CC_SEAM_MAX_GROUPS)), block(CC_THREADS);
    if (itemsize == 2) hipLaunchKernelGGL(component_seam_kernel<uint16_t>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(component_seam_kernel<uint32_t>, grid, block, 0, s, a);
    return grid.x;
}

void launch_component_flatten(hipStream_t s, uint32_t* parent, uint64_t nvox, int64_t n1, int64_t n2, uint32_t* wave_counts) {
    if (!nvox) return;
    hipLaunchKernelGGL(component_hoist_kernel, dim3((unsigned)(component_waves(nvox) / 4)), dim3(CC_THREADS), 0, s, parent, nvox, (uint32_t)n1,
                       (uint32_t)n2);
    hipLaunchKernelGGL(component_flatten_kernel, dim3((unsigned)(component_waves(nvox) / 4)), dim3(CC_THREADS), 0, s, parent, nvox, wave_counts);
}

void launch_component_emit(hipStream_t s, uint32_t* parent, uint64_t nvox, const uint64_t* wave_offsets, uint32_t* root_of_slot) {
    if (!nvox) return;
    hipLaunchKernelGGL(component_emit_kernel, dim3((unsigned)(component_waves(nvox) / 4)), dim3(CC_THREADS), 0, s, parent, nvox, wave_offsets,
                       root_of_slot);
}

void launch_component_stats(hipStream_t s, const uint32_t* parent, const ComponentGeometry& g, const ComponentStats& t) {
    if (!g.nvox) return;
    const uint64_t per_group = (uint64_t)CC_STATS_CHUNKS * 256 * (CC_THREADS / 64);
    hipLaunchKernelGGL(component_stats_kernel, dim3((unsigned)((g.nvox + per_group - 1) / per_group)), dim3(CC_THREADS), 0, s, parent, g, t);
}

uint32_t launch_component_keys(hipStream_t s, const void* vol, int itemsize, const uint32_t* root_of_slot, const ComponentStats& t, uint64_t nslots,
                               uint64_t* keys_out, uint32_t* index_out, unsigned long long* nonempty) {
    if (!nslots) return 0u;
    hipLaunchKernelGGL(component_keys_kernel, dim3(grid_for(nslots)), dim3(256), 0, s, vol, itemsize, root_of_slot, t, nslots, keys_out, index_out,
                       nonempty);
    return grid_for(nslots);
}

void launch_component_rows(hipStream_t s, const void* vol, int itemsize, const uint32_t* root_of_slot, const ComponentStats& t,
                           const uint32_t* order, uint64_t nslots, const unsigned long long* nonempty, uint32_t* row_of_slot,
                           const ComponentRows& rows) {
    if (!nslots) return;
    hipLaunchKernelGGL(component_rows_kernel, dim3(grid_for(nslots)), dim3(256), 0, s, vol, itemsize, root_of_slot, t, order, nslots, nonempty,
                       row_of_slot, rows);
}

uint32_t launch_component_image(hipStream_t s, const uint32_t* parent, const uint32_t* row_of_slot, uint64_t first, uint64_t count, uint32_t* rows_out) {
    if (!count) return 0u;
    hipLaunchKernelGGL(component_image_kernel, dim3(grid_for(count)), dim3(256), 0, s, parent, row_of_slot, first, count, rows_out);
    return grid_for(count);
}

uint32_t launch_component_relabel(hipStream_t s, const uint32_t* parent, const uint32_t* row_of_slot, uint64_t nvox, const uint32_t* new_label,
                                  void* vol, int itemsize) {
    if (!nvox) return 0u;
    if (itemsize == 2) hipLaunchKernelGGL(component_relabel_kernel<uint16_t>, dim3(grid_for(nvox)), dim3(256), 0, s, parent, row_of_slot, nvox, new_label, (uint16_t*)vol);
    else hipLaunchKernelGGL(component_relabel_kernel<uint32_t>, dim3(grid_for(nvox)), dim3(256), 0, s, parent, row_of_slot, nvox, new_label, (uint32_t*)vol);
    return grid_for(nvox);
}

}  // namespace ta
