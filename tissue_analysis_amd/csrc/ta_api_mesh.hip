// ta_api_mesh.hip -- the C ABI of include/tissue_scan_mesh.h: the triangle surface mesh of every requested cell (kernels_mesh.hip).
#include "../../include/tissue_scan_mesh.h"
#include "ta_ctx.h"
#include "ta_mesh.h"

namespace {

const char* const NO_MESH = "no mesh of the current extraction (run ta_mesh_extract)";

bool mesh_current(const ta_ctx* c) { return pass_current(c, c->mesh.seq); }

// MeshState::small for R rows and wf / wc waves of the face / corner kernels: flags u32[4] | wanted u8[R] (from byte 16) | the
// count/scan block of the faces | of the corners
struct MeshSmall {
    static constexpr uint64_t wanted = 16;
    ScanBlock faces, corners;
    MeshSmall(uint64_t R, uint64_t wf, uint64_t wc) : faces(wf, align16(wanted + R)), corners(wc, faces.end) {}
};
// ... of MeshState::work for F faces and V vertex records
struct MeshWork {
    uint64_t frec = 0, fnb, corner;
    SortLayout sort;                             // (one workspace for both sorts: the faces', then the vertex records')
    MeshWork(uint64_t F, uint64_t V)
        : fnb(align16(8 * F)), corner(fnb + align16(4 * F)), sort(F > V ? F : V, 4, corner + align16(8 * V)) {}
};
// the parts of MeshState::out; bounds: vbeg .. fend, the four columns the host reads (and the pass clears) as one
struct MeshOut {
    Part vcorner, vbeg, vend, fbeg, fend, tri, tcell, tnb, bounds;
    uint64_t bytes = 0;
    constexpr MeshOut(uint64_t R, uint64_t F, uint64_t V) {
        PartCursor at;
        vcorner = at.take(8 * V); vbeg = at.take(8 * R, 16); vend = at.take(8 * R); fbeg = at.take(8 * R); fend = at.take(8 * R);
        bounds = {vbeg.at, at.end() - vbeg.at};
        tri = at.take(24 * F, 16); tcell = at.take(8 * F, 16); tnb = at.take(8 * F, 16);
        bytes = at.end(16);
    }
};
static_assert(MeshOut(3, 2, 5).vbeg.at == 48 && MeshOut(3, 2, 5).fend.at == 120 && MeshOut(3, 2, 5).bounds.bytes == 96 && MeshOut(3, 2, 5).tri.at == 144 &&
              MeshOut(3, 2, 5).tcell.at == 192 && MeshOut(3, 2, 5).tnb.at == 208 && MeshOut(3, 2, 5).bytes == 224,
              "corners u64[V] | vbeg, vend, fbeg, fend u64[R] | triangles u32[2F][3] | cell u32[2F] | neighbour u32[2F], the groups from multiples of 16");

// drain the stream, look at the flags of the emit / resolve kernels, and read the cells and their CSR offsets back once
int mesh_finish(ta_ctx* c) {
    uint32_t flags[ta::MESH_NFLAGS] = {0, 0, 0, 0};
    TA_HIP(hipMemcpyAsync(flags, c->mesh.small.p, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    if (flags[ta::MESH_FLAG_RANGE] || flags[ta::MESH_FLAG_MISS] || flags[ta::MESH_FLAG_OVERRUN])
        return fail(TA_ERANGE, "the mesh pass found the volume changed since ta_extract (flags %u %u %u)", flags[0], flags[1], flags[2]);
    if (c->mesh.host_ready) return TA_OK;
    const uint64_t R = c->mesh.rows;
    std::vector<uint64_t> t;
    c->mesh.cells.clear(); c->mesh.voff.clear(); c->mesh.toff.clear();
    // (room for every row now: no push_back below allocates)
    int rc = host_alloc([&] { t.resize(4 * R); c->mesh.cells.reserve(R); c->mesh.voff.reserve(R + 1); c->mesh.toff.reserve(R + 1); });
    if (rc != TA_OK || (rc = read_columns(c, c->mesh.out.p, {{t.data(), MeshOut(R, c->mesh.faces, c->mesh.verts).bounds}})) != TA_OK) return rc;
    const uint64_t *vbeg = t.data(), *vend = vbeg + R, *fbeg = vend + R, *fend = fbeg + R;
    for (uint64_t r = 0; r < R; ++r) {
        if (vend[r] <= vbeg[r]) continue;
        if (fend[r] <= fbeg[r]) return fail(TA_ERANGE, "mesh: row %llu has vertices and no faces", (unsigned long long)r);
        c->mesh.cells.push_back((uint32_t)r);
        c->mesh.voff.push_back(vbeg[r]);
        c->mesh.toff.push_back(2 * fbeg[r]);
    }
    c->mesh.voff.push_back(c->mesh.verts);
    c->mesh.toff.push_back(2 * c->mesh.faces);
    c->mesh.host_ready = true;
    return TA_OK;
}

}  // namespace

extern "C" {

TA_API int ta_mesh_extract(ta_ctx* c, int sub_factor, const uint8_t* wanted_rows) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (sub_factor < 1) return fail(TA_EINVAL, "sub_factor must be >= 1, not %d", sub_factor);
    if (!c->vol) return fail(TA_EINVAL, "no volume set");
    if (c->first_owned) return fail(TA_EINVAL, "cell meshes are not available on a slab that carries a halo plane");
    int rc = extraction_preflight(c, "mesh pass");
    if (rc != TA_OK) return rc;
    c->mesh.seq = 0;
    c->mesh.host_ready = false;
    const uint64_t R = (uint64_t)c->max_label + 1;
    ta::MeshArgs a;
    a.vol = sweep_vol(c);
    a.n0 = c->mdims[0]; a.n1 = c->mdims[1]; a.n2 = c->mdims[2];
    a.s = sub_factor;
    a.m0 = (a.n0 + a.s - 1) / a.s; a.m1 = (a.n1 + a.s - 1) / a.s; a.m2 = (a.n2 + a.s - 1) / a.s;
    for (int k = 0; k < 3; ++k) a.inv[c->perm[k]] = k;
    a.rows = (uint32_t)R;
    const uint64_t nvox = (uint64_t)a.m0 * a.m1 * a.m2, ncorner = (uint64_t)(a.m0 + 1) * (a.m1 + 1) * (a.m2 + 1);
    const uint64_t wf = ta::mesh_waves(nvox), wc = ta::mesh_waves(ncorner);
    const MeshSmall S(R, wf, wc);
    if ((rc = c->mesh.small.reserve(S.corners.end)) != TA_OK) return rc;
    char* sm = (char*)c->mesh.small.p;
    a.flags = (uint32_t*)sm;
    a.wanted = (const uint8_t*)(sm + S.wanted);
    if ((rc = ensure_events(c->mesh.ev)) != TA_OK) return rc;
    TA_HIP(hipMemsetAsync(sm, 0, 16, c->stream));
    if (wanted_rows) TA_HIP(hipMemcpyAsync(sm + S.wanted, wanted_rows, R, hipMemcpyHostToDevice, c->stream));
    else TA_HIP(hipMemsetAsync(sm + S.wanted, 1, R, c->stream));
    // count -> scan: the totals are all the host needs before it sizes the output
    TA_HIP(hipEventRecord(c->mesh.ev[0], c->stream));
    ta::launch_mesh_face_count(c->stream, a, c->itemsize, S.faces.counts(sm));
    ta::launch_mesh_corner_count(c->stream, a, c->itemsize, S.corners.counts(sm));
    S.faces.scan(c->stream, sm);
    S.corners.scan(c->stream, sm);
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->mesh.ev[1], c->stream));
    uint64_t F = 0, V = 0;
    uint32_t flags[ta::MESH_NFLAGS] = {0, 0, 0, 0};
    TA_HIP(S.faces.read_total(c->stream, sm, &F));
    TA_HIP(S.corners.read_total(c->stream, sm, &V));
    TA_HIP(hipMemcpyAsync(flags, sm, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
    TA_HIP(hipStreamSynchronize(c->stream));
    if (flags[ta::MESH_FLAG_RANGE]) return fail(TA_ERANGE, "the mesh pass met a label above max_label=%u (the volume changed since ta_extract)", c->max_label);
    if (V > 0xFFFFFFFFull) return fail(TA_ERANGE, "the meshes have %llu vertices: more than 2^32 - 1", (unsigned long long)V);
    if (F > 0xFFFFFFFFull) return fail(TA_ERANGE, "the meshes have %llu faces: more than 2^32 - 1", (unsigned long long)F);
    const MeshWork Wk(F, V);
    const MeshOut O(R, F, V);
    if ((rc = c->mesh.work.reserve(Wk.sort.end)) != TA_OK) return rc;
    if ((rc = c->mesh.out.reserve(O.bytes)) != TA_OK) return rc;
    char* w = (char*)c->mesh.work.p;
    char* o = (char*)c->mesh.out.p;
    uint64_t* frec = (uint64_t*)(w + Wk.frec);
    uint32_t* fnb = (uint32_t*)(w + Wk.fnb);
    uint64_t* corner = (uint64_t*)(w + Wk.corner);
    SortView<uint32_t> vs(Wk.sort, w), fs(Wk.sort, w);      // (the vertex records', then the faces': both written into pair 0)
    uint64_t* vcorner = (uint64_t*)(o + O.vcorner.at);
    uint64_t *vbeg = (uint64_t*)(o + O.vbeg.at), *vend = (uint64_t*)(o + O.vend.at);
    uint64_t *fbeg = (uint64_t*)(o + O.fbeg.at), *fend = (uint64_t*)(o + O.fend.at);
    const int key_bits = c->max_label ? 32 - __builtin_clz(c->max_label) : 1;
    // emit -> group by cell -> resolve
    TA_HIP(hipEventRecord(c->mesh.ev[2], c->stream));
    TA_HIP(hipMemsetAsync(o + O.bounds.at, 0, O.bounds.bytes, c->stream));
    ta::launch_mesh_corner_emit(c->stream, a, c->itemsize, S.corners.offsets(sm), V, corner, vs.keys(), vs.idx());
    TA_HIP(vs.sort(c->stream, V, key_bits));
    ta::launch_mesh_bounds(c->stream, vs.keys(), V, vbeg, vend);
    ta::launch_mesh_gather(c->stream, corner, vs.idx(), V, vcorner);
    ta::launch_mesh_face_emit(c->stream, a, c->itemsize, S.faces.offsets(sm), F, frec, fnb, fs.keys(), fs.idx());
    TA_HIP(fs.sort(c->stream, F, key_bits));
    ta::launch_mesh_bounds(c->stream, fs.keys(), F, fbeg, fend);
    ta::launch_mesh_resolve(c->stream, a, fs.keys(), fs.idx(), frec, fnb, F, vcorner, vbeg, vend, (uint32_t*)(o + O.tri.at),
                            (uint32_t*)(o + O.tcell.at), (uint32_t*)(o + O.tnb.at));
    TA_HIP(hipGetLastError());
    TA_HIP(hipEventRecord(c->mesh.ev[3], c->stream));
    c->mesh.faces = F;
    c->mesh.verts = V;
    c->mesh.rows = (uint32_t)R;
    c->mesh.m[0] = a.m0; c->mesh.m[1] = a.m1; c->mesh.m[2] = a.m2;
    c->mesh.seq = c->extract_seq;
    return TA_OK;
}

TA_API int ta_mesh_size(ta_ctx* c, uint64_t* n_cells, uint64_t* n_vertices, uint64_t* n_triangles) {
    int rc = results_ready(c, mesh_current, NO_MESH);
    if (rc != TA_OK || (rc = mesh_finish(c)) != TA_OK) return rc;
    if (n_cells) *n_cells = (uint64_t)c->mesh.cells.size();
    if (n_vertices) *n_vertices = c->mesh.verts;
    if (n_triangles) *n_triangles = 2 * c->mesh.faces;
    return TA_OK;
}

TA_API int ta_mesh_get(ta_ctx* c, uint32_t* cells, uint64_t* vertex_offsets, uint64_t* triangle_offsets, uint64_t* corners,
                       uint32_t* triangles, uint32_t* triangle_cell, uint32_t* triangle_neighbor) {
    int rc = results_ready(c, mesh_current, NO_MESH);
    if (rc != TA_OK || (rc = mesh_finish(c)) != TA_OK) return rc;
    const uint64_t F = c->mesh.faces, V = c->mesh.verts;
    const MeshOut O(c->mesh.rows, F, V);
    if (cells && !c->mesh.cells.empty()) std::memcpy(cells, c->mesh.cells.data(), 4 * c->mesh.cells.size());
    if (vertex_offsets) std::memcpy(vertex_offsets, c->mesh.voff.data(), 8 * c->mesh.voff.size());
    if (triangle_offsets) std::memcpy(triangle_offsets, c->mesh.toff.data(), 8 * c->mesh.toff.size());
    const bool c_order = c->perm[0] == 0 && c->perm[1] == 1 && c->perm[2] == 2;
    // (another layout: the corners, converted to array-axis indices, then each cell's re-sorted: ord, and where each went: newpos)
    std::vector<uint64_t> k;
    std::vector<uint32_t> ord, newpos;
    if (!c_order && V && (rc = host_alloc([&] { k.resize(V); ord.resize(V); newpos.resize(V); })) != TA_OK) return rc;
    if ((rc = read_columns(c, c->mesh.out.p, {{k.empty() ? (void*)corners : k.data(), O.vcorner}, {triangles, O.tri}, {triangle_cell, O.tcell},
                                               {triangle_neighbor, O.tnb}})) != TA_OK) return rc;
    if (!c_order && V) {
        // the device sorted each cell's corners by their index in MEMORY order: convert them to C-order indices of the array
        // axes and sort each cell's vertices by those (a 2-D image, stored (n0, n1, 1), is such a layout too)
        int64_t g[3], ga[3];
        for (int a = 0; a < 3; ++a) { g[a] = c->mesh.m[a] + 1; ga[c->perm[a]] = g[a]; }
        for (uint64_t i = 0; i < V; ++i) {
            const uint64_t x = k[i];
            const int64_t k2 = (int64_t)(x % (uint64_t)g[2]), r = (int64_t)(x / (uint64_t)g[2]);
            int64_t ka[3];
            ka[c->perm[0]] = r / g[1]; ka[c->perm[1]] = r % g[1]; ka[c->perm[2]] = k2;
            k[i] = (uint64_t)((ka[0] * ga[1] + ka[1]) * ga[2] + ka[2]);
        }
        for (size_t ci = 0; ci + 1 < c->mesh.voff.size(); ++ci) {
            const uint64_t v0 = c->mesh.voff[ci], v1 = c->mesh.voff[ci + 1];
            for (uint64_t i = v0; i < v1; ++i) ord[i] = (uint32_t)i;
            std::sort(ord.begin() + v0, ord.begin() + v1, [&](uint32_t x, uint32_t y) { return k[x] < k[y]; });
            for (uint64_t i = v0; i < v1; ++i) newpos[ord[i]] = (uint32_t)i;
        }
        if (corners) for (uint64_t i = 0; i < V; ++i) corners[i] = k[ord[i]];
        if (triangles) for (uint64_t i = 0; i < 6 * F; ++i) triangles[i] = newpos[triangles[i]];
    }
    return TA_OK;
}

TA_API int ta_mesh_timing(ta_ctx* c, double* ms) {
    if (!c) return fail(TA_EINVAL, "ctx is NULL");
    if (!ms) return fail(TA_EINVAL, "NULL argument");
    if (c->mesh.seq == 0 || !c->mesh.ev[3]) return fail(TA_EINVAL, "no mesh pass has been run");
    hipEvent_t* ev = c->mesh.ev;
    const int rc = use_device(c);
    if (rc != TA_OK) return rc;
    TA_HIP(summed_ms(ev[3], {{ev[0], ev[1]}, {ev[2], ev[3]}}, ms));
    return TA_OK;
}

}  // extern "C"
