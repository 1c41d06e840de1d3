"""Cell meshes without a GPU: the NumPy restatement of tests/mesh_reference.py on known answers and exact invariants (enclosed
volume, closed surfaces, faces per wall against the C oracle), the C ABI of include/tissue_scan_mesh.h, and the PLY writer."""
import ctypes
import os
import re

import numpy as np

import mesh_reference as ref
from tissue_analysis_amd import CellMeshes, _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_mesh_symbols():
    text = open(os.path.join(ROOT, "include", "tissue_scan_mesh.h")).read()
    return sorted(set(re.findall(r"TA_API\s+(?:const\s+char\s*\*|int)\s+(ta_\w+)\s*\(", text)))


def _volumes():
    rng = np.random.default_rng(20261016)
    for shape, nlab, dt in (((6, 7, 9), 5, np.uint16), ((3, 11, 4), 30, np.uint32), ((9, 1, 13), 3, np.uint16),
                            ((5, 5, 1), 4, np.uint32)):
        yield rng.integers(0, nlab, size=shape).astype(dt)


def _cells(r):
    for i, l in enumerate(r["labels"].tolist()):
        t0, t1 = int(r["triangle_offsets"][i]), int(r["triangle_offsets"][i + 1])
        v0, v1 = int(r["vertex_offsets"][i]), int(r["vertex_offsets"][i + 1])
        yield l, slice(v0, v1), slice(t0, t1)


def test_single_voxel_and_two_voxel_cell():
    V = np.zeros((3, 3, 3), dtype=np.uint16)
    V[1, 1, 1] = 1
    r = ref.mesh(V, labels=[1])
    assert len(r["points"]) == 8 and len(r["triangles"]) == 12
    V = np.zeros((4, 3, 3), dtype=np.uint16)
    V[1:3, 1, 1] = 1
    r = ref.mesh(V, labels=[1])
    assert len(r["points"]) == 12 and len(r["triangles"]) == 20
    assert (r["triangle_neighbor"] == 0).all()


def test_cavity_faces_point_into_the_cavity():
    V = np.full((5, 5, 5), 0, dtype=np.uint16)
    V[1:4, 1:4, 1:4] = 2
    V[2, 2, 2] = 3                                      # the cavity
    r = ref.mesh(V, labels=[2])
    tri = r["triangles"].astype(np.int64)
    into = r["triangle_neighbor"] == 3
    assert into.sum() == 12
    K = r["corners"]
    a, b, c = K[tri[into, 0]], K[tri[into, 1]], K[tri[into, 2]]
    normal = np.cross(b - a, c - a)
    centre = (a + b + c) / 3.0
    # the cavity voxel (2, 2, 2) spans corners 2 .. 3: its centre is at corner coordinate 2.5
    assert (np.einsum("ij,ij->i", normal, np.array([2.5, 2.5, 2.5]) - centre) > 0).all()
    assert ref.six_volume(K, tri) == 6 * 26


def test_enclosed_volume_is_the_voxel_count():
    for V in _volumes():
        r = ref.mesh(V)
        counts = np.bincount(V.reshape(-1).astype(np.int64))
        for l, vs, ts in _cells(r):
            assert ref.six_volume(r["corners"], r["triangles"][ts]) == 6 * counts[l]
            assert (r["triangle_cell"][ts] == l).all()


def test_every_directed_edge_is_matched():
    for V in _volumes():
        r = ref.mesh(V)
        for l, vs, ts in _cells(r):
            t = r["triangles"][ts].astype(np.int64)
            e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
            fwd = sorted(map(tuple, e.tolist()))
            back = sorted(map(tuple, e[:, ::-1].tolist()))
            assert fwd == back, l
            assert t.min() >= vs.start and t.max() < vs.stop


def test_faces_per_wall_equal_the_c_oracle():
    from oracle import onepass_c
    for V in _volumes():
        r = ref.mesh(V)
        o = onepass_c.extract(V)
        cell, nb = r["triangle_cell"][0::2], r["triangle_neighbor"][0::2]
        axis = r["face_direction"] // 2
        inner = nb >= 0
        got = {}
        for c, n, a in zip(cell[inner].tolist(), nb[inner].tolist(), axis[inner].tolist()):
            got.setdefault((min(c, n), max(c, n)), np.zeros(3, dtype=np.int64))[a] += 1
        want = dict(((int(lo), int(hi)), 2 * np.asarray(f, dtype=np.int64))
                    for lo, hi, f in zip(o["pair_lo"], o["pair_hi"], o["pair_faces"]))
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), k


def test_sub_factor_meshes_the_strided_image():
    V = next(_volumes())
    for s in (2, 3):
        a, b = ref.mesh(V, sub_factor=s, voxelsize=(0.5, 1.0, 2.0)), ref.mesh(V[::s, ::s, ::s])
        assert np.array_equal(a["triangles"], b["triangles"]) and np.array_equal(a["corners"], b["corners"])
        np.testing.assert_array_equal(a["points"], (b["corners"] - 0.5) * (np.array([0.5, 1.0, 2.0]) * s))


def test_mesh_header_and_binding_agree():
    assert declared_mesh_symbols() == sorted(_capi.MESH_SYMBOLS)
    assert not set(_capi.MESH_SYMBOLS) & (set(_capi.SYMBOLS) | set(_capi.SIGNAL_SYMBOLS))


def test_library_exports_the_mesh_symbols_and_they_reject_a_null_context():
    lib = _capi.load()
    buf = (ctypes.c_uint64 * 64)()
    u = ctypes.c_uint64(0)
    dbl = ctypes.c_double(0)
    calls = {
        "ta_mesh_extract": (None, 1, None),
        "ta_mesh_size": (None, ctypes.byref(u), ctypes.byref(u), ctypes.byref(u)),
        "ta_mesh_get": (None, buf, buf, buf, buf, buf, buf, buf),
        "ta_mesh_timing": (None, ctypes.byref(dbl)),
    }
    assert sorted(calls) == sorted(_capi.MESH_SYMBOLS)
    for name in declared_mesh_symbols():
        assert hasattr(lib, name), name
        assert getattr(lib, name)(*calls[name]) == _capi.TA_EINVAL, name
        err = lib.ta_last_error()
        assert b"NULL" in err or b"ctx" in err, (name, err)


def _read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in head if h.startswith("element face")][0].split()[-1])
    pts = np.frombuffer(data, dtype="<f8", count=3 * nv, offset=end).reshape(nv, 3)
    face = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("v", "<u4", (3,)), ("label", "<i4"), ("neighbor", "<i4")]),
                         count=nf, offset=end + 24 * nv)
    assert (face["n"] == 3).all() and len(data) == end + 24 * nv + 21 * nf
    return pts, face["v"], face["label"], face["neighbor"]


def _as_meshes(r):
    return CellMeshes(r["labels"], r["points"], r["triangles"], r["triangle_cell"], r["triangle_neighbor"],
                      r["vertex_offsets"], r["triangle_offsets"])


def test_ply_round_trip(tmp_path):
    V = next(_volumes())
    m = _as_meshes(ref.mesh(V))
    p = str(tmp_path / "all.ply")
    m.to_ply(p)
    pts, tri, lab, nb = _read_ply(p)
    assert np.array_equal(pts, m.points) and np.array_equal(tri, m.triangles)
    assert np.array_equal(lab, m.triangle_cell) and np.array_equal(nb, m.triangle_neighbor)
    one = int(m.labels[1])
    m.to_ply(p, labels=[one])
    pts, tri, lab, nb = _read_ply(p)
    q, t = m[one]
    assert np.array_equal(pts, q) and np.array_equal(tri, t) and (lab == one).all()


def test_mapping_wall_and_composed():
    V = next(_volumes())
    r = ref.mesh(V)
    m = _as_meshes(r)
    assert list(m) == r["labels"].tolist() and len(m) == len(r["labels"])
    l1 = int(m.labels[1])
    pts, tri = m[l1]
    assert tri.max() < len(pts)
    l2 = int(m.triangle_neighbor[m.triangle_cell == l1][0])
    _, w = m.wall(l1, l2)
    sel = (m.triangle_cell == l1) & (m.triangle_neighbor == l2)
    assert len(w) == sel.sum() > 0
    p2, t2, c2 = m.composed(0.5)
    centre = pts.mean(axis=0)
    i = int(np.flatnonzero(m.labels == l1)[0])
    v0, v1 = int(m.vertex_offsets[i]), int(m.vertex_offsets[i + 1])
    np.testing.assert_allclose(p2[v0:v1], centre + 0.5 * (pts - centre))
    assert np.array_equal(m.composed(1.0)[0], m.points)
