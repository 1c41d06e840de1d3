"""Euler numbers without a GPU: the NumPy restatement of tests/topology_reference.py on shapes whose numbers are known and on the
properties the header states, `CellTopology` and `topological_defects` from hand-made columns, and include/tissue_scan_topology.h
against the binding and the library."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import range_tiles as rt
import topology_reference as tr
from tissue_analysis_amd import CellTopology, _capi
from tissue_analysis_amd.cell_topology import topological_defects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference on known shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,want", [(tr.ball, (1, 1)), (tr.shell, (2, 2)), (tr.torus, (0, 0)), (tr.double_torus, (-1, -1))],
                         ids=["ball", "shell", "torus", "double_torus"])
def test_known_shapes(shape, want):
    mask = shape()
    assert mask.any() and not mask[0].any() and not mask[:, 0].any() and not mask[:, :, 0].any()      # (inside its box)
    assert tr.euler_of_mask(mask) == want
    assert tr.euler_of_mask(np.ascontiguousarray(mask.transpose(2, 0, 1))) == want


def test_voxels_that_share_only_an_edge_or_a_corner():
    edge = np.zeros((4, 4, 4), dtype=bool)
    edge[1, 1, 1] = edge[1, 2, 2] = True
    corner = np.zeros((4, 4, 4), dtype=bool)
    corner[1, 1, 1] = corner[2, 2, 2] = True
    assert tr.euler_of_mask(edge) == (2, 1) and tr.euler_of_mask(corner) == (2, 1)
    face = np.zeros((4, 4, 4), dtype=bool)
    face[1, 1, 1] = face[1, 1, 2] = True
    assert tr.euler_of_mask(face) == (1, 1)


def test_a_full_volume_and_a_label_at_the_eight_corners():
    for dims in ((1, 1, 1), (3, 4, 5), (1, 7, 2)):
        c = tr.counts(np.full(dims, 2, dtype=np.uint16), 3)
        assert tr.euler(c, 6).tolist() == [0, 0, 1] and tr.euler(c, 26).tolist() == [0, 0, 1]
        assert int(c["n0"][2]) == int(np.prod(dims)) and int(c["v"][2]) == int(np.prod([d + 1 for d in dims]))
    V = tr.eight_corners()
    c = tr.counts(V, 4)
    assert int(c["n0"][3]) == 8 and tr.euler(c, 6)[3] == 8 and tr.euler(c, 26)[3] == 8
    assert not c["n1"][3].any() and int(c["v"][3]) == 64 and c["e"][3].tolist() == [32, 32, 32]
    # the rest of the volume: a box with its corners cut off is still a ball
    assert tr.euler(c, 6)[0] == 1 and tr.euler(c, 26)[0] == 1


def test_duality_of_the_two_connectivities():
    rng = np.random.default_rng(17)
    for i in range(40):
        dims = rng.integers(1, 7, size=3)
        X = np.zeros(tuple(dims + 2), dtype=bool)
        X[1:-1, 1:-1, 1:-1] = rng.random(tuple(dims)) < rng.uniform(0.2, 0.8)
        chi6, chi26 = tr.euler_of_mask(X)
        n6, n26 = tr.euler_of_mask(~X)
        assert n26 == chi6 + 1 and n6 == chi26 + 1, (i, dims)


def test_every_label_gives_the_numbers_of_its_binary_mask():
    V = rt.block_labels((9, 11, 13), np.uint16, 5, nlabels=6, block=(2, 3, 2))
    V[2:5, 3:6, 4:9] = rt.random_image((3, 3, 5), np.uint8, 6) % 7
    c = tr.counts(V, 7)
    for l in range(7):
        b = tr.counts((V == l).astype(np.uint8), 2)
        for name in tr.COLUMNS:
            assert np.array_equal(c[name][l], b[name][1]), (name, l)
    assert np.array_equal(c["n0"], np.bincount(V.reshape(-1), minlength=7).astype(np.uint64))


def test_exposed_faces_counted_by_brute_force():
    V = rt.random_image((6, 7, 5), np.uint8, 8) % 4
    c = tr.counts(V, 4)
    want = tr.exposed_faces(V, 4)
    assert np.array_equal(6 * c["n0"] - 2 * c["n1"].sum(axis=1), want)
    assert np.array_equal(2 * (tr.faces(c).sum(axis=1) - 3 * c["n0"].astype(np.int64)), want.astype(np.int64))


@pytest.mark.parametrize("box", [(1, 1, 1), (2, 5, 3), (4, 1, 6)])
def test_intrinsic_volumes_of_boxes_with_anisotropic_voxels(box):
    s = (0.5, 2.0, 1.25)
    a, b, c = box
    for at in ((0, 0, 0), (2, 1, 3)):                         # at the corner of the image and inside it
        V = np.zeros((8, 8, 10), dtype=np.uint16)
        V[at[0]:at[0] + a, at[1]:at[1] + b, at[2]:at[2] + c] = 1
        cts = tr.counts(V, 2)
        v1, v2 = tr.intrinsic(cts, s)
        assert v1[1] == pytest.approx(a * s[0] + b * s[1] + c * s[2], rel=1e-15)
        assert v2[1] == pytest.approx(b * c * s[1] * s[2] + a * c * s[0] * s[2] + a * b * s[0] * s[1], rel=1e-15)
        t = CellTopology(None, *[cts[k] for k in tr.COLUMNS], voxelsize=s)
        chi26, V1, V2, vol = t.intrinsic_volumes()
        assert chi26[1] == 1 and V1[1] == v1[1] and V2[1] == v2[1] and vol[1] == pytest.approx(a * b * c * s[0] * s[1] * s[2], rel=1e-15)
        assert t.mean_breadth()[1] == v1[1] / 2 and t.mean_breadth((1, 1, 1))[1] == (a + b + c) / 2


# ---- CellTopology from hand-made columns ------------------------------------------------------------------------------------------
def _topology(V, nrows, **kw):
    c = tr.counts(V, nrows)
    return CellTopology(None, *[c[k] for k in tr.COLUMNS], **kw), c


def test_cell_topology_columns_and_return_types():
    V = np.zeros((6, 9, 24), dtype=np.uint16)
    V[1:5, 1:8, 1:23] = tr.torus(2, 1, (4, 7, 22)) * 2         # (a coarse ring)
    V[0, 0, :5] = 3
    t, c = _topology(V, 4)
    assert len(t) == 4
    for name in tr.COLUMNS:
        col = getattr(t, name)
        assert col.dtype == np.int64 and np.array_equal(col, c[name].astype(np.int64))
    assert t.n1.shape == t.n2.shape == t.e.shape == (4, 3)
    chi = t.euler_number()
    assert chi.dtype == np.int64 and np.array_equal(chi, tr.euler(c, 6)) and np.array_equal(t.euler_number(26), tr.euler(c, 26))
    assert chi[1] == 0 and chi[3] == 1                         # (no voxels: the empty set), a bar
    with pytest.raises(ValueError):
        t.euler_number(18)
    got = t.of_labels([3, 2, 77, 0])
    assert got.dtype == np.int64 and got.tolist() == [1, int(chi[2]), 0, int(chi[0])]
    mb = t.of_labels([3, 77], "mean_breadth")
    assert mb.dtype == np.float64 and mb.tolist() == [(1 + 1 + 5) / 2.0, 0.0]
    assert t.of_labels([3], "half_surface").tolist() == [1 * 1 + 1 * 5 + 1 * 5]
    with pytest.raises(ValueError):
        t.of_labels([1], "genus")
    with pytest.raises(ValueError):
        CellTopology(None, c["n0"], c["n1"][:2], c["n2"], c["n3"], c["v"], c["e"])
    with pytest.raises(ValueError):
        CellTopology(None, *[c[k] for k in tr.COLUMNS], perm=(0, 1, 1))


def test_perm_carries_the_axis_columns_to_array_axes():
    V = np.zeros((5, 7, 9), dtype=np.uint16)
    V[1:3, 1:5, 2:8] = 1                                      # a box of 2 x 4 x 6
    t, _ = _topology(V, 2)
    assert t.faces()[1].tolist() == [3 * 4 * 6, 2 * 5 * 6, 2 * 4 * 7]          # lattice faces the box touches, each once
    perm = (2, 0, 1)                                          # memory axis k is array axis perm[k]
    Vm = np.ascontiguousarray(V.transpose(perm))
    vs = (0.5, 2.0, 1.25)
    p, _ = _topology(Vm, 2, perm=perm, voxelsize=vs)
    q = CellTopology(None, t.n0, t.n1, t.n2, t.n3, t.v, t.e, voxelsize=vs)
    assert np.array_equal(p.faces(), t.faces()) and np.array_equal(p.face_pairs(), t.face_pairs())
    assert np.array_equal(p.euler_number(), t.euler_number()) and np.array_equal(p.euler_number(26), t.euler_number(26))
    for a, b in zip(p.intrinsic_volumes(), q.intrinsic_volumes()):
        assert np.array_equal(a, b)
    assert p.mean_breadth()[1] == (2 * 0.5 + 4 * 2.0 + 6 * 1.25) / 2


def test_topological_defects_from_an_injected_component_table():
    V = np.zeros((9, 25, 49), dtype=np.uint16)
    V[:, :, :41] = tr.double_torus() * 4
    V[3:6, 10:13, 43:46] = 5                                  # a cube in the background ...
    V[4, 11, 44] = 6                                          # ... with a speck inside: a cavity
    V[0, 0, 48] = V[2, 0, 48] = 7                             # two blobs of one label
    t, c = _topology(V, 8)
    blobs = {0: 1, 4: 1, 5: 1, 6: 1, 7: 2}
    components = types.SimpleNamespace(per_label=lambda: dict(blobs))
    found = topological_defects(t, components)
    # (the background has two tunnels, through the handles, and two cavities, the handlebody and the cube: they cancel)
    assert t.euler_number()[[0, 6, 7]].tolist() == [1, 1, 2]
    assert found == {4: {'blobs': 1, 'euler': -1, 'tunnels_minus_cavities': 2},
                     5: {'blobs': 1, 'euler': 2, 'tunnels_minus_cavities': -1}}
    assert topological_defects(t, components, exclude=(0, 4)) == {5: found[5]}
    blobs[7] = 1
    assert topological_defects(t, components)[7] == {'blobs': 1, 'euler': 2, 'tunnels_minus_cavities': -1}
    assert all(type(v) is int for d in found.values() for v in d.values())


# ---- the plan -------------------------------------------------------------------------------------------------------------------
def test_the_plan_covers_one_more_plane_and_row_of_positions():
    assert tr.plan((15, 3, 255), 4)[:4] == (1, 1, 1, 1)
    assert tr.plan((16, 4, 256), 4)[:4] == (1, 2, 2, 4)       # one tile of voxels: the positions beyond it are tiles of their own
    assert tr.plan((17, 5, 257), 4)[:4] == (2, 2, 2, 8)
    assert tr.plan((16, 4, 512), 2)[:4] == (1, 2, 2, 4) and tr.plan((17, 5, 513), 2)[:4] == (2, 2, 2, 8)
    p = tr.plan((257, 1025, 9), 4)
    assert (p.tiles, p.per, p.groups) == (17 * 257, 5, 874) and p.per * (p.groups - 1) + p.tiles_in_last_group == p.tiles
    assert tr.plan((1, 1, 1), 2)[:6] == (1, 1, 1, 1, 1, 1)


def test_spill_bound_of_the_permutation_volume():
    V = rt.permutation_labels(rt.SPILL_DIMS, np.uint16, 1)
    assert tr.plan(V.shape, 2).groups == 4 and tr.label_spill_bound(V) == V.size - tr.LABEL_SLOTS


# ---- header, binding, library ---------------------------------------------------------------------------------------------------
def header():
    return open(os.path.join(ROOT, "include", "tissue_scan_topology.h")).read()


def test_header_and_binding_agree():
    text = header()
    declared = sorted(set(re.findall(r"TA_API\s+int\s+(ta_\w+)\s*\(", text)))
    assert declared == sorted(_capi.TOPOLOGY_SYMBOLS) and len(declared) == 4
    assert not set(_capi.TOPOLOGY_SYMBOLS) & set(_capi.SYMBOLS)
    assert len(re.findall(r"TA_API\s+int\s+ta_\w+_debug\s*\(", text)) == 1
    assert re.search(r"TA_API\s+int\s+ta_topology_debug\s*\(ta_ctx\*\s*ctx,\s*uint32_t\s+out\[4\]\)", text)
    lib = _capi.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.ta_version() == _capi.ABI_VERSION == 5


def test_constants_agree():
    kernel_header = open(os.path.join(ROOT, "tissue_analysis_amd", "csrc", "ta_topology.h")).read()
    assert int(re.search(r"TP_SLOTS\s*=\s*(\d+)", kernel_header).group(1)) == _capi.TOPOLOGY_SLOTS == tr.LABEL_SLOTS
    assert int(re.search(r"TP_MAX_GROUPS\s*=\s*(\d+)", kernel_header).group(1)) == _capi.TOPOLOGY_MAX_GROUPS == tr.MAX_GROUPS
    assert 4 * 52 * tr.LABEL_SLOTS <= 160 * 1024              # four workgroups of 52-byte rows in a CU's LDS


def test_a_null_context_is_refused_without_a_gpu():
    lib = _capi.load()
    assert lib.ta_topology_extract(None) == _capi.TA_EINVAL
    assert b"NULL" in lib.ta_last_error()
    assert lib.ta_topology_get(None, None, None, None, None, None, None) == _capi.TA_EINVAL
    out = (ctypes.c_uint32 * 4)()
    assert lib.ta_topology_debug(None, out) == _capi.TA_EINVAL and list(out) == [0, 0, 0, 0]
    ms = ctypes.c_double(-1.0)
    assert lib.ta_topology_timing(None, ctypes.byref(ms)) == _capi.TA_EINVAL and ms.value == -1.0
