"""Signal statistics on the MI355X (include/tissue_scan_signal.h, csrc/kernels_signal.hip) against the NumPy restatement of
tests/signal_reference.py: integers bit-exact, float results to 1e-12 relative."""
import os

import numpy as np
import pytest

import signal_reference as ref
from tissue_analysis_amd import DICT, LIST, NPLIST, SignalStats, SpatialImageAnalysis, _capi, synth
from tissue_analysis_amd.extraction import ResidentVolume
from tissue_analysis_amd.graph_from_image import graph_from_image

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _signal(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(dtype).max, size=shape, endpoint=True).astype(dtype)


def check_stats(st, V, S):
    """st: SignalStats of signal S over label image V (any layout)."""
    x = st.extraction
    V3 = V if V.ndim == 3 else V[:, :, None]
    if x.ids is None:
        rows = None
        nrows = x.nrows
    else:
        rows = np.searchsorted(x.ids, V3.astype(np.int64))
        nrows = x.ids.size
    r = ref.labels(V, S, nrows, rows)
    assert np.array_equal(st.n, r["n"])
    assert np.array_equal(st.n, x.count)
    assert np.array_equal(st.sum, r["sum"])
    assert np.array_equal(st.sumsq[:, 0], r["sumsq"]) and not st.sumsq[:, 1].any()
    present = r["n"] > 0
    assert np.array_equal(st._min[present], r["min"][present]) and np.array_equal(st._max[present], r["max"][present])
    assert (st._min[~present] == 0xFFFFFFFF).all() and (st._max[~present] == 0).all()
    m = ref.moments(r)
    for k in ("mean", "std", "min", "max"):
        np.testing.assert_allclose(getattr(st, k), m[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
    w = ref.walls(V, S)
    assert np.array_equal(st.lo, w["lo"]) and np.array_equal(st.hi, w["hi"])
    assert np.array_equal(x.pair_faces.sum(axis=1), w["faces"].sum(axis=1))
    assert np.array_equal(st.side_lo, w["side_lo"]) and np.array_equal(st.side_hi, w["side_hi"])
    f = w["faces"].sum(axis=1).astype(np.float64)
    np.testing.assert_allclose(st.wall_mean, (w["side_lo"] + w["side_hi"]).astype(np.float64) / (2 * f), rtol=1e-12)


def _run(V, S, **kw):
    rv = ResidentVolume(V)
    try:
        rv.extract(**kw)
        st = rv.signal(S)
    finally:
        rv.close()
    assert isinstance(st, SignalStats)
    return st


def test_adversarial_golden_volumes():
    z = np.load(os.path.join(GOLD, "adversarial_small.npz"))
    names = sorted(set(k.split("__")[0] for k in z.files))
    for i, name in enumerate(names):
        V = z[name + "__volume"]
        for sdt in (np.uint8, np.uint16):
            S = _signal(V.shape, sdt, i)
            check_stats(_run(V, S), V, S)


def test_config1_label_and_signal_types_and_layouts():
    c = synth.CONFIGS["C1"]
    V16 = synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], np.uint16)
    for ldt in (np.uint16, np.uint32):
        V = V16.astype(ldt)
        for sdt in (np.uint8, np.uint16):
            S = _signal(V.shape, sdt, 7)
            check_stats(_run(V, S), V, S)
    # F-ordered labels and signal; then a signal whose layout differs from the labels' (copied into theirs)
    VF, SF = np.asfortranarray(V16), np.asfortranarray(_signal(V16.shape, np.uint16, 8))
    check_stats(_run(VF, SF), VF, SF)
    SC = np.ascontiguousarray(SF)
    check_stats(_run(VF, SC), VF, SC)
    check_stats(_run(V16, SF), V16, SF)
    # rows that are not a multiple of the strip width (the scalar-load path)
    Vo = np.ascontiguousarray(V16[:, :, :61])
    So = _signal(Vo.shape, np.uint8, 9)
    check_stats(_run(Vo, So), Vo, So)


def test_two_dimensional_image():
    V = synth.voronoi_labels((1, 200, 150), 40, 3, np.uint16)[0]
    S = _signal(V.shape, np.uint16, 4)
    check_stats(_run(V, S), V, S)
    sia = SpatialImageAnalysis(V, background=None, return_type=DICT)
    got = sia.cell_signal(S)
    r = ref.moments(ref.labels(V, S, int(V.max()) + 1))
    assert all(abs(got[l] - r["mean"][l]) <= 1e-12 * abs(r["mean"][l]) for l in got)


def test_sparse_ids_compacted_context():
    rng = np.random.default_rng(5)
    ids = np.array([0, 7, 70000, 2**31 + 5, 2**32 - 2, 2**32 - 1], dtype=np.uint32)
    V = ids[rng.integers(0, ids.size, size=(12, 9, 33))]
    S = _signal(V.shape, np.uint16, 6)
    st = _run(V, S, sparse=True)
    assert st.ids is not None and np.array_equal(st.ids, ids.astype(np.int64))
    check_stats(st, V, S)


def test_two_slab_contexts_with_a_halo_sum_to_the_whole():
    import torch
    c = synth.CONFIGS["C1"]
    V = synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], np.uint16)
    S = _signal(V.shape, np.uint8, 11)
    L = int(V.max())
    cut = 37
    parts = []
    for lo, hi, halo in ((0, cut, False), (cut - 1, V.shape[0], True)):
        tv = torch.from_numpy(V[lo:hi].astype(np.int16)).cuda()
        ts = torch.from_numpy(S[lo:hi].copy()).cuda()
        torch.cuda.synchronize()
        ctx = _capi.Context(0)
        ctx.set_volume_device(tv.data_ptr(), 2, tv.shape, a0_origin=lo + (1 if halo else 0), has_low_halo=halo, keep=tv)
        ctx.set_signal_device(ts.data_ptr(), 1, keep=ts)
        ctx.extract(_capi.F_ALL, L)
        ctx.signal_extract()
        n, s, q, mn, mx = ctx.signal_labels()
        lo_, hi_, _ = ctx.adjacency()
        slo, shi = ctx.signal_walls()
        parts.append((n, s, q, dict(zip(((lo_.astype(np.uint64) << np.uint64(32)) | hi_).tolist(), zip(slo.tolist(), shi.tolist())))))
        ctx.close()
    r, w = ref.labels(V, S, L + 1), ref.walls(V, S)
    assert np.array_equal(parts[0][0] + parts[1][0], r["n"])
    assert np.array_equal(parts[0][1] + parts[1][1], r["sum"])
    assert np.array_equal(parts[0][2][:, 0] + parts[1][2][:, 0], r["sumsq"])
    tot = {}
    for p in parts:
        for k, (a, b) in p[3].items():
            t = tot.setdefault(k, [0, 0])
            t[0] += a
            t[1] += b
    assert sorted(tot) == w["keys"].tolist()
    assert [tot[k] for k in w["keys"].tolist()] == [[a, b] for a, b in zip(w["side_lo"].tolist(), w["side_hi"].tolist())]


def test_sumsq_carry_beyond_64_bits():
    """One label, more than 2^32 voxels, signal 65535 everywhere: sum of squares n * 65535^2 > 2^64."""
    import torch
    dims = (1040, 2048, 2048)                              # 4.36e9 voxels: 8.7 GB of labels + 8.7 GB of signal
    n = dims[0] * dims[1] * dims[2]
    assert n > 2**32
    vol = torch.full(dims, 3, dtype=torch.int16, device="cuda")
    sig = torch.full(dims, -1, dtype=torch.int16, device="cuda")      # 0xFFFF
    torch.cuda.synchronize()
    ctx = _capi.Context(0)
    try:
        ctx.set_volume_device(vol.data_ptr(), 2, dims, keep=vol)
        ctx.set_signal_device(sig.data_ptr(), 2, keep=sig)
        ctx.extract(_capi.F_VOLUME, 3)
        ctx.signal_extract(_capi.SIG_LABELS)
        cnt, s, q, mn, mx = ctx.signal_labels()
    finally:
        ctx.close()
        del vol, sig
        torch.cuda.empty_cache()
    want = n * 65535 * 65535
    assert int(cnt[3]) == n and int(s[3]) == n * 65535
    assert (int(q[3, 1]) << 64) | int(q[3, 0]) == want and want >= 2**64
    assert int(mn[3]) == 65535 and int(mx[3]) == 65535
    assert int(mn[0]) == 0xFFFFFFFF and int(cnt[0]) == 0


def test_invalidation_and_argument_errors():
    V = synth.voronoi_labels((20, 30, 40), 12, 1, np.uint16)
    S = _signal(V.shape, np.uint8, 2)
    rv = ResidentVolume(V)
    try:
        rv.extract()
        rv.ctx.set_signal(S)
        rv.ctx.signal_extract()
        rv.ctx.signal_labels()
        rv.ctx.relabel(np.arange(int(V.max()) + 1, dtype=np.uint32))
        for get in (rv.ctx.signal_labels, rv.ctx.signal_walls):
            with pytest.raises(_capi.TissueScanError) as e:
                get()
            assert e.value.code == _capi.TA_EINVAL
        with pytest.raises(TypeError, match="uint8 or uint16"):
            rv.signal(S.astype(np.float32))
        with pytest.raises(ValueError):
            rv.signal(S[:, :, :-1])
        with pytest.raises(_capi.TissueScanError):           # a new extraction invalidates, even of the same volume
            rv.extract()
            rv.ctx.signal_labels()
        check_stats(rv.signal(S), V, S)                      # and a new pass answers again
    finally:
        rv.close()


def test_analysis_methods_and_graph():
    c = synth.CONFIGS["C1"]
    V = synth.voronoi_labels(c["dims"], c["n_cells"], c["seed"], np.uint16)
    S = _signal(V.shape, np.uint16, 12)
    r = ref.labels(V, S, int(V.max()) + 1)
    m = ref.moments(r)
    w = ref.walls(V, S)
    for rt in (DICT, LIST, NPLIST):
        sia = SpatialImageAnalysis(V, ignoredlabels=0, return_type=rt, background=1)
        labels = sia.labels()
        for stat in ("mean", "std", "min", "max", "sum"):
            got = sia.cell_signal(S, statistic=stat)
            want = r["sum"][labels] if stat == "sum" else m[stat][labels]
            vals = np.array([got[l] for l in labels]) if rt == DICT else np.asarray(got)
            if stat == "sum":
                assert np.array_equal(vals.astype(np.uint64), want)
            else:
                np.testing.assert_allclose(vals, want, rtol=1e-12)
        with pytest.raises(ValueError):
            sia.cell_signal(S, statistic="median")
        areas = sia.wall_areas(real=False)
        keys = [tuple(k) for k in np.asarray(areas[0]).tolist()] if rt == NPLIST else list(areas)
        means, sides = sia.wall_signal(S), sia.wall_signal(S, statistic="sides")
        assert list(means) == keys and list(sides) == keys
        pos = np.searchsorted(w["keys"], [(a << 32) | b for a, b in keys])
        f = w["faces"].sum(axis=1)[pos].astype(np.float64)
        np.testing.assert_allclose([means[k] for k in keys], (w["side_lo"][pos] + w["side_hi"][pos]) / (2 * f), rtol=1e-12)
        np.testing.assert_allclose([sides[k][0] for k in keys], w["side_lo"][pos] / f, rtol=1e-12)
        np.testing.assert_allclose([sides[k][1] for k in keys], w["side_hi"][pos] / f, rtol=1e-12)
    assert sia._resident().uploads == 1
    sia = SpatialImageAnalysis(V, ignoredlabels=0, return_type=DICT, background=1)
    g = graph_from_image(sia, background=1, spatio_temporal_properties=["volume", "mean_signal", "wall_signal"], signal=S,
                         ignore_cells_at_stack_margins=False)
    ms, valid = g.vertex_column("mean_signal")
    cell = sia.cell_signal(S)
    for vid, v, ok in zip(g.vertex_ids.tolist(), ms.tolist(), valid.tolist()):
        if ok:
            assert v == cell[vid]
    ws, wvalid = g.edge_column("wall_signal")
    walls = sia.wall_signal(S)
    assert wvalid.all()
    for a, b, v in zip(g.edge_sources.tolist(), g.edge_targets.tolist(), ws.tolist()):
        assert v == walls[(min(a, b), max(a, b))]
    plain = graph_from_image(V, background=1, spatio_temporal_properties=["volume", "mean_signal"])
    assert "mean_signal" not in plain.vertex_property_names()


def test_full_size_c4_uint16_signal():
    import torch
    from tissue_analysis_amd import device as dev
    c = synth.CONFIGS["C4"]
    dims, dtype = c["dims"], np.dtype(c["dtype"])
    ctx = dev.torch_context(0)
    vol, L = dev.synth_slab(ctx, dims, dtype, c["n_cells"], c["seed"])
    S = _signal(dims, np.uint16, 13)
    sig = torch.from_numpy(S.view(np.int16)).cuda()
    torch.cuda.synchronize()
    try:
        ctx.set_volume_device(vol.data_ptr(), dtype.itemsize, vol.shape, keep=vol)
        ctx.set_signal_device(sig.data_ptr(), 2, keep=sig)
        ctx.extract(_capi.F_ALL, L)
        ctx.signal_extract()
        n, s, q, mn, mx = ctx.signal_labels()
        lo, hi, faces = ctx.adjacency()
        slo, shi = ctx.signal_walls()
        count = ctx.labels()[0]
    finally:
        ctx.close()
    V = vol.cpu().numpy().view(dtype)
    del vol, sig
    torch.cuda.empty_cache()
    r = ref.labels(V, S, L + 1)
    assert np.array_equal(n, count) and np.array_equal(n, r["n"]) and np.array_equal(s, r["sum"])
    assert np.array_equal(q[:, 0], r["sumsq"]) and not q[:, 1].any()
    p = r["n"] > 0
    assert np.array_equal(mn[p], r["min"][p]) and np.array_equal(mx[p], r["max"][p])
    w = ref.walls(V, S)
    assert np.array_equal(lo, w["lo"]) and np.array_equal(hi, w["hi"]) and np.array_equal(faces.sum(axis=1), w["faces"].sum(axis=1))
    assert np.array_equal(slo, w["side_lo"]) and np.array_equal(shi, w["side_hi"])
