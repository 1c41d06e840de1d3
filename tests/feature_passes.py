"""What test_gpu_tile_ranges.py and test_gpu_feature_table_spills.py share: a context over a label volume (uploaded, or adopted
from a torch tensor with or without a low halo plane), and the comparison of the signal, overlap and wall-geometry passes with
tests/signal_reference.py, tests/overlap_reference.py and tests/wall_geometry_reference.py -- every number an exact integer --
and of the launch plan the device reports with tests/range_tiles.py."""
import numpy as np

import overlap_reference
import range_tiles as rt
import signal_reference
import wall_geometry_reference
from tissue_analysis_amd import _capi

A0_ORIGIN = 40                          # global coordinate of the first owned plane of the slabs with a halo


def code(call, *args):
    try:
        call(*args)
    except _capi.TissueScanError as e:
        return e.code
    return _capi.TA_OK


def tensor(a):
    """A CUDA tensor with the bytes of the unsigned array `a` (torch has no unsigned 16 / 32-bit types)."""
    import torch
    signed = {1: np.uint8, 2: np.int16, 4: np.int32}[a.dtype.itemsize]
    t = torch.from_numpy(np.ascontiguousarray(a).view(signed).copy()).cuda()
    torch.cuda.synchronize()
    return t


def poke(t, index, value):
    """Write the unsigned `value` into voxel `index` of the tensor made by tensor(), and wait for it."""
    import torch
    bits = 8 * t.element_size()
    v = int(value)
    t[index] = v - (1 << bits) if t.element_size() > 1 and v >= 1 << (bits - 1) else v
    torch.cuda.synchronize()


class Pass(object):
    """A context over V.  adopted: V lives in a torch tensor (self.t) the test may edit; first_owned = 1 implies it."""

    def __init__(self, V, first_owned=0, adopted=False):
        self.V, self.first_owned = V, int(first_owned)
        self.origin = A0_ORIGIN if first_owned else 0
        self.ctx = _capi.Context(0)
        self.t = None
        if adopted or first_owned:
            self.t = tensor(V)
            self.ctx.set_volume_device(self.t.data_ptr(), V.dtype.itemsize, V.shape, a0_origin=self.origin, has_low_halo=bool(first_owned),
                                       keep=self.t)
        else:
            self.ctx.set_volume(V)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    def extract(self, max_label=None, features=_capi.F_ALL):
        self.max_label = int(self.V.max()) if max_label is None else int(max_label)
        self.ctx.extract(features, self.max_label)
        self.ctx.synchronize()

    def set_signal(self, S):
        if self.t is None:
            self.ctx.set_signal(S)
        else:
            ts = tensor(S)
            self.ctx.set_signal_device(ts.data_ptr(), S.dtype.itemsize, keep=ts)

    def set_overlap(self, B):
        if self.t is None:
            self.ctx.set_overlap(B)
        else:
            tb = tensor(B)
            self.ctx.set_overlap_device(tb.data_ptr(), B.dtype.itemsize, keep=tb)

    def plan(self, which):
        return rt.plan(self.V.shape, self.first_owned, self.V.dtype.itemsize, which)

    # -- each check runs the pass and returns the device's diagnostics
    def check_plan(self, debug, which):
        p = self.plan(which)
        assert (debug["tiles_per_group"], debug["groups"]) == (p.per, p.groups), (debug, p)

    def check_signal(self, S, what=_capi.SIG_LABELS | _capi.SIG_WALLS, V=None):
        """V: what the volume holds now, when that is not what the context was made with."""
        V = self.V if V is None else V
        ctx = self.ctx
        ctx.signal_extract(what)
        debug = ctx.signal_debug()
        self.check_plan(debug, "signal")
        if what & _capi.SIG_LABELS:
            r = signal_reference.labels(V, S, self.max_label + 1, first_owned=self.first_owned)
            n, s, q, mn, mx = ctx.signal_labels()
            assert np.array_equal(n, r["n"]) and int(n.sum()) == V[self.first_owned:].size
            assert np.array_equal(s, r["sum"])
            assert np.array_equal(q[:, 0], r["sumsq"]) and not q[:, 1].any()
            assert np.array_equal(mn, r["min"]) and np.array_equal(mx, r["max"])       # (absent rows: UINT32_MAX and 0 on both sides)
        else:
            assert code(ctx.signal_labels) == _capi.TA_EINVAL
            assert debug["label_spills"] == 0
        if what & _capi.SIG_WALLS:
            w = signal_reference.walls(V, S, first_owned=self.first_owned)
            lo, hi, faces = ctx.adjacency()
            assert np.array_equal(lo, w["lo"]) and np.array_equal(hi, w["hi"])
            assert np.array_equal(faces.sum(axis=1), w["faces"].sum(axis=1))
            slo, shi = ctx.signal_walls()
            assert np.array_equal(slo, w["side_lo"]) and np.array_equal(shi, w["side_hi"])
        else:
            assert code(ctx.signal_walls) == _capi.TA_EINVAL
            assert debug["pair_spills"] == 0
        return debug

    def check_overlap(self, B, V=None):
        V = self.V if V is None else V
        ctx = self.ctx
        ctx.overlap_extract()
        a, b, n = ctx.overlap_get()
        want = overlap_reference.table(V, B, first_owned=self.first_owned)
        assert np.array_equal(a.astype(np.int64), want[0]) and np.array_equal(b.astype(np.int64), want[1])
        assert np.array_equal(n, want[2]) and int(n.sum()) == V[self.first_owned:].size
        debug = ctx.overlap_debug()
        self.check_plan(debug, "overlap")
        assert debug["passes"] == ctx.overlap_timing_compaction()[1]
        return debug

    def check_wallgeo(self, V=None):
        V = self.V if V is None else V
        ctx = self.ctx
        ctx.wallgeo_extract()
        want = wall_geometry_reference.rows(V, first_owned=self.first_owned, a0_origin=self.origin)
        lo, hi, faces = ctx.adjacency()
        assert np.array_equal(lo.astype(np.int64), want["lo"]) and np.array_equal(hi.astype(np.int64), want["hi"])
        got = dict(zip(("fwd", "rev", "sum1", "sum2"), ctx.wallgeo_get()))
        for name in ("fwd", "rev", "sum1", "sum2"):
            assert got[name].shape == want[name].shape, name
            assert np.array_equal(got[name], want[name]), name
        assert np.array_equal(got["fwd"] + got["rev"], faces)
        debug = ctx.wallgeo_debug()
        assert debug["spills"] == ctx.wallgeo_spills()
        if want["lo"].size:
            self.check_plan(debug, "wallgeo")
        else:                                                        # no pair, no launch
            assert (debug["tiles_per_group"], debug["groups"], debug["spills"]) == (0, 0, 0)
        return debug, want
