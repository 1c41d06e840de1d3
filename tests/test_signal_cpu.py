"""Signal statistics without a GPU: the NumPy restatement (tests/signal_reference.py) against scipy.ndimage and the C oracle's
face counts, and the C ABI of include/tissue_scan_signal.h (declarations, exports, NULL-context checks)."""
import ctypes
import os
import re

import numpy as np
import pytest

import signal_reference as ref
from tissue_analysis_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_signal_symbols():
    text = open(os.path.join(ROOT, "include", "tissue_scan_signal.h")).read()
    return sorted(set(re.findall(r"TA_API\s+(?:const\s+char\s*\*|int)\s+(ta_\w+)\s*\(", text)))


def _volumes():
    rng = np.random.default_rng(20261016)
    for shape, nlab, dt, st in (((6, 7, 9), 5, np.uint16, np.uint8), ((3, 11, 4), 30, np.uint32, np.uint16),
                                ((9, 1, 13), 3, np.uint16, np.uint16), ((5, 5, 1), 4, np.uint32, np.uint8)):
        V = rng.integers(0, nlab, size=shape).astype(dt)
        S = rng.integers(0, np.iinfo(st).max, size=shape, endpoint=True).astype(st)
        yield V, S, nlab


def test_restatement_agrees_with_scipy_ndimage():
    from scipy import ndimage
    for V, S, nlab in _volumes():
        r = ref.labels(V, S, nlab)
        m = ref.moments(r)
        idx = np.arange(nlab)
        present = r["n"] > 0
        Sf = S.astype(np.float64)
        assert np.array_equal(r["n"], np.bincount(V.reshape(-1).astype(np.int64), minlength=nlab))
        assert np.array_equal(r["sum"][present], np.asarray(ndimage.sum_labels(Sf, V, idx[present])).astype(np.uint64))
        np.testing.assert_allclose(m["mean"][present], ndimage.mean(Sf, V, idx[present]), rtol=1e-12)
        np.testing.assert_allclose(m["std"][present] ** 2, ndimage.variance(Sf, V, idx[present]), rtol=1e-9, atol=1e-9)
        assert np.array_equal(m["min"][present], ndimage.minimum(Sf, V, idx[present]))
        assert np.array_equal(m["max"][present], ndimage.maximum(Sf, V, idx[present]))


def test_restatement_faces_equal_the_c_oracle():
    from oracle import onepass_c
    for V, S, _ in _volumes():
        w = ref.walls(V, S)
        o = onepass_c.extract(V)
        assert np.array_equal(w["lo"], o["pair_lo"]) and np.array_equal(w["hi"], o["pair_hi"])
        assert np.array_equal(w["faces"], o["pair_faces"])


def test_restatement_halo_slabs_sum_to_the_whole():
    for V, S, nlab in _volumes():
        if V.shape[0] < 4:
            continue
        whole_l, whole_w = ref.labels(V, S, nlab), ref.walls(V, S)
        cut = V.shape[0] // 2
        a_l, a_w = ref.labels(V[:cut], S[:cut], nlab), ref.walls(V[:cut], S[:cut])
        b_l = ref.labels(V[cut - 1:], S[cut - 1:], nlab, first_owned=1)
        b_w = ref.walls(V[cut - 1:], S[cut - 1:], first_owned=1)
        for k in ("n", "sum", "sumsq"):
            assert np.array_equal(a_l[k] + b_l[k], whole_l[k]), k
        got = {}
        for w in (a_w, b_w):
            for key, lo, hi in zip(w["keys"].tolist(), w["side_lo"].tolist(), w["side_hi"].tolist()):
                g = got.setdefault(key, [0, 0])
                g[0] += lo
                g[1] += hi
        assert sorted(got) == whole_w["keys"].tolist()
        assert [got[k] for k in whole_w["keys"].tolist()] == [[a, b] for a, b in zip(whole_w["side_lo"].tolist(),
                                                                                      whole_w["side_hi"].tolist())]


def test_signal_header_and_binding_agree():
    assert declared_signal_symbols() == sorted(_capi.SIGNAL_SYMBOLS)


def test_signal_symbols_are_not_in_the_core_list():
    assert not set(_capi.SIGNAL_SYMBOLS) & set(_capi.SYMBOLS)


def test_library_exports_the_signal_symbols_and_they_reject_a_null_context():
    lib = _capi.load()
    i64 = (ctypes.c_int64 * 3)(4, 4, 4)
    buf = (ctypes.c_uint64 * 64)()
    dbl = ctypes.c_double(0)
    calls = {
        "ta_signal_set": (None, buf, 1, i64, None),
        "ta_signal_set_device": (None, buf, 1),
        "ta_signal_extract": (None, 3),
        "ta_signal_get_labels": (None, buf, buf, buf, buf, buf),
        "ta_signal_get_walls": (None, buf, buf),
        "ta_signal_timing": (None, ctypes.byref(dbl)),
        "ta_signal_debug": (None, (ctypes.c_uint32 * 4)()),
    }
    assert sorted(calls) == sorted(_capi.SIGNAL_SYMBOLS)
    for name in declared_signal_symbols():
        assert hasattr(lib, name), name
        assert getattr(lib, name)(*calls[name]) == _capi.TA_EINVAL, name
        err = lib.ta_last_error()
        assert b"NULL" in err or b"ctx" in err, (name, err)


def test_signal_dtype_is_checked_before_any_device_work():
    ctx = _capi.Context.__new__(_capi.Context)          # (no GPU needed: the checks run before the C call)
    ctx._vol_layout = ((4, 4, 4), (16, 4, 1))
    with pytest.raises(TypeError, match="uint8 or uint16"):
        _capi.Context.set_signal(ctx, np.zeros((4, 4, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        _capi.Context.set_signal(ctx, np.zeros((4, 4, 5), dtype=np.uint8))
