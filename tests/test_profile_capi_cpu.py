"""include/tissue_scan_profile.h against the binding and the library, without a GPU: the declared names are
_capi.PROFILE_SYMBOLS, the library exports them, and a NULL context is refused before anything touches a device."""
import ctypes
import os
import re

from tissue_analysis_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "tissue_scan_profile.h")).read()


def test_header_and_binding_agree():
    declared = sorted(set(re.findall(r"TA_API\s+int\s+(ta_\w+)\s*\(", header())))
    assert declared == sorted(_capi.PROFILE_SYMBOLS) and len(declared) == 4
    lib = _capi.load()
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name


def test_constants_agree():
    text = header()
    assert int(re.search(r"#define\s+TA_PROF_SIGNAL\s+(\d+)u", text).group(1)) == _capi.PROF_SIGNAL
    assert int(re.search(r"#define\s+TA_PROF_MAX_BINS\s+(\d+)", text).group(1)) == _capi.PROFILE_MAX_BINS
    kernel_header = open(os.path.join(ROOT, "tissue_analysis_amd", "csrc", "ta_profile.h")).read()
    assert int(re.search(r"PROF_SLOTS\s*=\s*(\d+)", kernel_header).group(1)) == _capi.PROFILE_SLOTS


def test_a_null_context_is_refused_without_a_gpu():
    lib = _capi.load()
    edges = (ctypes.c_double * 3)(0.0, 1.0, 4.0)
    assert lib.ta_profile_extract(None, 2, edges, 0) == _capi.TA_EINVAL
    assert b"NULL" in lib.ta_last_error()
    assert lib.ta_profile_extract(None, 2, edges, _capi.PROF_SIGNAL) == _capi.TA_EINVAL
    assert lib.ta_profile_get(None, None, None, None, None, None) == _capi.TA_EINVAL
    out = (ctypes.c_uint32 * 4)()
    assert lib.ta_profile_debug(None, out) == _capi.TA_EINVAL
    ms = ctypes.c_double(-1.0)
    assert lib.ta_profile_timing(None, ctypes.byref(ms)) == _capi.TA_EINVAL and ms.value == -1.0
