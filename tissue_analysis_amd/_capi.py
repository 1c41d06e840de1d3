"""ctypes binding of include/tissue_scan.h (libtissue_scan.so).

This is the only door from Python into the HIP kernels.  There is no CPU fallback: if the
shared library is missing, or no gfx950 GPU is visible, the product path raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TISSUE_SCAN_LIB") or os.path.join(_HERE, "libtissue_scan.so")

TA_OK, TA_EINVAL, TA_EHIP, TA_ENOMEM, TA_ERANGE, TA_ECAPACITY, TA_ENODEVICE = 0, -1, -2, -3, -4, -5, -6
F_VOLUME, F_BBOX, F_MOMENT1, F_MOMENT2, F_ADJACENCY = 1, 2, 4, 8, 16
F_ALL = 31
ADJ_LOCAL, ADJ_MERGED, ADJ_PARTIAL = 0, 1, 2
ABI_VERSION = 5          # TA_ABI_VERSION of include/tissue_scan.h this binding was written against
FEATURES = dict(VOLUME=F_VOLUME, BBOX=F_BBOX, MOMENT1=F_MOMENT1, MOMENT2=F_MOMENT2,
                ADJACENCY=F_ADJACENCY)
OPT_IMPL, OPT_TILE_PLANES, OPT_PAIR_SLOTS, OPT_TIMING, OPT_TIMING_RING, OPT_VOLUME_SLACK, OPT_SWEEP_SHAPE, OPT_SWEEP_SHAPE_USED = 1, 2, 3, 4, 5, 6, 7, 8
OPT_TILE_PLANES_USED = 9         # read only: the tile height the last sweep was launched with (0 before any sweep)
STREAM_LEGACY_DEFAULT = 1          # TA_STREAM_LEGACY_DEFAULT of include/tissue_scan.h

_vp, _i64, _u32, _u64, _ci, _f64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_double
_P = ctypes.POINTER

# Every symbol every header under include/ declares, with its (restype, argtypes): the one list of them.  All live in the same
# library; `load()` walks this table, and the *_SYMBOLS tuples below are its keys, header by header.
DECLARED = {
    "tissue_scan.h": {
        "ta_version": (_ci, []),
        "ta_adjacency_scope": (_ci, [_vp, _P(_ci)]),
        "ta_last_error": (ctypes.c_char_p, []),
        "ta_device_count": (_ci, [_P(_ci)]),
        "ta_ctx_create": (_ci, [_ci, _P(_vp)]),
        "ta_ctx_destroy": (_ci, [_vp]),
        "ta_ctx_set_stream": (_ci, [_vp, _vp]),
        "ta_ctx_set_option": (_ci, [_vp, _ci, _i64]),
        "ta_ctx_get_option": (_ci, [_vp, _ci, _P(_i64)]),
        "ta_ctx_synchronize": (_ci, [_vp]),
        "ta_volume_set": (_ci, [_vp, _vp, _ci, _P(_i64), _P(_i64)]),
        "ta_volume_set_device": (_ci, [_vp, _vp, _ci, _P(_i64), _i64, _ci]),
        "ta_volume_max_label": (_ci, [_vp, _P(_u32)]),
        "ta_volume_label_census": (_ci, [_vp, _P(_u32), _P(_u32)]),
        "ta_label_census_get": (_ci, [_vp, _vp]),
        "ta_volume_compact_labels": (_ci, [_vp, _vp, _u32, _P(_u32)]),
        "ta_volume_is_compact": (_ci, [_vp, _P(_ci), _P(_u32)]),
        "ta_volume_rerank": (_ci, [_vp]),
        "ta_volume_uncompact": (_ci, [_vp]),
        "ta_volume_owned_planes": (_ci, [_vp, _P(_i64)]),
        "ta_volume_plane_events": (_ci, [_vp, _vp]),
        "ta_volume_relabel": (_ci, [_vp, _vp, _u32]),
        "ta_volume_get": (_ci, [_vp, _vp]),
        "ta_volume_map": (_ci, [_vp, _vp, _u32, _vp, _ci, _vp]),
        "ta_volume_first_layer": (_ci, [_vp, _u32, _ci, _vp]),
        "ta_volume_hollow": (_ci, [_vp, _u32, _ci, _ci, _vp]),
        "ta_volume_layer18": (_ci, [_vp, _vp]),
        "ta_wall_voxels_count": (_ci, [_vp, _P(_i64)]),
        "ta_wall_voxels_get": (_ci, [_vp, _vp, _vp, _P(_f64)]),
        "ta_wall_medians": (_ci, [_vp, _ci, _P(_i64), _P(_f64)]),
        "ta_wall_medians_get": (_ci, [_vp, _vp, _vp, _vp]),
        "ta_wall_voxels_get_by_pair": (_ci, [_vp, _vp, _vp, _P(_f64)]),
        "ta_extract": (_ci, [_vp, _u32, _u32]),
        "ta_get_labels": (_ci, [_vp, _vp, _vp, _vp, _vp]),
        "ta_adjacency_size": (_ci, [_vp, _P(_i64)]),
        "ta_adjacency_get": (_ci, [_vp, _vp, _vp, _vp]),
        "ta_timing": (_ci, [_vp, _P(_f64), _P(_f64), _P(_f64), _P(_u64)]),
        "ta_timing_series": (_ci, [_vp, _P(_f64), _ci, _P(_ci)]),
        "ta_read_probe": (_ci, [_vp, _vp, _u64, _ci, _P(_f64)]),
        "ta_debug_counters": (_ci, [_vp, _P(_u32)]),
        "ta_bind_accumulators": (_ci, [_vp, _vp, _vp, _u32]),
        "ta_accumulators_device": (_ci, [_vp, _P(_vp), _P(_vp), _P(_u32)]),
        "ta_accumulators_reduced": (_ci, [_vp]),
        "ta_adjacency_device": (_ci, [_vp, _P(_vp), _P(_vp), _P(_i64)]),
        "ta_adjacency_export": (_ci, [_vp, _vp, _vp, _i64]),
        "ta_adjacency_merge": (_ci, [_vp, _vp, _vp, _i64]),
        "ta_adjacency_pack": (_ci, [_vp, _vp, _i64]),
        "ta_adjacency_pack_shared": (_ci, [_vp, _vp, _i64]),
        "ta_adjacency_merge_blocks": (_ci, [_vp, _vp, _ci, _i64]),
        "ta_synth_voronoi": (_ci, [_vp, _vp, _ci, _P(_i64), _i64, _i64, _vp, _P(ctypes.c_int32), _vp]),
        "ta_device_malloc": (_ci, [_vp, _u64, _P(_vp)]),
        "ta_device_free": (_ci, [_vp, _vp]),
        "ta_memcpy_d2h": (_ci, [_vp, _vp, _vp, _u64]),
        "ta_memcpy_h2d": (_ci, [_vp, _vp, _vp, _u64]),
    },
    "tissue_scan_signal.h": {
        "ta_signal_set": (_ci, [_vp, _vp, _ci, _P(_i64), _P(_i64)]),
        "ta_signal_set_device": (_ci, [_vp, _vp, _ci]),
        "ta_signal_extract": (_ci, [_vp, _u32]),
        "ta_signal_get_labels": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp]),
        "ta_signal_get_walls": (_ci, [_vp, _vp, _vp]),
        "ta_signal_timing": (_ci, [_vp, _P(_f64)]),
        "ta_signal_debug": (_ci, [_vp, _P(_u32)]),
    },
    "tissue_scan_mesh.h": {
        "ta_mesh_extract": (_ci, [_vp, _ci, _vp]),
        "ta_mesh_size": (_ci, [_vp, _P(_u64), _P(_u64), _P(_u64)]),
        "ta_mesh_get": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "ta_mesh_timing": (_ci, [_vp, _P(_f64)]),
    },
    "tissue_scan_overlap.h": {
        "ta_overlap_set": (_ci, [_vp, _vp, _ci, _P(_i64), _P(_i64)]),
        "ta_overlap_set_device": (_ci, [_vp, _vp, _ci]),
        "ta_overlap_set_capacity": (_ci, [_vp, _ci]),
        "ta_overlap_extract": (_ci, [_vp]),
        "ta_overlap_size": (_ci, [_vp, _P(_u64)]),
        "ta_overlap_get": (_ci, [_vp, _vp, _vp, _vp]),
        "ta_overlap_timing": (_ci, [_vp, _P(_f64)]),
        "ta_overlap_timing_compaction": (_ci, [_vp, _P(_f64), _P(_ci)]),
        "ta_overlap_debug": (_ci, [_vp, _P(_u32)]),
    },
    "tissue_scan_junctions.h": {
        "ta_junctions_extract": (_ci, [_vp]),
        "ta_junctions_size": (_ci, [_vp, _P(_u64), _P(_u64), _P(_u64)]),
        "ta_junctions_get_edges": (_ci, [_vp, _vp, _vp, _vp]),
        "ta_junctions_get_vertices": (_ci, [_vp, _vp, _vp, _vp]),
        "ta_junctions_timing": (_ci, [_vp, _P(_f64), _P(_f64)]),
        "ta_junctions_debug": (_ci, [_vp, _P(_u32)]),
    },
    "tissue_scan_wallgeo.h": {
        "ta_wallgeo_extract": (_ci, [_vp]),
        "ta_wallgeo_get": (_ci, [_vp, _vp, _vp, _vp, _vp]),
        "ta_wallgeo_spills": (_ci, [_vp, _P(_u32)]),
        "ta_wallgeo_debug": (_ci, [_vp, _P(_u32)]),
        "ta_wallgeo_timing": (_ci, [_vp, _P(_f64)]),
    },
    "tissue_scan_components.h": {
        "ta_components_extract": (_ci, [_vp]),
        "ta_components_size": (_ci, [_vp, _P(_u64)]),
        "ta_components_get": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp]),
        "ta_components_image": (_ci, [_vp, _i64, _i64, _vp]),
        "ta_components_relabel": (_ci, [_vp, _vp, _u64]),
        "ta_components_timing": (_ci, [_vp, _P(_f64), _P(_f64)]),
        "ta_components_debug": (_ci, [_vp, _P(_u32)]),
    },
    "tissue_scan_distance.h": {
        "ta_distance_extract": (_ci, [_vp, _ci, _u32, _P(_f64), _u32]),
        "ta_distance_get": (_ci, [_vp, _vp, _vp, _vp]),
        "ta_distance_image": (_ci, [_vp, _i64, _i64, _vp]),
        "ta_distance_timing": (_ci, [_vp, _P(_f64), _P(_f64)]),
        "ta_distance_set_batch": (_ci, [_vp, _i64]),
        "ta_distance_debug": (_ci, [_vp, _P(_u32)]),
    },
    "tissue_scan_nearest.h": {
        "ta_nearest_extract": (_ci, [_vp, _u32, _u32, _P(_f64), _f64, _u32]),
        "ta_nearest_get": (_ci, [_vp, _vp, _vp]),
        "ta_nearest_image": (_ci, [_vp, _i64, _i64, _vp, _vp]),
        "ta_nearest_apply": (_ci, [_vp]),
        "ta_nearest_timing": (_ci, [_vp, _P(_f64), _P(_f64)]),
        "ta_nearest_debug": (_ci, [_vp, _P(_u32)]),
        "ta_nearest_set_batch": (_ci, [_vp, _i64]),
    },
    "tissue_scan_profile.h": {
        "ta_profile_extract": (_ci, [_vp, _ci, _P(_f64), _u32]),
        "ta_profile_get": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp]),
        "ta_profile_debug": (_ci, [_vp, _P(_u32)]),
        "ta_profile_timing": (_ci, [_vp, _P(_f64)]),
    },
    "tissue_scan_sighist.h": {
        "ta_sighist_extract": (_ci, [_vp, _ci]),
        "ta_sighist_get": (_ci, [_vp, _vp]),
        "ta_sigrank_extract": (_ci, [_vp, _ci, _vp]),
        "ta_sigrank_get": (_ci, [_vp, _vp]),
        "ta_sighist_debug": (_ci, [_vp, _P(_u32)]),
        "ta_sighist_timing": (_ci, [_vp, _P(_f64), _P(_f64)]),
    },
    "tissue_scan_sigmoments.h": {
        "ta_sigmom_extract": (_ci, [_vp]),
        "ta_sigmom_get": (_ci, [_vp, _vp, _vp, _vp, _vp]),
        "ta_sigmom_debug": (_ci, [_vp, _P(_u32)]),
        "ta_sigmom_timing": (_ci, [_vp, _P(_f64)]),
    },
    "tissue_scan_cosignal.h": {
        "ta_cosignal_set": (_ci, [_vp, _vp, _ci, _P(_i64), _P(_i64)]),
        "ta_cosignal_set_device": (_ci, [_vp, _vp, _ci]),
        "ta_cosignal_extract": (_ci, [_vp, _u32, _u32]),
        "ta_cosignal_get": (_ci, [_vp] + [_vp] * 11),
        "ta_cosignal_debug": (_ci, [_vp, _P(_u32)]),
        "ta_cosignal_timing": (_ci, [_vp, _P(_f64)]),
        "ta_cosignal_thresholds": (_ci, [_vp, _P(_u32), _P(_u32)]),
    },
    "tissue_scan_topology.h": {
        "ta_topology_extract": (_ci, [_vp]),
        "ta_topology_get": (_ci, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "ta_topology_debug": (_ci, [_vp, _P(_u32)]),
        "ta_topology_timing": (_ci, [_vp, _P(_f64)]),
    },
    "tissue_scan_resample.h": {
        "ta_resample_set_source": (_ci, [_vp, _vp, _ci, _P(_i64), _P(_i64)]),
        "ta_resample_set_source_device": (_ci, [_vp, _vp, _ci, _P(_i64)]),
        "ta_resample_extract": (_ci, [_vp, _P(_f64), _ci, _u32]),
        "ta_resample_get": (_ci, [_vp, _vp, _i64, _i64]),
        "ta_resample_device": (_ci, [_vp, _P(_vp), _P(_ci)]),
        "ta_resample_outside": (_ci, [_vp, _P(_u64)]),
        "ta_resample_timing": (_ci, [_vp, _P(_f64)]),
        "ta_resample_debug": (_ci, [_vp, _P(_u32)]),
        "ta_resample_as_overlap": (_ci, [_vp]),
        "ta_resample_as_signal": (_ci, [_vp]),
    },
    "tissue_scan_extents.h": {
        "ta_extents_extract": (_ci, [_vp, _P(_f64), _u32]),
        "ta_extents_get": (_ci, [_vp, _vp, _vp]),
        "ta_extents_debug": (_ci, [_vp, _P(_u32)]),
        "ta_extents_timing": (_ci, [_vp, _P(_f64)]),
    },
}

SYMBOLS = tuple(DECLARED["tissue_scan.h"])          # (kept apart from the feature headers' lists: this is tissue_scan.h's)

SIGNAL_SYMBOLS = tuple(DECLARED["tissue_scan_signal.h"])
SIG_LABELS, SIG_WALLS = 1, 2           # TA_SIG_LABELS / TA_SIG_WALLS
SIGNAL_DTYPES = (np.uint8, np.uint16)

MESH_SYMBOLS = tuple(DECLARED["tissue_scan_mesh.h"])
MESH_OUTSIDE = 0xFFFFFFFF              # TA_MESH_OUTSIDE

OVERLAP_SYMBOLS = tuple(DECLARED["tissue_scan_overlap.h"])

JUNCTION_SYMBOLS = tuple(DECLARED["tissue_scan_junctions.h"])

WALLGEO_SYMBOLS = tuple(DECLARED["tissue_scan_wallgeo.h"])

COMPONENT_SYMBOLS = tuple(DECLARED["tissue_scan_components.h"])
COMPONENT_NONE = 0xFFFFFFFF            # TA_COMPONENT_NONE
COMPONENT_MAX_VOXELS = 1 << 31         # voxels of a buffer the component pass takes

DISTANCE_SYMBOLS = tuple(DECLARED["tissue_scan_distance.h"])
DIST_OWN_WALL, DIST_FROM_LABEL = 0, 1  # TA_DIST_OWN_WALL / TA_DIST_FROM_LABEL
DIST_EDGE_IS_SITE = 1                  # TA_DIST_EDGE_IS_SITE

NEAREST_SYMBOLS = tuple(DECLARED["tissue_scan_nearest.h"])
NEAREST_NOT_FROM = 1                   # TA_NEAREST_NOT_FROM
NEAREST_NONE = 0xFFFFFFFF              # TA_NEAREST_NONE

PROFILE_SYMBOLS = tuple(DECLARED["tissue_scan_profile.h"])
PROF_SIGNAL = 1                        # TA_PROF_SIGNAL
PROFILE_MAX_BINS = 64                  # TA_PROF_MAX_BINS
PROFILE_SLOTS = 1024                   # PROF_SLOTS of csrc/ta_profile.h: slots of a workgroup's LDS table

SIGHIST_SYMBOLS = tuple(DECLARED["tissue_scan_sighist.h"])
SIGRANK_MAX_RANKS = 8                  # TA_SIGRANK_MAX_RANKS
SIGRANK_NONE = 0xFFFFFFFF              # value of a rank >= n
SIGHIST_SLOTS = 39                     # TA_SH_SLOTS of csrc/ta_sighist.h: rows of 256 counters in a workgroup's LDS table
SIGHIST_MAX_GROUPS = 65536             # TA_SH_MAX_GROUPS: workgroups of the digit pass at most (the plan: tests/sighist_reference.py)

SIGMOM_SYMBOLS = tuple(DECLARED["tissue_scan_sigmoments.h"])
SIGMOM_SLOTS = 448                     # SM_SLOTS of csrc/ta_sigmoments.h: rows of a workgroup's LDS table
SIGMOM_MAX_GROUPS = 1024               # SM_MAX_GROUPS: workgroups of the pass at most (the plan: tests/sigmoment_reference.py)

COSIGNAL_SYMBOLS = tuple(DECLARED["tissue_scan_cosignal.h"])
COSIGNAL_COLUMNS = ("n", "sum_a", "sum_b", "sq_aa", "sq_bb", "sq_ab", "n_a", "n_b", "n_ab", "sum_a_over", "sum_b_over")   # ta_cosignal_get's order
COSIG_SLOTS = 512                      # COSIG_SLOTS of csrc/ta_cosignal.h: rows of a workgroup's LDS table
COSIG_MAX_GROUPS = 1024                # COSIG_MAX_GROUPS: workgroups of the pass at most (the plan: that of the signal pass)

TOPOLOGY_SYMBOLS = tuple(DECLARED["tissue_scan_topology.h"])
TOPOLOGY_SLOTS = 768                   # TP_SLOTS of csrc/ta_topology.h: rows of a workgroup's LDS table
TOPOLOGY_MAX_GROUPS = 1024             # TP_MAX_GROUPS: workgroups of the pass at most (the plan: tests/topology_reference.py)

RESAMPLE_SYMBOLS = tuple(DECLARED["tissue_scan_resample.h"])
RS_NEAREST, RS_LINEAR = 0, 1           # TA_RS_NEAREST / TA_RS_LINEAR
RESAMPLE_DTYPES = (np.uint8, np.uint16, np.uint32)

EXTENT_SYMBOLS = tuple(DECLARED["tissue_scan_extents.h"])
EXTENT_SLOTS = 768                     # EX_SLOTS of csrc/ta_extents.h: rows of a workgroup's LDS table
EXTENT_MAX_GROUPS = 1024               # EX_MAX_GROUPS: workgroups of the pass at most (the plan: tests/extent_reference.py)


def exchange_words(capacity_pairs):
    """uint64 words of one exchange block (TA_EXCHANGE_WORDS in include/tissue_scan.h)."""
    return 2 + 4 * int(capacity_pairs)


class TissueScanError(RuntimeError):
    def __init__(self, code, message):
        RuntimeError.__init__(self, "libtissue_scan error %d: %s" % (code, message))
        self.code = code


_lib = None


def load():
    """Load libtissue_scan.so (built in-tree by `python -m tissue_analysis_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: the HIP extension has not been built "
            "(run `python -m tissue_analysis_amd.build`); there is no CPU fallback" % LIB_PATH)
    # PyTorch-ROCm ships its own copy of the HIP / HSA runtime; libtissue_scan.so is linked against /opt/rocm's.  Two
    # runtimes in one process cannot both open the GPU ("No HIP GPUs are available" from whichever comes second) unless
    # torch's is the one the loader sees first -- then this library binds to it too.  So when torch is installed, it is
    # imported before the library is opened, whatever order the caller's imports have.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for symbols in DECLARED.values():
        for name, (restype, argtypes) in symbols.items():
            fn = getattr(lib, name)      # AttributeError here == the .so does not match the header
            fn.restype, fn.argtypes = restype, argtypes
    if lib.ta_version() != ABI_VERSION:
        raise ImportError("%s speaks ABI version %d, this binding %d: rebuild it (python -m tissue_analysis_amd.build --force)"
                          % (LIB_PATH, lib.ta_version(), ABI_VERSION))
    _lib = lib
    return lib


def _check(rc):
    if rc != TA_OK:
        raise TissueScanError(rc, load().ta_last_error().decode(errors="replace"))


def device_count():
    n = ctypes.c_int(0)
    _check(load().ta_device_count(ctypes.byref(n)))
    return n.value


def feature_mask(names):
    if isinstance(names, int):
        return names
    m = 0
    for n in names:
        m |= FEATURES[n.upper()]
    return m


def _i64x3(v):
    return (ctypes.c_int64 * 3)(*[int(x) for x in v])


def _spacing(spacing):
    sp = [float(v) for v in spacing]
    if len(sp) != 3:
        raise ValueError("spacing must have three entries")
    return (ctypes.c_double * 3)(*sp)


def _dense_permuted(a):
    """True when the array is dense in some axis permutation (C, F or transposed layouts)."""
    order = sorted(range(a.ndim), key=lambda d: (a.shape[d] != 1, -a.strides[d]))
    expect = a.dtype.itemsize
    for d in reversed(order):
        if a.shape[d] != 1 and a.strides[d] != expect:
            return False
        expect *= a.shape[d]
    return True


def _empty_like(like, what, dtype=None):
    """An array for the pass `what` to fill: the shape and the memory order of `like` (the array given to set_volume)."""
    out = np.empty_like(like, dtype=dtype)
    if not _dense_permuted(out):
        raise ValueError("%s needs a dense (possibly axis-permuted) volume" % what)
    return out


class Context(object):
    """One ta_ctx == one GPU.  Thin, explicit wrapper: every method is one C call."""

    def __init__(self, device=0, stream=None):
        self._lib = load()
        self._h = ctypes.c_void_p()
        _check(self._lib.ta_ctx_create(int(device), ctypes.byref(self._h)))
        self.device = int(device)
        self._keep = []      # objects whose device memory the context currently points at
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ta_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()
        self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _doubles(self, fn, n, *more):
        """The n doubles that fn(ctx, &d[0], .., &d[n - 1], *more) writes -- the shape of every ta_*_timing."""
        out = [ctypes.c_double(0.0) for _ in range(n)]
        _check(fn(self._h, *([ctypes.byref(v) for v in out] + list(more))))
        return tuple(v.value for v in out)

    def _debug_words(self, fn):
        """The four uint32 words that fn(ctx, out[4]) writes -- the shape of every ta_*_debug."""
        out = (ctypes.c_uint32 * 4)()
        _check(fn(self._h, out))
        return [int(v) for v in out]

    def _census_ids(self, n):
        """The n ascending ids (uint32) of the census the context holds."""
        ids = np.zeros(n, dtype=np.uint32)
        if n:
            _check(self._lib.ta_label_census_get(self._h, ids.ctypes.data_as(ctypes.c_void_p)))
        return ids

    # -- plumbing
    def set_stream(self, stream_handle):
        """stream_handle: a hipStream_t as an integer; 0 = the device's legacy default (null) stream -- what
        torch.cuda.default_stream().cuda_stream is; None = a private non-blocking stream owned by the context."""
        if stream_handle is None:
            h = 0
        elif int(stream_handle) == 0:
            h = STREAM_LEGACY_DEFAULT
        else:
            h = int(stream_handle)
        _check(self._lib.ta_ctx_set_stream(self._h, ctypes.c_void_p(h)))

    def set_option(self, key, value):
        _check(self._lib.ta_ctx_set_option(self._h, int(key), int(value)))

    def get_option(self, key):
        v = ctypes.c_int64(0)
        _check(self._lib.ta_ctx_get_option(self._h, int(key), ctypes.byref(v)))
        return int(v.value)

    def synchronize(self):
        _check(self._lib.ta_ctx_synchronize(self._h))

    # -- volume
    def set_volume(self, array):
        """Upload a uint16/uint32 numpy volume in whatever dense layout it has."""
        a = np.asarray(array)
        if a.ndim != 3:
            raise ValueError("a 3D volume is required")
        if a.dtype not in (np.uint16, np.uint32):
            raise TypeError("label volumes must be uint16 or uint32, not %s" % a.dtype)
        if not _dense_permuted(a):
            a = np.ascontiguousarray(a)
        _check(self._lib.ta_volume_set(self._h, ctypes.c_void_p(a.ctypes.data), a.dtype.itemsize,
                                       _i64x3(a.shape), _i64x3(a.strides)))
        self._vol_layout = (tuple(a.shape), tuple(s // a.dtype.itemsize for s in a.strides))
        # the library's order of the axes in memory: by decreasing stride, size-1 axes first
        self._memory_axes = tuple(sorted(range(3), key=lambda d: -(float("inf") if a.shape[d] == 1 else a.strides[d])))
        self._owned_planes = int(a.shape[int(np.argmax(a.strides))])         # planes of the slowest MEMORY axis
        self._halo_planes = 0

    def relabel(self, lut):
        """In place on the resident volume: v -> lut[v] for v < len(lut) (host uint32 table)."""
        lut = np.ascontiguousarray(lut, dtype=np.uint32)
        _check(self._lib.ta_volume_relabel(self._h, ctypes.c_void_p(lut.ctypes.data), int(lut.size)))

    def get_volume(self, out):
        """Copy the resident volume into `out`, which must have the dtype, shape and dense layout
        of the array given to set_volume()."""
        if not (isinstance(out, np.ndarray) and _dense_permuted(out) and out.flags.writeable):
            raise ValueError("get_volume needs a writeable dense (possibly axis-permuted) ndarray")
        _check(self._lib.ta_volume_get(self._h, ctypes.c_void_p(out.ctypes.data)))
        return out

    def map_labels(self, lut, fill, like):
        """out[p] = lut[V[p]] (fill beyond the table): `lut` is a 1-D array of a 1/2/4/8-byte dtype;
        the result has that dtype and the shape and layout of `like` (the array given to set_volume)."""
        lut = np.ascontiguousarray(lut)
        if lut.dtype.itemsize not in (1, 2, 4, 8):
            raise TypeError("lookup tables of %s are not supported" % lut.dtype)
        out = _empty_like(like, "map_labels", lut.dtype)
        fillv = np.array([fill]).astype(lut.dtype)
        _check(self._lib.ta_volume_map(self._h, ctypes.c_void_p(lut.ctypes.data), int(lut.size),
                                       ctypes.c_void_p(fillv.ctypes.data), int(lut.dtype.itemsize),
                                       ctypes.c_void_p(out.ctypes.data)))
        return out

    def first_layer(self, background, keep_background, like):
        """voxel_first_layer of the resident volume (SIA:1024-1046) as a host image shaped and laid out like `like`
        (the array given to set_volume)."""
        out = _empty_like(like, "first_layer")
        _check(self._lib.ta_volume_first_layer(self._h, int(background), int(bool(keep_background)),
                                               ctypes.c_void_p(out.ctypes.data)))
        return out

    def hollow(self, background, remove_background, like, label_bits=0):
        """hollow_out_cells of the resident volume (SIA:74-95): the labels where their integer Laplacian (modulo
        2^label_bits, 0 = the volume's own width) is not zero (and, with remove_background, where they are not the
        background), 0 elsewhere; shaped and laid out like `like`."""
        out = _empty_like(like, "hollow")
        _check(self._lib.ta_volume_hollow(self._h, int(background) & 0xFFFFFFFF, int(bool(remove_background)), int(label_bits),
                                          ctypes.c_void_p(out.ctypes.data)))
        return out

    def layer18(self, like):
        """uint8 image, 1 where a voxel has one of its 18 neighbours in another label (cells_voxel_layer, SIA:1399-1448,
        for every label at once); shaped and laid out like `like`."""
        out = _empty_like(like, "layer18", np.uint8)
        _check(self._lib.ta_volume_layer18(self._h, ctypes.c_void_p(out.ctypes.data)))
        return out

    def wall_voxels(self, by_pair=False):
        """All (pair, wall voxel) records of the resident volume: lo u32[n], hi u32[n], coords i32[n,3]
        (array-axis order), ordered by the voxel's position in memory -- or, with by_pair, grouped by (lo, hi) on the
        device with each pair's voxels in memory order; plus the kernels' milliseconds."""
        n = ctypes.c_int64(0)
        _check(self._lib.ta_wall_voxels_count(self._h, ctypes.byref(n)))
        pairs = np.empty((n.value, 2), dtype=np.uint32)
        coords = np.empty((n.value, 3), dtype=np.int32)
        ms = ctypes.c_double(0.0)
        fetch = self._lib.ta_wall_voxels_get_by_pair if by_pair else self._lib.ta_wall_voxels_get
        _check(fetch(self._h, pairs.ctypes.data, coords.ctypes.data, ctypes.byref(ms)))
        return pairs[:, 0], pairs[:, 1], coords, ms.value

    def wall_medians(self, max_iter=200):
        """The median voxel of every wall of the resident volume, computed on the device (C-ordered volumes): keys
        uint64[E] = lo << 32 | hi ascending, sizes uint32[E] (wall voxels), medians int32[E, 3] (array-axis order), and
        the kernels' milliseconds (grouping by pair included) and `moving` bool[E]: walls whose iteration had not settled after
        `max_iter` Weiszfeld passes (the reference raises for such a wall: the caller does, for the walls it asks for)."""
        n = ctypes.c_int64(0)
        _check(self._lib.ta_wall_voxels_count(self._h, ctypes.byref(n)))
        count, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
        _check(self._lib.ta_wall_medians(self._h, int(max_iter), ctypes.byref(count), ctypes.byref(ms)))
        E = count.value
        pairs = np.empty((E, 2), dtype=np.uint32)
        sizes = np.empty(E, dtype=np.uint32)
        med = np.empty((E, 3), dtype=np.int32)
        _check(self._lib.ta_wall_medians_get(self._h, pairs.ctypes.data, sizes.ctypes.data, med.ctypes.data))
        keys = (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64)
        moving = (sizes & np.uint32(0x80000000)) != 0
        return keys, sizes & np.uint32(0x7FFFFFFF), med, ms.value, moving

    def set_volume_device(self, dev_ptr, itemsize, buf_dims, a0_origin=0, has_low_halo=False, keep=None):
        _check(self._lib.ta_volume_set_device(self._h, ctypes.c_void_p(int(dev_ptr)), int(itemsize),
                                              _i64x3(buf_dims), int(a0_origin), int(bool(has_low_halo))))
        d = [int(x) for x in buf_dims]
        self._vol_layout = (tuple(d), (d[1] * d[2], d[2], 1))
        self._memory_axes = (0, 1, 2)
        self._keep = [keep]
        self._owned_planes = int(buf_dims[0]) - (1 if has_low_halo else 0)
        self._halo_planes = 1 if has_low_halo else 0
        # a torch tensor that is a view of a larger storage: tell the library how many bytes are readable behind it
        try:
            st = keep.untyped_storage()
            end = (keep.storage_offset() + keep.numel()) * keep.element_size()
            if keep.is_contiguous() and int(keep.data_ptr()) == int(dev_ptr) and st.nbytes() > end:
                self.set_option(OPT_VOLUME_SLACK, int(st.nbytes() - end))
        except AttributeError:
            pass

    def _in_label_layout(self, a, what):
        """`a` (a companion of the label volume: its signal, the second label volume) with the label volume's shape checked and in
        its memory layout; `what` = what the two error texts call it."""
        layout = getattr(self, "_vol_layout", None)
        if layout is None:
            raise ValueError("set a label volume before %s" % what[0])
        shape, el = layout
        if a.ndim == 2 and len(shape) == 3 and shape[2] == 1:
            a = a[:, :, None]
        if tuple(a.shape) != shape:
            raise ValueError("the %s shape %s differs from the label volume's %s" % (what[1], tuple(a.shape), shape))
        same = all(n == 1 or st == e * a.dtype.itemsize for n, st, e in zip(a.shape, a.strides, el))
        if not same:              # the labels' layout: a flat buffer viewed with their element strides
            flat = np.empty(int(np.prod(shape)), dtype=a.dtype)
            view = np.lib.stride_tricks.as_strided(flat, shape=shape, strides=[e * a.dtype.itemsize for e in el])
            view[...] = a
            a = view
        return a

    def _plane_range(self, first_plane, nplanes):
        """(nplanes, voxels) of `nplanes` buffer planes from `first_plane` along memory axis 0 (None: all that follow)."""
        planes = self.owned_planes() + self._halo_planes          # (asked of the library: a size-1 axis moves the slowest MEMORY axis)
        if nplanes is None:
            nplanes = planes - int(first_plane)
        return int(nplanes), max(int(nplanes), 0) * (int(np.prod(self._vol_layout[0])) // planes)

    # -- signal image (include/tissue_scan_signal.h)
    def set_signal(self, array):
        """Upload a uint8 / uint16 intensity image of the label volume's shape.  One stored in another axis permutation than
        the labels is copied into the labels' layout first."""
        if hasattr(array, "adopt_as_signal"):          # an image on another grid: resampled onto the labels' on the device (resample.OnGrid)
            self._signal_itemsize = array.adopt_as_signal(self)
            return
        a = np.asarray(array)
        if a.dtype not in SIGNAL_DTYPES:
            raise TypeError("signal images must be uint8 or uint16, not %s" % a.dtype)
        a = self._in_label_layout(a, ("its signal", "signal's"))
        _check(self._lib.ta_signal_set(self._h, ctypes.c_void_p(a.ctypes.data), a.dtype.itemsize, _i64x3(a.shape), _i64x3(a.strides)))
        self._signal_itemsize = a.dtype.itemsize

    def set_signal_device(self, dev_ptr, itemsize, keep=None):
        """Adopt a device-resident signal: dense C order with the label volume's buffer dims (halo plane included)."""
        _check(self._lib.ta_signal_set_device(self._h, ctypes.c_void_p(int(dev_ptr)), int(itemsize)))
        self._keep_sig = keep
        self._signal_itemsize = int(itemsize)

    def signal_extract(self, what=SIG_LABELS | SIG_WALLS):
        """Enqueue the signal pass over the current extraction (SIG_LABELS | SIG_WALLS)."""
        _check(self._lib.ta_signal_extract(self._h, int(what)))

    def signal_labels(self):
        """(n u64[R], sum u64[R], sumsq u64[R, 2] (lo, hi words), min u32[R], max u32[R]), rows as labels()."""
        R = self._max_label + 1
        n, s = np.zeros(R, dtype=np.uint64), np.zeros(R, dtype=np.uint64)
        q = np.zeros((R, 2), dtype=np.uint64)
        mn, mx = np.zeros(R, dtype=np.uint32), np.zeros(R, dtype=np.uint32)
        _check(self._lib.ta_signal_get_labels(self._h, n.ctypes.data, s.ctypes.data, q.ctypes.data, mn.ctypes.data, mx.ctypes.data))
        return n, s, q, mn, mx

    def signal_walls(self):
        """(side_lo u64[P], side_hi u64[P]), rows as adjacency()."""
        P = self.adjacency_size()
        lo, hi = np.zeros(P, dtype=np.uint64), np.zeros(P, dtype=np.uint64)
        _check(self._lib.ta_signal_get_walls(self._h, lo.ctypes.data, hi.ctypes.data))
        return lo, hi

    def signal_debug(self):
        """Diagnostics of the last signal pass: records that missed a workgroup's LDS tables (label_spills, pair_spills) and the
        launch plan (tiles_per_group, groups)."""
        out = self._debug_words(self._lib.ta_signal_debug)
        return dict(label_spills=out[0], pair_spills=out[1], tiles_per_group=out[2], groups=out[3])

    def signal_timing(self):
        return self._doubles(self._lib.ta_signal_timing, 1)[0]

    # -- cell meshes (include/tissue_scan_mesh.h)
    def mesh(self, sub_factor=1, wanted_rows=None):
        """The surface meshes of the rows with wanted_rows[row] != 0 (uint8, one per row of the last extraction; None = every
        row, background included) on vol[::s, ::s, ::s].  Returns (cells u32[C] (rows), vertex_offsets u64[C+1],
        triangle_offsets u64[C+1], corners u64[V] (C-order index on the corner grid of dims ceil(n / s) + 1), triangles
        u32[T, 3], triangle_cell u32[T] (rows), triangle_neighbor u32[T] (rows, MESH_OUTSIDE at the border), device ms)."""
        keep = None
        if wanted_rows is not None:
            keep = np.ascontiguousarray(wanted_rows, dtype=np.uint8)
            if keep.size != self._max_label + 1:
                raise ValueError("wanted_rows has %d entries, the extraction %d rows" % (keep.size, self._max_label + 1))
        _check(self._lib.ta_mesh_extract(self._h, int(sub_factor), None if keep is None else keep.ctypes.data))
        C, V, T = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self._lib.ta_mesh_size(self._h, ctypes.byref(C), ctypes.byref(V), ctypes.byref(T)))
        C, V, T = C.value, V.value, T.value
        cells = np.zeros(C, dtype=np.uint32)
        voff, toff = np.zeros(C + 1, dtype=np.uint64), np.zeros(C + 1, dtype=np.uint64)
        corners = np.zeros(V, dtype=np.uint64)
        tri = np.zeros((T, 3), dtype=np.uint32)
        tcell, tnb = np.zeros(T, dtype=np.uint32), np.zeros(T, dtype=np.uint32)
        _check(self._lib.ta_mesh_get(self._h, cells.ctypes.data, voff.ctypes.data, toff.ctypes.data, corners.ctypes.data,
                                     tri.ctypes.data, tcell.ctypes.data, tnb.ctypes.data))
        return cells, voff, toff, corners, tri, tcell, tnb, self.mesh_timing()

    def mesh_timing(self):
        return self._doubles(self._lib.ta_mesh_timing, 1)[0]

    # -- label overlap with a second label volume (include/tissue_scan_overlap.h)
    def set_overlap(self, array):
        """Upload the second label volume B (uint16 / uint32, the label volume's shape).  One stored in another axis permutation
        than the labels is copied into the labels' layout first."""
        a = np.asarray(array)
        if a.dtype not in (np.uint16, np.uint32):
            raise TypeError("label volumes must be uint16 or uint32, not %s" % a.dtype)
        a = self._in_label_layout(a, ("the one it is compared with", "second volume's"))
        _check(self._lib.ta_overlap_set(self._h, ctypes.c_void_p(a.ctypes.data), a.dtype.itemsize, _i64x3(a.shape), _i64x3(a.strides)))
        self._keep_overlap = None

    def set_overlap_device(self, dev_ptr, itemsize, keep=None):
        """Adopt a device-resident B: dense C order with the label volume's buffer dims (halo plane included)."""
        _check(self._lib.ta_overlap_set_device(self._h, ctypes.c_void_p(int(dev_ptr)), int(itemsize)))
        self._keep_overlap = keep

    def set_overlap_capacity(self, log2_slots=0):
        """log2 of the slots the pass's device hash table starts with (0 = automatic); a table that is too small is grown."""
        _check(self._lib.ta_overlap_set_capacity(self._h, int(log2_slots)))

    def overlap_extract(self):
        """Enqueue the overlap pass over the label volume and B."""
        _check(self._lib.ta_overlap_extract(self._h))

    def overlap_size(self):
        n = ctypes.c_uint64(0)
        _check(self._lib.ta_overlap_size(self._h, ctypes.byref(n)))
        return int(n.value)

    def overlap_get(self):
        """(a u32[P], b u32[P], n u64[P]): the voxels n with label a in the volume and b in B, sorted by (a, b)."""
        P = self.overlap_size()
        a, b = np.zeros(P, dtype=np.uint32), np.zeros(P, dtype=np.uint32)
        n = np.zeros(P, dtype=np.uint64)
        _check(self._lib.ta_overlap_get(self._h, a.ctypes.data, b.ctypes.data, n.ctypes.data))
        return a, b, n

    def overlap_debug(self):
        """Diagnostics of the last run of the overlap pass kernel: records that missed a workgroup's LDS table (spills), the runs
        it took (passes) and the launch plan (tiles_per_group, groups).  Settles the table."""
        out = self._debug_words(self._lib.ta_overlap_debug)
        return dict(spills=out[0], passes=out[1], tiles_per_group=out[2], groups=out[3])

    def overlap_timing(self):
        """Milliseconds of the pass kernel of the last overlap_extract."""
        return self._doubles(self._lib.ta_overlap_timing, 1)[0]

    def overlap_timing_compaction(self):
        """(milliseconds of compaction + sort of the settled table, runs of the pass kernel it took)."""
        passes = ctypes.c_int(0)
        ms, = self._doubles(self._lib.ta_overlap_timing_compaction, 1, ctypes.byref(passes))
        return ms, int(passes.value)

    # -- cell junctions (include/tissue_scan_junctions.h)
    def junctions_extract(self):
        """Enqueue the counting walk over the 2 x 2 x 2 blocks of the label volume."""
        _check(self._lib.ta_junctions_extract(self._h))

    def junctions_size(self):
        """(rows of the edge table, rows of the vertex table, blocks of five labels or more); settles the tables."""
        e, v, d = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self._lib.ta_junctions_size(self._h, ctypes.byref(e), ctypes.byref(v), ctypes.byref(d)))
        return int(e.value), int(v.value), int(d.value)

    def junctions_get(self):
        """((labels u32[E, 3], n u64[E], sums u64[E, 3]), the same with [V, 4] labels for the vertices, degenerate): rows sorted by
        their labels, sums of the doubled block centres in array-axis order."""
        E, V, degenerate = self.junctions_size()
        el, en, es = np.zeros((E, 3), dtype=np.uint32), np.zeros(E, dtype=np.uint64), np.zeros((E, 3), dtype=np.uint64)
        vl, vn, vs = np.zeros((V, 4), dtype=np.uint32), np.zeros(V, dtype=np.uint64), np.zeros((V, 3), dtype=np.uint64)
        _check(self._lib.ta_junctions_get_edges(self._h, el.ctypes.data, en.ctypes.data, es.ctypes.data))
        _check(self._lib.ta_junctions_get_vertices(self._h, vl.ctypes.data, vn.ctypes.data, vs.ctypes.data))
        return (el, en, es), (vl, vn, vs), degenerate

    def junctions_timing(self):
        """(milliseconds of the two walks over the volume, milliseconds of everything after them) of settled tables."""
        return self._doubles(self._lib.ta_junctions_timing, 2)

    def junctions_debug(self):
        """What the last pass launched: the tasks of a walk, and the workgroups of the kernel that writes the sort keys of the edge
        and of the vertex records (0 without records).  Settles the tables."""
        out = self._debug_words(self._lib.ta_junctions_debug)
        return dict(tasks=out[0], edge_key_groups=out[1], vertex_key_groups=out[2])

    # -- wall geometry (include/tissue_scan_wallgeo.h)
    def wallgeo_extract(self):
        """Enqueue the wall-geometry pass over the current extraction (which needs its adjacency)."""
        _check(self._lib.ta_wallgeo_extract(self._h))

    def wallgeo_get(self):
        """(fwd u64[P, 3], rev u64[P, 3], sum1 u64[P, 3], sum2 u64[P, 6]), rows as adjacency(), array axes."""
        P = self.adjacency_size()
        fwd, rev, s1 = np.zeros((P, 3), dtype=np.uint64), np.zeros((P, 3), dtype=np.uint64), np.zeros((P, 3), dtype=np.uint64)
        s2 = np.zeros((P, 6), dtype=np.uint64)
        _check(self._lib.ta_wallgeo_get(self._h, fwd.ctypes.data, rev.ctypes.data, s1.ctypes.data, s2.ctypes.data))
        return fwd, rev, s1, s2

    def wallgeo_spills(self):
        """Records of the last pass that missed a workgroup's LDS table and went to the global rows directly."""
        n = ctypes.c_uint32(0)
        _check(self._lib.ta_wallgeo_spills(self._h, ctypes.byref(n)))
        return int(n.value)

    def wallgeo_debug(self):
        """wallgeo_spills() and the launch plan (tiles_per_group, groups; 0 and 0 when there was no pair and no launch)."""
        out = self._debug_words(self._lib.ta_wallgeo_debug)
        return dict(spills=out[0], tiles_per_group=out[2], groups=out[3])

    def wallgeo_timing(self):
        return self._doubles(self._lib.ta_wallgeo_timing, 1)[0]

    # -- connected components of the labels (include/tissue_scan_components.h)
    def components_extract(self):
        """Enqueue the union-find over the label volume, up to the count of its components."""
        _check(self._lib.ta_components_extract(self._h))

    def components_size(self):
        """Rows of the component table; settles it."""
        n = ctypes.c_uint64(0)
        _check(self._lib.ta_components_size(self._h, ctypes.byref(n)))
        return int(n.value)

    def components_get(self):
        """(label u32[R], n u64[R], first i32[R, 3], bbox i32[R, 6], sum1 u64[R, 3]): one row per component, sorted by
        (label, first), coordinates in array axes."""
        R = self.components_size()
        label, n = np.zeros(R, dtype=np.uint32), np.zeros(R, dtype=np.uint64)
        first, bbox = np.zeros((R, 3), dtype=np.int32), np.zeros((R, 6), dtype=np.int32)
        sum1 = np.zeros((R, 3), dtype=np.uint64)
        _check(self._lib.ta_components_get(self._h, label.ctypes.data, n.ctypes.data, first.ctypes.data, bbox.ctypes.data, sum1.ctypes.data))
        return label, n, first, bbox, sum1

    def components_image(self, first_plane=0, nplanes=None):
        """uint32 rows of the voxels of `nplanes` buffer planes from `first_plane` along memory axis 0 (None: all that follow), flat
        and in memory order; COMPONENT_NONE where the voxel's component has no row."""
        nplanes, count = self._plane_range(first_plane, nplanes)
        out = np.zeros(count, dtype=np.uint32)
        _check(self._lib.ta_components_image(self._h, int(first_plane), nplanes, out.ctypes.data))
        return out

    def components_relabel(self, new_label):
        """In place on the resident volume: every voxel of row r becomes new_label[r] (host uint32 table, one entry per row)."""
        new_label = np.ascontiguousarray(new_label, dtype=np.uint32)
        _check(self._lib.ta_components_relabel(self._h, ctypes.c_void_p(new_label.ctypes.data), int(new_label.size)))

    def components_timing(self):
        """(milliseconds of the kernels that walk the volume, milliseconds of everything after them) of a settled table."""
        return self._doubles(self._lib.ta_components_timing, 2)

    def components_debug(self):
        """What the last pass launched: the tiles of the local pass, the workgroups of the seam pass, of the last image or relabel
        launch since the extract (0 if none) and of the key kernel.  Settles the table."""
        out = self._debug_words(self._lib.ta_components_debug)
        return dict(tiles=out[0], seam_groups=out[1], stream_groups=out[2], key_groups=out[3])

    # -- distance maps (include/tissue_scan_distance.h)
    def distance_extract(self, mode=DIST_OWN_WALL, site_label=0, spacing=(1.0, 1.0, 1.0), flags=0):
        """Enqueue the three passes of the exact squared distance transform over the current extraction, and its table.  spacing
        in array-axis order; site_label (an id) is read with DIST_FROM_LABEL only."""
        _check(self._lib.ta_distance_extract(self._h, int(mode), int(site_label) & 0xFFFFFFFF, _spacing(spacing), int(flags)))

    def distance_get(self):
        """(min2 f64[R], max2 f64[R], pole i32[R, 3]), rows as labels(); +inf, +inf, (-1, -1, -1) for a row without voxels."""
        R = getattr(self, "_max_label", 0) + 1          # (no extraction yet: the library answers TA_EINVAL)
        min2, max2 = np.zeros(R, dtype=np.float64), np.zeros(R, dtype=np.float64)
        pole = np.zeros((R, 3), dtype=np.int32)
        _check(self._lib.ta_distance_get(self._h, min2.ctypes.data, max2.ctypes.data, pole.ctypes.data))
        return min2, max2, pole

    def distance_image(self, first_plane=0, nplanes=None):
        """float64 squared distances of the voxels of `nplanes` buffer planes from `first_plane` along memory axis 0 (None: all that
        follow), flat and in memory order."""
        nplanes, count = self._plane_range(first_plane, nplanes)
        out = np.zeros(count, dtype=np.float64)
        _check(self._lib.ta_distance_image(self._h, int(first_plane), nplanes, out.ctypes.data))
        return out

    def distance_timing(self):
        """(milliseconds of the row pass and the two column passes, milliseconds of the table passes)."""
        return self._doubles(self._lib.ta_distance_timing, 2)

    def distance_set_batch(self, columns=0):
        """Columns a launch of a column pass takes (0 = automatic); the results do not depend on it."""
        _check(self._lib.ta_distance_set_batch(self._h, int(columns)))

    def distance_debug(self):
        """What the last distance_extract launched: the workgroups of the row pass, of the extremes and pole kernels and of the
        table initialisation, and the launches of the column kernel along both axes together."""
        out = self._debug_words(self._lib.ta_distance_debug)
        return dict(row_groups=out[0], voxel_groups=out[1], init_groups=out[2], column_launches=out[3])

    # -- nearest-label maps (include/tissue_scan_nearest.h)
    def nearest_extract(self, empty_label=0, not_from_label=None, spacing=(1.0, 1.0, 1.0), max_d2=float("inf")):
        """Enqueue the three passes of the exact nearest-label transform over the current extraction, and the counts of the voxels
        every label gains: the voxels of `empty_label` (an id) are filled from all others, those of `not_from_label` (an id, None =
        nothing excluded) are neither sites nor filled; an empty voxel is filled when its squared distance is <= max_d2.  spacing
        in array-axis order."""
        flags = 0 if not_from_label is None else NEAREST_NOT_FROM
        _check(self._lib.ta_nearest_extract(self._h, int(empty_label) & 0xFFFFFFFF, int(not_from_label or 0) & 0xFFFFFFFF,
                                            _spacing(spacing), float(max_d2), flags))

    def nearest_get(self):
        """(gained u64[R], filled voxels, empty voxels left unfilled), rows as labels()."""
        gained = np.zeros(getattr(self, "_max_label", 0) + 1, dtype=np.uint64)          # (no extraction yet: the library answers TA_EINVAL)
        totals = np.zeros(2, dtype=np.uint64)
        _check(self._lib.ta_nearest_get(self._h, gained.ctypes.data, totals.ctypes.data))
        return gained, int(totals[0]), int(totals[1])

    def nearest_image(self, first_plane=0, nplanes=None, nearest=True, d2=True):
        """(uint32 nearest labels (ids; NEAREST_NONE without a site), float64 squared distances) of the voxels of `nplanes` buffer
        planes from `first_plane` along memory axis 0 (None: all that follow), flat and in memory order; None for the one not asked
        for."""
        nplanes, count = self._plane_range(first_plane, nplanes)
        n = np.zeros(count, dtype=np.uint32) if nearest else None
        d = np.zeros(count, dtype=np.float64) if d2 else None
        _check(self._lib.ta_nearest_image(self._h, int(first_plane), nplanes, None if n is None else n.ctypes.data,
                                          None if d is None else d.ctypes.data))
        return n, d

    def nearest_apply(self):
        """In place on the resident volume: every filled voxel takes its nearest label.  Every table is stale afterwards."""
        _check(self._lib.ta_nearest_apply(self._h))

    def nearest_timing(self):
        """(milliseconds of the row pass and the two column passes, milliseconds of the counting pass)."""
        return self._doubles(self._lib.ta_nearest_timing, 2)

    def nearest_set_batch(self, columns=0):
        """Columns a launch of a column pass takes (0 = automatic); the results do not depend on it."""
        _check(self._lib.ta_nearest_set_batch(self._h, int(columns)))

    def nearest_debug(self):
        """What the last nearest_extract launched: the workgroups of the row pass, of the counting pass and of the apply pass, and
        the launches of the column kernel along both axes together."""
        out = self._debug_words(self._lib.ta_nearest_debug)
        return dict(row_groups=out[0], count_groups=out[1], apply_groups=out[2], column_launches=out[3])

    # -- distance-shell profiles (include/tissue_scan_profile.h)
    def profile_extract(self, edges2, signal=False):
        """Enqueue the profile pass over the current distance map: edges2 = K + 1 ascending SQUARED distances (float64); with
        `signal` also the statistics of the signal image of the context."""
        e = np.ascontiguousarray(edges2, dtype=np.float64).reshape(-1)
        _check(self._lib.ta_profile_extract(self._h, int(e.size) - 1, e.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                            PROF_SIGNAL if signal else 0))
        self._profile_shape = (self._max_label + 1, int(e.size) - 1, bool(signal))

    def profile_get(self):
        """(n u64[R, K], sum u64[R, K], sumsq u64[R, K, 2] (lo, hi words), min u32[R, K], max u32[R, K]), rows as labels(); the
        four signal columns are None for a pass without signal."""
        R, K, signal = getattr(self, "_profile_shape", (1, 1, False))        # (no pass yet: the library answers TA_EINVAL)
        n = np.zeros((R, K), dtype=np.uint64)
        if not signal:
            _check(self._lib.ta_profile_get(self._h, n.ctypes.data, None, None, None, None))
            return n, None, None, None, None
        s, q = np.zeros((R, K), dtype=np.uint64), np.zeros((R, K, 2), dtype=np.uint64)
        mn, mx = np.zeros((R, K), dtype=np.uint32), np.zeros((R, K), dtype=np.uint32)
        _check(self._lib.ta_profile_get(self._h, n.ctypes.data, s.ctypes.data, q.ctypes.data, mn.ctypes.data, mx.ctypes.data))
        return n, s, q, mn, mx

    def profile_debug(self):
        """Diagnostics of the last profile pass: records that missed a workgroup's LDS table (spills) and the launch plan
        (tiles_per_group, groups)."""
        out = self._debug_words(self._lib.ta_profile_debug)
        return dict(spills=out[0], tiles_per_group=out[2], groups=out[3])

    def profile_timing(self):
        return self._doubles(self._lib.ta_profile_timing, 1)[0]

    # -- signal histograms and order statistics (include/tissue_scan_sighist.h)
    def sighist_extract(self, log2_width):
        """Enqueue the histogram pass over the current extraction: bin = S >> log2_width, 2^(bits - log2_width) <= 256 bins."""
        _check(self._lib.ta_sighist_extract(self._h, int(log2_width)))
        self._sighist_shape = (self._max_label + 1, 1 << (8 * self._signal_itemsize - int(log2_width)))

    def sighist_get(self):
        """counts u64[R, B], rows as labels()."""
        counts = np.zeros(getattr(self, "_sighist_shape", (1, 1)), dtype=np.uint64)      # (no pass yet: the library answers TA_EINVAL)
        _check(self._lib.ta_sighist_get(self._h, counts.ctypes.data))
        return counts

    def sigrank_extract(self, ranks):
        """Enqueue the radix select over the current extraction: ranks u64[R, n] (n <= SIGRANK_MAX_RANKS), 0-based, per row of
        labels(); a rank at or above the row's voxels (conventionally 2^64 - 1) gives SIGRANK_NONE."""
        r = np.ascontiguousarray(ranks, dtype=np.uint64)
        rows = getattr(self, "_max_label", None)               # (no extraction yet: the library answers TA_EINVAL)
        if r.ndim != 2 or (rows is not None and r.shape[0] != rows + 1):
            raise ValueError("ranks must be [%s, n], not %s" % ("rows" if rows is None else rows + 1, r.shape))
        _check(self._lib.ta_sigrank_extract(self._h, int(r.shape[1]), r.ctypes.data))
        self._sigrank_shape = r.shape

    def sigrank_get(self):
        """values u32[R, n]: the order statistics, SIGRANK_NONE where the rank was not below the row's voxels."""
        values = np.zeros(getattr(self, "_sigrank_shape", (1, 1)), dtype=np.uint32)
        _check(self._lib.ta_sigrank_get(self._h, values.ctypes.data))
        return values

    def sighist_debug(self):
        """Diagnostics of the last digit-kernel launch of either pass: counts that missed a workgroup's LDS table (spills) and the
        launch plan (tiles_per_group, groups)."""
        out = self._debug_words(self._lib.ta_sighist_debug)
        return dict(spills=out[0], tiles_per_group=out[2], groups=out[3])

    def sighist_timing(self):
        """(ms_hist, ms_rank): HIP-event milliseconds of the last histogram pass and of all kernels of the last select; None for
        one without valid results."""
        a, b = self._doubles(self._lib.ta_sighist_timing, 2)
        some = lambda v: None if v != v else v
        return some(a), some(b)

    # -- signal-weighted moments (include/tissue_scan_sigmoments.h)
    def sigmom_extract(self):
        """Enqueue the signal-moment pass over the current extraction and the signal image of the context."""
        _check(self._lib.ta_sigmom_extract(self._h))
        self._sigmom_rows = self._max_label + 1

    def sigmom_rows(self):
        """(n u64[R], w u64[R], m1 u64[R, 3], m2 u64[R, 6, 2] (lo, hi words)), rows as labels(); MEMORY-axis order, axis 0 counted
        from the first owned plane of the buffer (`memory_axes()` has the array axis of each)."""
        R = getattr(self, "_sigmom_rows", 1)                   # (no pass yet: the library answers TA_EINVAL)
        n, w = np.zeros(R, dtype=np.uint64), np.zeros(R, dtype=np.uint64)
        m1, m2 = np.zeros((R, 3), dtype=np.uint64), np.zeros((R, 6, 2), dtype=np.uint64)
        _check(self._lib.ta_sigmom_get(self._h, n.ctypes.data, w.ctypes.data, m1.ctypes.data, m2.ctypes.data))
        return n, w, m1, m2

    def sigmom_debug(self):
        """Diagnostics of the last signal-moment pass: records that missed a workgroup's LDS table (spills) and the launch plan
        (tiles_per_group, groups)."""
        out = self._debug_words(self._lib.ta_sigmom_debug)
        return dict(spills=out[0], tiles_per_group=out[2], groups=out[3])

    def sigmom_timing(self):
        return self._doubles(self._lib.ta_sigmom_timing, 1)[0]

    # -- two-channel statistics (include/tissue_scan_cosignal.h): channel A is the signal image, channel B is set here
    def set_cosignal(self, array):
        """Upload channel B: a uint8 / uint16 intensity image of the label volume's shape.  One stored in another axis permutation
        than the labels is copied into the labels' layout first."""
        a = np.asarray(array)
        if a.dtype not in SIGNAL_DTYPES:
            raise TypeError("signal images must be uint8 or uint16, not %s" % a.dtype)
        a = self._in_label_layout(a, ("its second signal", "second signal's"))
        _check(self._lib.ta_cosignal_set(self._h, ctypes.c_void_p(a.ctypes.data), a.dtype.itemsize, _i64x3(a.shape), _i64x3(a.strides)))
        self._keep_cosig = None

    def set_cosignal_device(self, dev_ptr, itemsize, keep=None):
        """Adopt a device-resident channel B: dense C order with the label volume's buffer dims (halo plane included)."""
        _check(self._lib.ta_cosignal_set_device(self._h, ctypes.c_void_p(int(dev_ptr)), int(itemsize)))
        self._keep_cosig = keep

    def cosignal_extract(self, thr_a=0, thr_b=0):
        """Enqueue the two-channel pass over the current extraction, the signal image (A) and channel B; a voxel is over in a
        channel when its value is > the threshold."""
        _check(self._lib.ta_cosignal_extract(self._h, int(thr_a), int(thr_b)))
        self._cosig_rows = self._max_label + 1

    def cosignal_rows(self):
        """A dict of COSIGNAL_COLUMNS, rows as labels(): uint64 [R], the three sq_* columns uint64 [R, 2] (lo, hi words)."""
        R = getattr(self, "_cosig_rows", 1)                    # (no pass yet: the library answers TA_EINVAL)
        cols = dict((k, np.zeros((R, 2) if k.startswith("sq_") else R, dtype=np.uint64)) for k in COSIGNAL_COLUMNS)
        _check(self._lib.ta_cosignal_get(self._h, *[cols[k].ctypes.data for k in COSIGNAL_COLUMNS]))
        return cols

    def cosignal_debug(self):
        """Diagnostics of the last two-channel pass: records that missed a workgroup's LDS table (spills) and the launch plan
        (tiles_per_group, groups)."""
        out = self._debug_words(self._lib.ta_cosignal_debug)
        return dict(spills=out[0], tiles_per_group=out[2], groups=out[3])

    def cosignal_timing(self):
        return self._doubles(self._lib.ta_cosignal_timing, 1)[0]

    def cosignal_thresholds(self):
        """(thr_a, thr_b) of the last two-channel pass."""
        a, b = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(self._lib.ta_cosignal_thresholds(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    # -- Euler numbers (include/tissue_scan_topology.h)
    def topology_extract(self):
        """Enqueue the pass over the 2 x 2 x 2 blocks of the resident volume, for the rows of the current extraction."""
        _check(self._lib.ta_topology_extract(self._h))
        self._topology_rows = self._max_label + 1

    def topology_rows(self):
        """(n0 u64[R], n1 u64[R, 3], n2 u64[R, 3], n3 u64[R], v u64[R], e u64[R, 3]), rows as labels(); the per-axis columns in
        MEMORY-axis order (`memory_axes()` has the array axis of each)."""
        R = getattr(self, "_topology_rows", 1)                 # (no pass yet: the library answers TA_EINVAL)
        one, three = (lambda: np.zeros(R, dtype=np.uint64)), (lambda: np.zeros((R, 3), dtype=np.uint64))
        n0, n1, n2, n3, v, e = one(), three(), three(), one(), one(), three()
        _check(self._lib.ta_topology_get(self._h, n0.ctypes.data, n1.ctypes.data, n2.ctypes.data, n3.ctypes.data, v.ctypes.data,
                                         e.ctypes.data))
        return n0, n1, n2, n3, v, e

    def topology_debug(self):
        """Diagnostics of the last pass: records that missed a workgroup's LDS table (spills), blocks of more than one label
        (mixed, saturating) and the launch plan (tiles_per_group, groups)."""
        out = self._debug_words(self._lib.ta_topology_debug)
        return dict(spills=out[0], mixed=out[1], tiles_per_group=out[2], groups=out[3])

    def topology_timing(self):
        return self._doubles(self._lib.ta_topology_timing, 1)[0]

    # -- resampling a second volume onto the label grid (include/tissue_scan_resample.h)
    def set_resample_source(self, array):
        """Upload the source volume (uint8 / uint16 / uint32, any 3-D shape, any dense axis permutation)."""
        a = np.asarray(array)
        if a.ndim != 3:
            raise ValueError("a 3D source volume is required")
        if a.dtype not in RESAMPLE_DTYPES:
            raise TypeError("source volumes must be uint8, uint16 or uint32, not %s" % a.dtype)
        if not _dense_permuted(a):
            a = np.ascontiguousarray(a)
        _check(self._lib.ta_resample_set_source(self._h, ctypes.c_void_p(a.ctypes.data), a.dtype.itemsize, _i64x3(a.shape), _i64x3(a.strides)))
        self._keep_resample_source = None
        self._resample_itemsize = a.dtype.itemsize

    def set_resample_source_device(self, dev_ptr, itemsize, dims, keep=None):
        """Adopt a device-resident source: dense C order with `dims`."""
        _check(self._lib.ta_resample_set_source_device(self._h, ctypes.c_void_p(int(dev_ptr)), int(itemsize), _i64x3(dims)))
        self._keep_resample_source = keep
        self._resample_itemsize = int(itemsize)

    def resample_extract(self, matrix, mode=RS_NEAREST, fill=0):
        """Enqueue the gather pass: `matrix` is the 3 x 4 index matrix (target voxel index -> continuous source index)."""
        m = np.ascontiguousarray(matrix, dtype=np.float64)
        if m.shape != (3, 4):
            raise ValueError("the index matrix must be 3 x 4, not %s" % (m.shape,))
        _check(self._lib.ta_resample_extract(self._h, m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(mode), int(fill) & 0xFFFFFFFF))

    def resample_get(self, first_plane=0, nplanes=None):
        """The voxels of `nplanes` buffer planes of the result from `first_plane` along memory axis 0 (None: all that follow), flat
        and in memory order, in the source's dtype."""
        nplanes, count = self._plane_range(first_plane, nplanes)
        _, itemsize = self.resample_device()
        out = np.zeros(count, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32}[itemsize])
        _check(self._lib.ta_resample_get(self._h, out.ctypes.data, int(first_plane), nplanes))
        return out

    def resample_device(self):
        """(device pointer, itemsize) of the result; the context owns the buffer."""
        p, n = ctypes.c_void_p(), ctypes.c_int(0)
        _check(self._lib.ta_resample_device(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, int(n.value)

    def resample_outside(self):
        """Owned target voxels of the last pass that received `fill`."""
        n = ctypes.c_uint64(0)
        _check(self._lib.ta_resample_outside(self._h, ctypes.byref(n)))
        return int(n.value)

    def resample_timing(self):
        return self._doubles(self._lib.ta_resample_timing, 1)[0]

    def resample_debug(self):
        """What the last pass launched: whole 16-byte strips or scalar stores (vector), the mode, the launch plan."""
        out = self._debug_words(self._lib.ta_resample_debug)
        return dict(vector=bool(out[0]), mode=out[1], tiles_per_group=out[2], groups=out[3])

    def resample_as_overlap(self):
        """Hand the result to the overlap pass as its B (a nearest-neighbour result of uint16 / uint32)."""
        _check(self._lib.ta_resample_as_overlap(self._h))
        self._keep_overlap = None

    def resample_as_signal(self):
        """Hand the result to the signal passes (uint8 / uint16)."""
        _check(self._lib.ta_resample_as_signal(self._h))
        self._keep_sig = None
        self._signal_itemsize = self.resample_device()[1]

    # -- oriented extents (include/tissue_scan_extents.h)
    def extents_extract(self, weights):
        """Enqueue the extent pass over the current extraction: weights f64[R, 3, 3], per row of labels() three directions k with
        one weight per MEMORY axis d (unit direction times voxel size; `memory_axes()` has the array axis of each d)."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim != 3 or w.shape[1:] != (3, 3):
            raise ValueError("weights must be [rows, 3, 3], not %s" % (w.shape,))
        _check(self._lib.ta_extents_extract(self._h, w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(w.shape[0])))
        self._extent_rows = int(w.shape[0])

    def extents_rows(self):
        """(lo f64[R, 3], hi f64[R, 3]): the smallest and the largest projection of every row's voxels per direction, +inf and
        -inf for a row without voxels."""
        R = getattr(self, "_extent_rows", 1)                   # (no pass yet: the library answers TA_EINVAL)
        lo, hi = np.zeros((R, 3), dtype=np.float64), np.zeros((R, 3), dtype=np.float64)
        _check(self._lib.ta_extents_get(self._h, lo.ctypes.data, hi.ctypes.data))
        return lo, hi

    def extents_debug(self):
        """Diagnostics of the last extent pass: records that missed a workgroup's LDS table (spills) and the launch plan
        (tiles_per_group, groups)."""
        out = self._debug_words(self._lib.ta_extents_debug)
        return dict(spills=out[0], tiles_per_group=out[2], groups=out[3])

    def extents_timing(self):
        return self._doubles(self._lib.ta_extents_timing, 1)[0]

    def memory_axes(self):
        """perm[k] = the array axis of memory axis k of the resident volume (slowest first), as the library orders them."""
        return self._memory_axes

    def max_label(self):
        v = ctypes.c_uint32(0)
        _check(self._lib.ta_volume_max_label(self._h, ctypes.byref(v)))
        return v.value

    # -- sparse label ids
    def label_census(self):
        """(max id, ascending uint32 ids present in the resident volume): np.unique on the device."""
        top, n = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(self._lib.ta_volume_label_census(self._h, ctypes.byref(top), ctypes.byref(n)))
        return top.value, self._census_ids(n.value)

    def compact_labels(self, ids=None):
        """From now on the sweep reads a copy of the volume written in the RANKS of its ids (`ids`: an ascending unique list
        that covers the volume, e.g. the union over the slabs of a partitioned volume; None = this volume's own census).
        Returns the rank -> id table (uint32): rows of `labels()` are ranks, `adjacency()` answers in ids."""
        n = ctypes.c_uint32(0)
        if ids is None:
            _check(self._lib.ta_volume_compact_labels(self._h, None, 0, ctypes.byref(n)))
        else:
            ids = np.ascontiguousarray(ids, dtype=np.uint32)
            _check(self._lib.ta_volume_compact_labels(self._h, ids.ctypes.data_as(ctypes.c_void_p), ids.size, ctypes.byref(n)))
        return self._census_ids(n.value)

    def is_compact(self):
        flag, n = ctypes.c_int(0), ctypes.c_uint32(0)
        _check(self._lib.ta_volume_is_compact(self._h, ctypes.byref(flag), ctypes.byref(n)))
        return bool(flag.value)

    def compact_ids(self):
        """The rank -> id table of a compacted context (uint32, ascending)."""
        flag, n = ctypes.c_int(0), ctypes.c_uint32(0)
        _check(self._lib.ta_volume_is_compact(self._h, ctypes.byref(flag), ctypes.byref(n)))
        if not flag.value:
            raise TissueScanError(TA_EINVAL, "the context is not compacted")
        return self._census_ids(n.value)

    # -- hot path
    def rerank(self):
        """Compaction is a SNAPSHOT of the voxels: after rewriting an adopted device buffer in place, refresh the rank copy the
        sweep reads (asynchronous; an id outside the census makes the next extraction's getters raise TA_ERANGE)."""
        _check(self._lib.ta_volume_rerank(self._h))

    def uncompact(self):
        """Back to dense rows 0 .. max_label (releases the rank copy)."""
        _check(self._lib.ta_volume_uncompact(self._h))

    def owned_planes(self):
        n = ctypes.c_int64(0)
        _check(self._lib.ta_volume_owned_planes(self._h, ctypes.byref(n)))
        return int(n.value)

    def plane_events(self):
        """uint64[owned planes]: label changes along the fast axis in every owned plane of the resident volume (the weight
        distributed.balanced_cuts balances)."""
        out = np.zeros(self.owned_planes(), dtype=np.uint64)      # (asked of the library: a size-1 axis moves the slowest MEMORY axis)
        _check(self._lib.ta_volume_plane_events(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def extract(self, features, max_label):
        _check(self._lib.ta_extract(self._h, feature_mask(features), int(max_label)))
        self._max_label = int(max_label)

    def labels(self):
        """(count u64[L+1], bbox i32[L+1,6], sum1 u64[L+1,3], sum2 u64[L+1,6])"""
        n = self._max_label + 1
        count = np.zeros(n, dtype=np.uint64)
        bbox = np.zeros((n, 6), dtype=np.int32)
        sum1 = np.zeros((n, 3), dtype=np.uint64)
        sum2 = np.zeros((n, 6), dtype=np.uint64)
        _check(self._lib.ta_get_labels(self._h, count.ctypes.data, bbox.ctypes.data, sum1.ctypes.data,
                                       sum2.ctypes.data))
        return count, bbox, sum1, sum2

    def adjacency_size(self):
        """Pair count of the last extraction (drains the stream, validates its flags)."""
        n = ctypes.c_int64(0)
        _check(self._lib.ta_adjacency_size(self._h, ctypes.byref(n)))
        return int(n.value)

    def adjacency_scope(self):
        """ADJ_LOCAL / ADJ_MERGED / ADJ_PARTIAL: which pairs the adjacency getters answer with right now."""
        scope = ctypes.c_int(0)
        _check(self._lib.ta_adjacency_scope(self._h, ctypes.byref(scope)))
        return scope.value

    def adjacency(self, allow_partial=False):
        """(lo u32[n], hi u32[n], faces u64[n,3]) sorted by (lo, hi).  After a pack_shared exchange the context holds
        only this rank's private pairs + the travelling pairs of all ranks: that list is handed out only when asked for
        by name (SlabJob.result_arrays assembles the global list from it)."""
        if not allow_partial and self.adjacency_scope() == ADJ_PARTIAL:
            raise TissueScanError(TA_EINVAL, "this context holds a PARTIAL pair list (private + travelling pairs of a "
                                             "slab exchange): use SlabJob.result_arrays() for the global list")
        n = ctypes.c_int64(0)
        _check(self._lib.ta_adjacency_size(self._h, ctypes.byref(n)))
        lo = np.zeros(n.value, dtype=np.uint32)
        hi = np.zeros(n.value, dtype=np.uint32)
        faces = np.zeros((n.value, 3), dtype=np.uint64)
        _check(self._lib.ta_adjacency_get(self._h, lo.ctypes.data, hi.ctypes.data, faces.ctypes.data))
        return lo, hi, faces

    def timing(self):
        nbytes = ctypes.c_uint64(0)
        a, b, t = self._doubles(self._lib.ta_timing, 3, ctypes.byref(nbytes))
        # (a duration no event recorded comes back as NaN -- TA_OPT_TIMING 0, or 1 for what only mode 2 brackets -- and is
        #  handed on as None: "not measured" must never read as "took no time" in a bandwidth figure)
        some = lambda v: None if v != v else v
        return dict(ms_sweep=some(a), ms_adjacency=some(b), ms_total=some(t), bytes_read=nbytes.value)

    def timing_series(self, capacity=4096):
        """Sweep-kernel milliseconds of the last extractions (oldest first; OPT_TIMING_RING of them at most)."""
        buf = (ctypes.c_double * int(capacity))()
        n = ctypes.c_int(0)
        _check(self._lib.ta_timing_series(self._h, buf, int(capacity), ctypes.byref(n)))
        return [buf[i] for i in range(n.value)]

    def read_probe(self, dev_ptr, nbytes, repeats=5):
        """Milliseconds of the fastest of `repeats` read-only streaming passes over a device buffer."""
        ms = ctypes.c_double(0.0)
        _check(self._lib.ta_read_probe(self._h, ctypes.c_void_p(int(dev_ptr)), int(nbytes), int(repeats), ctypes.byref(ms)))
        return ms.value

    def debug_counters(self):
        out = (ctypes.c_uint32 * 16)()
        _check(self._lib.ta_debug_counters(self._h, out))
        d = dict(range_flag=out[0], pair_overflow=out[1], label_spills=out[2], pair_spills=out[3])
        if any(out[8:16]):
            d["stamps"] = [int(v) for v in out[8:16]]
        return d

    # -- multi-GPU views
    def bind_accumulators(self, sums_ptr, boxes_ptr, max_label, keep=None):
        _check(self._lib.ta_bind_accumulators(self._h, ctypes.c_void_p(int(sums_ptr) if sums_ptr else 0),
                                              ctypes.c_void_p(int(boxes_ptr) if boxes_ptr else 0),
                                              int(max_label)))
        self._keep_acc = keep

    def accumulators_reduced(self):
        """The bound accumulators now hold other ranks' contributions (see include/tissue_scan.h)."""
        _check(self._lib.ta_accumulators_reduced(self._h))

    def adjacency_device(self):
        k, f, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(0)
        _check(self._lib.ta_adjacency_device(self._h, ctypes.byref(k), ctypes.byref(f), ctypes.byref(n)))
        return k.value, f.value, n.value

    def adjacency_export(self, keys_ptr, faces_ptr, capacity):
        _check(self._lib.ta_adjacency_export(self._h, ctypes.c_void_p(int(keys_ptr) if keys_ptr else 0),
                                             ctypes.c_void_p(int(faces_ptr) if faces_ptr else 0), int(capacity)))

    def adjacency_merge(self, keys_ptr, faces_ptr, npairs):
        _check(self._lib.ta_adjacency_merge(self._h, ctypes.c_void_p(int(keys_ptr) if keys_ptr else 0),
                                            ctypes.c_void_p(int(faces_ptr) if faces_ptr else 0), int(npairs)))

    def adjacency_pack(self, block_ptr, capacity):
        """Enqueue: write this rank's exchange block (exchange_words(capacity) uint64 words)."""
        _check(self._lib.ta_adjacency_pack(self._h, ctypes.c_void_p(int(block_ptr)), int(capacity)))

    def adjacency_pack_shared(self, block_ptr, capacity):
        """Enqueue: keep the pairs no other rank can hold (needs the REDUCED boxes), pack the rest."""
        _check(self._lib.ta_adjacency_pack_shared(self._h, ctypes.c_void_p(int(block_ptr)), int(capacity)))

    def adjacency_merge_blocks(self, blocks_ptr, nblocks, capacity):
        """Enqueue: rebuild the adjacency from all ranks' gathered exchange blocks."""
        _check(self._lib.ta_adjacency_merge_blocks(self._h, ctypes.c_void_p(int(blocks_ptr)), int(nblocks),
                                                   int(capacity)))

    # -- synthetic workload + raw memory
    def synth_voronoi(self, dev_ptr, dtype, dims, a_begin, a_count, seeds, grid, ell=None):
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        g = (ctypes.c_int32 * 3)(*[int(x) for x in grid])
        ell_arr = None if ell is None else np.ascontiguousarray(np.concatenate(ell), dtype=np.int64)
        _check(self._lib.ta_synth_voronoi(self._h, ctypes.c_void_p(int(dev_ptr)), np.dtype(dtype).itemsize,
                                          _i64x3(dims), int(a_begin), int(a_count), seeds.ctypes.data, g,
                                          None if ell_arr is None else ell_arr.ctypes.data))

    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        _check(self._lib.ta_device_malloc(self._h, int(nbytes), ctypes.byref(p)))
        return p.value

    def free(self, ptr):
        _check(self._lib.ta_device_free(self._h, ctypes.c_void_p(int(ptr))))

    def d2h(self, host_array, dev_ptr):
        _check(self._lib.ta_memcpy_d2h(self._h, host_array.ctypes.data, ctypes.c_void_p(int(dev_ptr)),
                                       host_array.nbytes))

    def h2d(self, dev_ptr, host_array):
        a = np.ascontiguousarray(host_array)
        _check(self._lib.ta_memcpy_h2d(self._h, ctypes.c_void_p(int(dev_ptr)), a.ctypes.data, a.nbytes))
