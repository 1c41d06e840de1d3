"""The decisions the Python layer makes in one place each, checked without a device: when a pass over the current extraction
sweeps first (`ResidentVolume.over_extraction`, driven here by a stub that has `.last` and `.extract` only), what a voxel size is
(`_tables.voxelsize3`), and which symbols `_capi` declares per header (its one table against the fourteen lists the binding had
when they were written out by hand)."""
import numpy as np
import pytest

from tissue_analysis_amd import _capi

EINVAL, ERANGE = _capi.TA_EINVAL, _capi.TA_ERANGE


class Swept(object):
    def __init__(self, sparse):
        self.sparse = sparse


class Stub(object):
    """What over_extraction may touch of a ResidentVolume: `.last` and `.extract`."""

    def __init__(self, last=None):
        self.last = last
        self.sweeps = []

    def extract(self, features=_capi.F_ALL, max_label=None, sparse=None):
        self.sweeps.append((features, max_label, sparse))
        self.last = Swept(bool(sparse))
        return self.last


def over_extraction(stub, enqueue):
    from tissue_analysis_amd.extraction import ResidentVolume
    return ResidentVolume.over_extraction(stub, enqueue)


def failing(codes):
    """An enqueue that raises TissueScanError(code) for every code of `codes` in turn (None: succeeds), and records its calls."""
    calls, codes = [], list(codes)

    def enqueue(x):
        calls.append(x)
        code = codes.pop(0) if codes else None
        if code is not None:
            raise _capi.TissueScanError(code, "call %d" % len(calls))
        return "value %d" % len(calls)
    return enqueue, calls


def test_a_current_extraction_is_not_swept_again():
    x0 = Swept(False)
    stub = Stub(x0)
    enqueue, calls = failing([])
    x, value = over_extraction(stub, enqueue)
    assert x is x0 and value == "value 1" and calls == [x0] and stub.sweeps == [] and stub.last is x0


def test_no_extraction_is_one_sweep_then_one_enqueue():
    stub = Stub(None)
    enqueue, calls = failing([])
    x, value = over_extraction(stub, enqueue)
    assert stub.sweeps == [(_capi.F_ALL, None, None)]
    assert x is stub.last and calls == [x] and value == "value 1"


@pytest.mark.parametrize("sparse", [True, False])
def test_a_stale_extraction_is_swept_with_the_same_sparse(sparse):
    x0 = Swept(sparse)
    stub = Stub(x0)
    enqueue, calls = failing([EINVAL])
    x, value = over_extraction(stub, enqueue)
    assert stub.sweeps == [(_capi.F_ALL, None, sparse)] and stub.sweeps[0][2] is sparse
    assert x is stub.last and x is not x0 and calls == [x0, x] and value == "value 2"


def test_a_second_einval_propagates_after_one_sweep():
    stub = Stub(Swept(False))
    enqueue, calls = failing([EINVAL, EINVAL])
    with pytest.raises(_capi.TissueScanError) as e:
        over_extraction(stub, enqueue)
    assert e.value.code == EINVAL and "call 2" in str(e.value) and len(calls) == 2 and len(stub.sweeps) == 1


def test_an_einval_after_the_first_sweep_propagates():
    stub = Stub(None)
    enqueue, calls = failing([EINVAL])
    with pytest.raises(_capi.TissueScanError) as e:
        over_extraction(stub, enqueue)
    assert e.value.code == EINVAL and len(calls) == 1 and len(stub.sweeps) == 1


def test_another_error_propagates_without_a_sweep():
    x0 = Swept(True)
    stub = Stub(x0)
    enqueue, calls = failing([ERANGE])
    with pytest.raises(_capi.TissueScanError) as e:
        over_extraction(stub, enqueue)
    assert e.value.code == ERANGE and calls == [x0] and stub.sweeps == [] and stub.last is x0


def test_voxelsize3():
    from tissue_analysis_amd._tables import voxelsize3
    assert voxelsize3((2, 3)) == (2.0, 3.0, 1.0) and voxelsize3((2, 3, 4)) == (2.0, 3.0, 4.0)
    assert voxelsize3(np.array([0.5, 2, 4])) == (0.5, 2.0, 4.0) and voxelsize3([2, 3]) == (2.0, 3.0, 1.0)
    assert all(type(v) is float for v in voxelsize3((2, 3)) + voxelsize3(np.array([1, 2, 3])))
    for bad in ((2,), (2, 3, 4, 5)):
        with pytest.raises(ValueError) as e:
            voxelsize3(bad)
        assert str(e.value) == "voxelsize must have two or three entries"


# the fourteen lists as the binding spelled them out before it had one table
DECLARED = {
    "SYMBOLS": (
        "ta_version", "ta_adjacency_scope", "ta_last_error", "ta_device_count", "ta_ctx_create", "ta_ctx_destroy",
        "ta_ctx_set_stream", "ta_ctx_set_option", "ta_ctx_get_option", "ta_ctx_synchronize", "ta_volume_set",
        "ta_volume_set_device", "ta_volume_max_label", "ta_volume_label_census", "ta_label_census_get", "ta_volume_compact_labels",
        "ta_volume_is_compact", "ta_volume_rerank", "ta_volume_uncompact", "ta_volume_owned_planes", "ta_volume_plane_events",
        "ta_volume_relabel", "ta_volume_get", "ta_volume_map",
        "ta_volume_first_layer", "ta_volume_hollow", "ta_volume_layer18", "ta_wall_voxels_count", "ta_wall_voxels_get",
        "ta_wall_voxels_get_by_pair", "ta_wall_medians", "ta_wall_medians_get",
        "ta_extract", "ta_get_labels",
        "ta_adjacency_size", "ta_adjacency_get", "ta_timing", "ta_timing_series", "ta_read_probe", "ta_debug_counters",
        "ta_bind_accumulators",
        "ta_accumulators_device", "ta_accumulators_reduced", "ta_adjacency_device", "ta_adjacency_export", "ta_adjacency_merge",
        "ta_adjacency_pack", "ta_adjacency_pack_shared", "ta_adjacency_merge_blocks", "ta_synth_voronoi",
        "ta_device_malloc", "ta_device_free", "ta_memcpy_d2h", "ta_memcpy_h2d",
    ),
    "SIGNAL_SYMBOLS": (
        "ta_signal_set", "ta_signal_set_device", "ta_signal_extract", "ta_signal_get_labels", "ta_signal_get_walls",
        "ta_signal_timing", "ta_signal_debug",
    ),
    "MESH_SYMBOLS": ("ta_mesh_extract", "ta_mesh_size", "ta_mesh_get", "ta_mesh_timing"),
    "OVERLAP_SYMBOLS": (
        "ta_overlap_set", "ta_overlap_set_device", "ta_overlap_set_capacity", "ta_overlap_extract", "ta_overlap_size",
        "ta_overlap_get", "ta_overlap_timing", "ta_overlap_timing_compaction", "ta_overlap_debug",
    ),
    "JUNCTION_SYMBOLS": (
        "ta_junctions_extract", "ta_junctions_size", "ta_junctions_get_edges", "ta_junctions_get_vertices", "ta_junctions_timing",
        "ta_junctions_debug",
    ),
    "WALLGEO_SYMBOLS": ("ta_wallgeo_extract", "ta_wallgeo_get", "ta_wallgeo_spills", "ta_wallgeo_debug", "ta_wallgeo_timing"),
    "COMPONENT_SYMBOLS": (
        "ta_components_extract", "ta_components_size", "ta_components_get", "ta_components_image", "ta_components_relabel",
        "ta_components_timing", "ta_components_debug",
    ),
    "DISTANCE_SYMBOLS": ("ta_distance_extract", "ta_distance_get", "ta_distance_image", "ta_distance_timing",
                         "ta_distance_set_batch", "ta_distance_debug"),
    "NEAREST_SYMBOLS": ("ta_nearest_extract", "ta_nearest_get", "ta_nearest_image", "ta_nearest_apply", "ta_nearest_timing",
                        "ta_nearest_debug", "ta_nearest_set_batch"),
    "PROFILE_SYMBOLS": ("ta_profile_extract", "ta_profile_get", "ta_profile_debug", "ta_profile_timing"),
    "SIGHIST_SYMBOLS": ("ta_sighist_extract", "ta_sighist_get", "ta_sigrank_extract", "ta_sigrank_get", "ta_sighist_debug",
                        "ta_sighist_timing"),
    "SIGMOM_SYMBOLS": ("ta_sigmom_extract", "ta_sigmom_get", "ta_sigmom_debug", "ta_sigmom_timing"),
    "TOPOLOGY_SYMBOLS": ("ta_topology_extract", "ta_topology_get", "ta_topology_debug", "ta_topology_timing"),
    "RESAMPLE_SYMBOLS": ("ta_resample_set_source", "ta_resample_set_source_device", "ta_resample_extract", "ta_resample_get",
                         "ta_resample_device", "ta_resample_outside", "ta_resample_timing", "ta_resample_debug",
                         "ta_resample_as_overlap", "ta_resample_as_signal"),
}


def test_every_symbol_tuple_is_what_it_was():
    assert len(DECLARED) == 14
    union = []
    for name, want in DECLARED.items():
        got = getattr(_capi, name)
        assert isinstance(got, tuple) and len(got) == len(want) and set(got) == set(want), name
        union += list(got)
    assert len(union) == len(set(union)) == sum(len(v) for v in DECLARED.values())


def test_every_declared_symbol_gets_its_signature():
    lib = _capi.load()
    for name in DECLARED:
        for symbol in getattr(_capi, name):
            fn = getattr(lib, symbol)
            assert fn.argtypes is not None and fn.restype is not None, symbol
