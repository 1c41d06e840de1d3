"""Connected components of the labels without a GPU: the NumPy / SciPy restatement (tests/components_reference.py) against
scipy.ndimage.label per label, and the host side -- `LabelComponents`, its slab merge, the analysis methods and the graph column
-- on tables injected as the device would deliver them."""
import numpy as np
import pytest
from scipy import ndimage

import components_reference as ref
from oracle import onepass
from tissue_analysis_amd import DICT, Extraction, LabelComponents, SpatialImage, SpatialImageAnalysis3D, _capi, synth
from tissue_analysis_amd.graph_from_image import graph_from_image

FACES = ndimage.generate_binary_structure(3, 1)


def as_components(rows, **kw):
    return LabelComponents(rows[0], rows[1], rows[2], rows[3], rows[4], **kw)


def same_table(got, want):
    """got: LabelComponents, want: rows of ref.table()."""
    for g, w in zip((got.label, got.n, got.first, got.bbox, got.sum1), want):
        assert g.shape == w.shape and np.array_equal(g, w)


def check_against_ndimage(V):
    rows, image = ref.table(V)
    label, n, first, bbox, sum1 = rows
    assert image.shape == V.shape and image.max() == label.size - 1
    total = 0
    for l in np.unique(V).tolist():
        blobs, k = ndimage.label(V == l, structure=FACES)
        at = np.flatnonzero(label == l)
        assert at.size == k                                                 # as many rows as scipy finds blobs
        total += k
        sets = set(frozenset(np.flatnonzero(blobs.reshape(-1) == b + 1).tolist()) for b in range(k))
        for r in at.tolist():
            mine = np.flatnonzero(image.reshape(-1) == r)
            assert frozenset(mine.tolist()) in sets                         # ... of the same voxels
            xyz = np.stack(np.unravel_index(mine, V.shape), axis=1)
            assert n[r] == mine.size and np.array_equal(first[r], xyz[0])
            assert np.array_equal(bbox[r], np.concatenate([xyz.min(axis=0), xyz.max(axis=0) + 1]))
            assert np.array_equal(sum1[r], xyz.sum(axis=0).astype(np.uint64))
    assert total == label.size
    assert np.array_equal(np.lexsort((first[:, 2], first[:, 1], first[:, 0], label)), np.arange(label.size))


def test_restatement_against_ndimage_label():
    check_against_ndimage(synth.voronoi_labels((30, 28, 36), 60, 3, dtype=np.uint16))
    rng = np.random.default_rng(11)
    check_against_ndimage(rng.integers(0, 3, size=(9, 10, 12)).astype(np.uint16))
    V = np.zeros((3, 3, 3), dtype=np.uint16)
    V[0, 0, 0] = V[1, 1, 0] = V[1, 1, 1] = 5                               # an edge contact, then a face contact
    rows, image = ref.table(V)
    assert rows[0].tolist() == [0, 5, 5] and rows[1].tolist() == [24, 1, 2]
    assert image[0, 0, 0] == 1 and image[1, 1, 0] == 2 and image[1, 1, 1] == 2


def test_the_synthetic_tissue_has_fragmented_labels():
    V = synth.voronoi_labels((64, 64, 64), 200, 3)
    cc = as_components(ref.table(V)[0])
    per = cc.per_label()
    assert len(per) == 156 and len(cc) == 243 and len(cc.fragmented()) == 28
    assert sum(per.values()) == 243 and int(cc.n.sum()) == V.size


def injected():
    # label 3: three blobs, the two largest tie at 5 voxels; label 9: one blob; label 4: two blobs
    label = [3, 3, 3, 4, 4, 9]
    n = [5, 2, 5, 1, 7, 4]
    first = [[0, 0, 0], [0, 4, 1], [2, 0, 0], [1, 1, 1], [1, 3, 0], [5, 5, 5]]
    bbox = [f + [f[0] + 1, f[1] + 1, f[2] + k] for f, k in zip(first, n)]
    sum1 = [[f[0] * k, f[1] * k, f[2] * k + k * (k - 1) // 2] for f, k in zip(first, n)]
    return LabelComponents(label, n, first, bbox, sum1, voxelsize=(0.5, 2.0, 1.0))


def test_label_components_on_an_injected_table():
    cc = injected()
    assert len(cc) == 6 and cc.label.dtype == np.int64 and cc.n.dtype == np.uint64 and cc.sum1.dtype == np.uint64
    assert cc.per_label() == {3: 3, 4: 2, 9: 1}
    assert cc.fragmented() == {3: 3, 4: 2} and cc.fragmented(exclude=(3,)) == {4: 2}
    assert cc.rows_of(3).tolist() == [0, 1, 2] and cc.rows_of(4).tolist() == [3, 4] and cc.rows_of(7).tolist() == []
    assert cc.largest().tolist() == [True, False, False, False, True, True]      # the tie goes to the smaller first
    assert cc.split_map().tolist() == [3, 10, 11, 12, 4, 9]
    assert cc.split_map(next_label=100).tolist() == [3, 100, 101, 102, 4, 9]
    assert cc.erase_map(3).tolist() == [3, 0, 3, 0, 4, 9]
    assert cc.erase_map(6, erase_value=1).tolist() == [3, 1, 1, 1, 4, 9]
    assert cc.erase_map(0).tolist() == cc.label.tolist()
    c = cc.centroid(real=False)
    assert np.array_equal(c[0], [0.0, 0.0, 2.0]) and np.array_equal(c[4], [1.0, 3.0, 3.0])
    assert np.array_equal(cc.centroid()[4], [0.5, 6.0, 3.0])
    assert np.array_equal(ref.split_labels(cc.label, cc.n), cc.split_map())
    assert np.array_equal(ref.erase_labels(cc.label, cc.n, 3), cc.erase_map(3))
    empty = LabelComponents([], [], [], [], [])
    assert len(empty) == 0 and empty.per_label() == {} and empty.largest().shape == (0,) and empty.split_map().shape == (0,)
    with pytest.raises(ValueError):
        LabelComponents([1, 2], [1], [[0, 0, 0]] * 2, [[0] * 6] * 2, [[0] * 3] * 2)
    with pytest.raises(ValueError):
        LabelComponents([1], [1], [[0, 0]], [[0] * 6], [[0] * 3])


def u_volume():
    """Voronoi cells, and a U of label 500 whose arms run along axis 0 through planes 2 .. 20 and are joined at plane 20 only: a cut
    below plane 20 leaves two rows in the lower slab that only the upper slab joins."""
    V = synth.voronoi_labels((24, 20, 30), 30, 3, dtype=np.uint16)
    V[2:21, 5, 4] = 500
    V[2:21, 5, 12] = 500
    V[20, 5, 4:13] = 500
    V[6:9, 15, 20:23] = 500                                                 # and a blob of the same label on its own
    return V


@pytest.mark.parametrize("cuts", [(11,), (7, 15), (3, 8, 13, 19)])
def test_merge_of_slab_tables_equals_the_whole(cuts):
    V = u_volume()
    whole, _ = ref.table(V)
    assert np.count_nonzero(whole[0] == 500) == 2
    parts, seams = ref.slabs(V, cuts)
    assert np.count_nonzero(parts[0][0] == 500) >= 2                        # the arms are apart in the lowest slab
    assert sum(p[0].size for p in parts) > whole[0].size
    merged = LabelComponents.merge([as_components(p) for p in parts], seams)
    same_table(merged, whole)
    with pytest.raises(ValueError):
        LabelComponents.merge([as_components(p) for p in parts], seams[:-1] if len(seams) > 1 else seams + seams)


def test_a_halo_only_component_has_no_row():
    V = np.ones((3, 4, 5), dtype=np.uint16)
    V[0, 1, 1] = 7                                                          # in the halo plane only
    V[0, 2, 2] = V[1, 2, 2] = 8                                             # reaches an owned plane
    rows, image = ref.table(V, first_owned=1, a0_origin=10)
    assert rows[0].tolist() == [1, 8] and rows[1].tolist() == [39, 1]
    assert image[0, 1, 1] == ref.NONE and image[0, 2, 2] == 1 and image[0, 0, 0] == 0
    assert rows[2][1].tolist() == [10, 2, 2] and rows[3][1].tolist() == [10, 2, 2, 11, 3, 3]


def analysis(V, **kw):
    x = Extraction.from_arrays(V.shape, onepass.extract(V))
    return SpatialImageAnalysis3D(SpatialImage(V, voxelsize=(0.5, 0.25, 2.0)), return_type=DICT, background=1, extraction=x, **kw)


def test_analysis_methods_and_graph_column_on_an_injected_table():
    V = synth.voronoi_labels((64, 64, 64), 200, 3)
    sia = analysis(V, ignoredlabels=0)
    want = as_components(ref.table(V)[0], voxelsize=(0.5, 0.25, 2.0))
    sia._components = want                                                  # as the device would deliver it
    assert sia.label_components() is want
    frag = sia.disconnected_labels()
    assert frag and set(frag) <= set(want.fragmented()) and not set(frag) & {0, 1}
    assert frag == dict((l, k) for l, k in want.fragmented().items() if l not in (0, 1))
    ids = [l for l in sia.labels()][:40]
    g = graph_from_image(sia, labels=list(ids), background=1, spatio_temporal_properties=['volume', 'n_components'])
    col = g.vertex_property('n_components')
    per = want.per_label()
    assert dict((int(l), int(k)) for l, k in col.items()) == dict((l, per[l]) for l in ids)
    assert max(col.values()) > 1
    g = graph_from_image(sia, labels=list(ids), background=1, spatio_temporal_properties=['volume'])
    assert 'n_components' not in list(g.vertex_property_names())


def test_null_context_is_rejected_without_a_gpu():
    lib = _capi.load()
    for name in _capi.COMPONENT_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.ta_components_extract(None) == _capi.TA_EINVAL
    assert b"NULL" in lib.ta_last_error()
    assert lib.ta_components_size(None, None) == _capi.TA_EINVAL
    assert lib.ta_components_get(None, None, None, None, None, None) == _capi.TA_EINVAL
    assert lib.ta_components_image(None, 0, 0, None) == _capi.TA_EINVAL
    assert lib.ta_components_relabel(None, None, 0) == _capi.TA_EINVAL
    assert lib.ta_components_timing(None, None, None) == _capi.TA_EINVAL
    assert lib.ta_components_debug(None, None) == _capi.TA_EINVAL
    assert lib.ta_version() == 5
