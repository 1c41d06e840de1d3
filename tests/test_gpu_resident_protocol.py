"""When a pass of a ResidentVolume sweeps first: the nine calls that run over the current extraction, each on a volume that was
never swept (the call sweeps, and answers what it answers after an explicit sweep), on one whose extraction an edit through the
context made stale (the call sweeps again with the same `sparse`, and answers the same) and on one whose extraction is current
(the call does not sweep and uploads nothing).  The volume is tiny: six boxes that touch each other inside a margin of label 0,
so that there are walls, a background and empty voxels for the nearest-label pass."""
import functools

import numpy as np
import pytest

from tissue_analysis_amd import _capi
from tissue_analysis_amd.extraction import ResidentVolume, wants_compaction

pytestmark = pytest.mark.gpu

SHAPE = (9, 10, 12)
SPARSE_IDS = (0, 5, 300000, 300007)


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def boxes():
    """uint16: labels 1..6 as 7 x 4 x {3, 4, 3} boxes, two along axis 1 and three along axis 2, label 0 around them."""
    V = np.zeros(SHAPE, dtype=np.uint16)
    label = 0
    for y in ((1, 5), (5, 9)):
        for z in ((1, 4), (4, 8), (8, 11)):
            label += 1
            V[1:8, y[0]:y[1], z[0]:z[1]] = label
    return frozen(V)


@functools.lru_cache(maxsize=None)
def sparse_boxes():
    """uint32, the ids SPARSE_IDS: sparse enough for the sweep to run in their ranks."""
    lut = np.array([0, 5, 300000, 300007, 5, 300000, 300007], dtype=np.uint32)
    return frozen(lut[boxes()])


@functools.lru_cache(maxsize=None)
def signal():
    return frozen(np.random.default_rng(11).integers(0, 256, SHAPE).astype(np.uint8))


CALLS = {
    "signal": lambda rv: rv.signal(signal()),
    "signal_histogram": lambda rv: rv.signal_histogram(signal()),
    "signal_quantiles": lambda rv: rv.signal_quantiles(signal(), q=[0.5]),
    "signal_moments": lambda rv: rv.signal_moments(signal()),
    "topology": lambda rv: rv.topology(),
    "meshes": lambda rv: rv.meshes(),
    "distance_map": lambda rv: rv.distance_map(),
    "nearest_labels": lambda rv: rv.nearest_labels(),
    "wall_geometry": lambda rv: rv.wall_geometry(),
}
IMAGES = {"distance_map": lambda r: {"image()": r.image()},
          "nearest_labels": lambda r: {"nearest()": r.nearest(), "distance()": r.distance()}}


def public_arrays(name, result):
    """Every public array (and count) the result of a call carries, by name; the images of the two passes that keep one."""
    out = dict((k, v) for k, v in vars(result).items()
               if not k.startswith("_") and k != "ms" and isinstance(v, (np.ndarray, int, tuple)))
    assert any(isinstance(v, np.ndarray) and v.size for v in out.values()), name
    out.update(IMAGES.get(name, lambda r: {})(result))
    return out


def answer(name, rv):
    result = CALLS[name](rv)
    ms = rv.ms[name]
    assert isinstance(ms, float) and ms > 0.0, (name, ms)
    return public_arrays(name, result)


def same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert np.array_equal(got[k], want[k], equal_nan=want[k].dtype.kind == "f"), k
        else:
            assert got[k] == want[k], k


@functools.lru_cache(maxsize=None)
def swept_first(name, sparse=False):
    """The answer of the call on a ResidentVolume that was extracted first: what every other order must give, bit for bit."""
    rv = ResidentVolume(sparse_boxes() if sparse else boxes())
    try:
        assert rv.extract().sparse == sparse
        return answer(name, rv)
    finally:
        rv.close()


def test_the_volumes_are_what_the_cases_need():
    V = boxes()
    assert V.dtype == np.uint16 and V.shape == SHAPE and np.unique(V).tolist() == list(range(7))
    assert (V[0] == 0).all() and (V[:, 0] == 0).all() and (V[:, :, -1] == 0).all()
    assert (V[:, :, :-1] != V[:, :, 1:])[(V[:, :, :-1] > 0) & (V[:, :, 1:] > 0)].any()          # cells touch cells
    W = sparse_boxes()
    assert W.dtype == np.uint32 and tuple(np.unique(W).tolist()) == SPARSE_IDS
    assert wants_compaction(int(W.max()), len(SPARSE_IDS)) and 300008 > 8 * 4 and 300007 >= 1 << 18


@pytest.mark.parametrize("name", list(CALLS))
def test_a_fresh_volume_is_swept_first(name):
    rv = ResidentVolume(boxes())
    try:
        assert rv.last is None
        got = answer(name, rv)
        assert rv.last is not None and not rv.last.sparse and rv.uploads == 1
        same(got, swept_first(name))
    finally:
        rv.close()


def stale_then(name, V, sparse):
    rv = ResidentVolume(V)
    try:
        x0 = rv.extract()
        assert x0.sparse == sparse
        # the identity on every id: the voxels stay, the extraction is stale (a compacted context takes one entry per rank)
        rv.ctx.relabel(x0.ids.astype(np.uint32) if sparse else np.arange(7, dtype=np.uint32))
        got = answer(name, rv)
        assert rv.last is not x0 and rv.last.sparse == x0.sparse == sparse and rv.uploads == 1
        same(got, swept_first(name, sparse))
    finally:
        rv.close()


@pytest.mark.parametrize("name", list(CALLS))
def test_a_stale_extraction_is_swept_again_with_the_same_sparse(name):
    stale_then(name, boxes(), False)


def test_a_stale_sparse_extraction_stays_sparse():
    stale_then("topology", sparse_boxes(), True)


@pytest.mark.parametrize("name", list(CALLS))
def test_a_current_extraction_is_not_swept_again(name):
    rv = ResidentVolume(boxes())
    try:
        x0 = rv.extract()
        got = answer(name, rv)
        assert rv.last is x0 and rv.uploads == 1
        same(got, swept_first(name))
    finally:
        rv.close()
