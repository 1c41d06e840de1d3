"""The host copy of a ResidentVolume after an edit on the device, in every memory layout: `relabel`, `relabel_components` and
`apply_nearest` copy the volume back in the device's memory order, which is the order of the image that was uploaded -- so
`rv.host` must keep that image's layout, also where it has to become a copy of its own because the image is read-only.  And the
images that come back as flat bytes in memory order (`components_image`, `distance_image`, `nearest_images`) over a range of
planes of an image that is not C-ordered."""
import functools

import numpy as np
import pytest

import nearest_reference
from tissue_analysis_amd import _capi
from tissue_analysis_amd.extraction import ResidentVolume

pytestmark = pytest.mark.gpu

LUT = np.array([0, 1, 2, 1, 4, 0], dtype=np.uint32)
LAYOUTS = {
    "C": lambda V: np.array(V, order="C"),
    "F": lambda V: np.asfortranarray(V),
    "transposed": lambda V: np.ascontiguousarray(V.transpose(1, 2, 0)).transpose(2, 0, 1),
}


@functools.lru_cache(maxsize=None)
def volume():
    V = np.random.default_rng(5).integers(0, 6, (5, 6, 7)).astype(np.uint16)
    V.setflags(write=False)
    return V


@functools.lru_cache(maxsize=None)
def nearest_filled():
    n, d2 = nearest_reference.brute(volume(), 0)
    image = nearest_reference.result(volume(), n, d2, 0)[0]
    assert (image != volume()).any() and not (image == 0).any()
    image.setflags(write=False)
    return image


def edit_relabel(rv):
    return rv.relabel(LUT), LUT[volume()].astype(np.uint16)


def edit_relabel_components(rv):
    table = rv.components().split_map()
    rows = np.array(rv.components_image())
    assert rows.shape == volume().shape and not (rows == _capi.COMPONENT_NONE).any()
    assert (table[rows] != volume()).any() and int(table.max()) <= 0xFFFF          # fragments get labels of their own
    return rv.relabel_components(table), table[rows].astype(np.uint16)


def edit_apply_nearest(rv):
    rv.nearest_labels(empty=0)
    return rv.apply_nearest(), nearest_filled()


EDITS = {"relabel": edit_relabel, "relabel_components": edit_relabel_components, "apply_nearest": edit_apply_nearest}


def test_the_layouts_differ_in_memory_only():
    V = volume()
    orders = set()
    for name, make in LAYOUTS.items():
        a = make(V)
        assert np.array_equal(a, V) and a.dtype == np.uint16 and a.flags.writeable and _capi._dense_permuted(a), name
        orders.add(tuple(np.argsort(a.strides).tolist()))
    assert len(orders) == 3 and not LAYOUTS["transposed"](V).flags.f_contiguous
    assert not np.array_equal(LUT[V], V)


@pytest.mark.parametrize("writeable", [True, False], ids=["writeable", "readonly"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("edit", list(EDITS))
def test_the_host_copy_follows_an_edit(edit, layout, writeable):
    given = LAYOUTS[layout](volume())
    given.setflags(write=writeable)
    rv = ResidentVolume(given)
    try:
        assert rv.is_input and rv.host is given
        x, want = EDITS[edit](rv)
        assert rv.host.shape == want.shape and rv.host.dtype == want.dtype
        assert np.array_equal(rv.host, want), "rv.host is not the edited image, element by element"
        assert rv.host.flags.writeable and rv.host.strides == given.strides
        if writeable:
            assert rv.is_input and np.shares_memory(rv.host, given) and np.array_equal(given, want)
        else:
            assert not rv.is_input and not np.shares_memory(rv.host, given) and np.array_equal(given, volume())
        assert rv.last is x and np.array_equal(x.count, np.bincount(want.reshape(-1), minlength=x.nrows))
    finally:
        rv.close()


def test_plane_ranges_of_the_images_in_fortran_order():
    given = LAYOUTS["F"](volume())
    rv = ResidentVolume(given)
    try:
        slow = int(np.argmax(given.strides))
        assert slow == 2
        planes = (slice(None), slice(None), slice(1, 3))
        rv.components()
        full, part = [rv.components_image()], [rv.components_image(1, 2)]
        rv.distance_map()
        full.append(rv.distance_image())
        part.append(rv.distance_image(1, 2))
        rv.nearest_labels(empty=0)
        full += rv.nearest_images()
        part += rv.nearest_images(1, 2)
        assert [a.dtype for a in full] == [np.uint32, np.float64, np.uint32, np.float64]
        n, d2 = nearest_reference.brute(volume(), 0)
        assert np.array_equal(full[2], n) and np.array_equal(full[3], d2)
        for whole, some in zip(full, part):
            assert whole.shape == given.shape and some.shape == (5, 6, 2) and some.dtype == whole.dtype
            assert np.array_equal(some, whole[planes])
            assert some.strides == tuple(s // 2 * some.dtype.itemsize for s in given.strides)
    finally:
        rv.close()
