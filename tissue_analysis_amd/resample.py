"""A second volume on another grid -- the next frame of a time lapse, a signal channel of another stack depth -- sampled through
an affine map onto the grid of the resident label volume, on the GPU (include/tissue_scan_resample.h,
csrc/kernels_resample.hip): nearest neighbour for labels, trilinear for signals.  The result stays in device memory, where the
overlap and the signal passes read it.

The device pass speaks voxel indices only: a 3 x 4 index matrix takes a target voxel index to a continuous source index.
`index_matrix` builds it from a physical transform and the two voxel sizes.  Estimating the transform (registration) is not part
of this library."""
from __future__ import annotations

import numpy as np

from . import _capi

_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _homogeneous(transform):
    """`transform` as a 4 x 4 float64 matrix: None = identity, a 3 x 3 one (a 2-D image's) leaves axis 2 alone."""
    if transform is None:
        return np.eye(4)
    t = np.asarray(transform, dtype=np.float64)
    if t.shape == (3, 3):
        full = np.eye(4)
        full[:2, :2] = t[:2, :2]
        full[:2, 3] = t[:2, 2]
        if not np.array_equal(t[2], (0.0, 0.0, 1.0)):
            raise ValueError("the last row of a homogeneous 3 x 3 transform must be (0, 0, 1)")
        return full
    if t.shape != (4, 4):
        raise ValueError("a transform is a 4 x 4 homogeneous matrix (3 x 3 for 2-D images), not %s" % (t.shape,))
    if not np.array_equal(t[3], (0.0, 0.0, 0.0, 1.0)):
        raise ValueError("the last row of a homogeneous 4 x 4 transform must be (0, 0, 0, 1)")
    return t


def _voxelsize3(vs):
    v = [float(x) for x in np.asarray((1.0, 1.0, 1.0) if vs is None else vs, dtype=np.float64).reshape(-1)]
    if len(v) == 2:
        v.append(1.0)
    if len(v) != 3 or not all(np.isfinite(x) and x > 0.0 for x in v):
        raise ValueError("a voxel size has two or three positive finite entries")
    return np.array(v)


def index_matrix(transform=None, target_voxelsize=None, source_voxelsize=None):
    """The 3 x 4 index matrix diag(1 / vs_src) . T . diag(vs_tgt) of `transform`, a 4 x 4 (3 x 3 for 2-D images) homogeneous
    matrix that maps PHYSICAL TARGET coordinates to PHYSICAL SOURCE coordinates; None is a pure voxel-size change.  The matrix
    takes a target voxel index (i0, i1, i2, 1) to the continuous source index."""
    t = _homogeneous(transform)
    vt, vs = _voxelsize3(target_voxelsize), _voxelsize3(source_voxelsize)
    m = t[:3].copy()
    m[:, :3] = m[:, :3] * vt[None, :]
    return m / vs[:, None]


def transform_points(points, transform):
    """The points (N x 3, or N x 2 with a 3 x 3 transform; one point as a vector) carried through the homogeneous `transform`:
    barycentres or junction positions of one frame in the coordinates of the other.  Host arithmetic, float64."""
    p = np.asarray(points, dtype=np.float64)
    one = p.ndim == 1
    p = np.atleast_2d(p)
    k = p.shape[1]
    if k not in (2, 3):
        raise ValueError("points have two or three coordinates")
    t = _homogeneous(transform)
    if k == 2:
        p = np.concatenate([p, np.zeros((p.shape[0], 1))], axis=1)
    out = (p @ t[:3, :3].T + t[:3, 3])[:, :k]
    return out[0] if one else out


def _cuda_tensor(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda") and bool(x.is_cuda)


def _set_source(ctx, source):
    """Upload or adopt `source` (a NumPy array or a contiguous CUDA tensor; a 2-D one becomes (X, Y, 1)); returns its itemsize."""
    if _cuda_tensor(source):
        shape = tuple(int(d) for d in source.shape)
        if len(shape) == 2:
            shape = shape + (1,)
        if len(shape) != 3 or not source.is_contiguous():
            raise ValueError("a device-resident source must be a contiguous 2-D or 3-D tensor")
        if source.element_size() not in _DTYPES or source.is_floating_point():
            raise TypeError("source tensors must hold 1-, 2- or 4-byte integers")
        ctx.set_resample_source_device(source.data_ptr(), source.element_size(), shape, keep=source)
        return source.element_size()
    a = np.asarray(source)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.dtype not in _capi.RESAMPLE_DTYPES:
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError("source volumes must be integer arrays, not %s" % a.dtype)
        if a.size and (a.min() < 0 or a.max() > np.iinfo(np.uint32).max):
            raise ValueError("source values must fit in uint32")
        a = a.astype(np.uint16 if (a.size == 0 or a.max() <= 65535) else np.uint32)
    ctx.set_resample_source(a)
    return a.dtype.itemsize


class Resampled(object):
    """The result of one gather pass, resident on the device of `resident` until its next resample (or a label volume of other
    dims).

        outside     owned target voxels that fell outside the source and received `fill`
        ms          milliseconds of the kernel on the device
        order       0 = nearest neighbour, 1 = trilinear
    """

    def __init__(self, resident, order, dtype):
        self.resident = resident            # (keeps the context, which owns the buffer, alive)
        self.order = int(order)
        self.dtype = np.dtype(dtype)
        self.shape = tuple(resident.host.shape)
        ctx = resident.ctx
        self.outside = ctx.resample_outside()
        self.ms = ctx.resample_timing()
        self._serial = resident._resample_serial

    def _current(self):
        r = self.resident
        if r.ctx is None or r._resample_serial != self._serial:
            raise ValueError("this Resampled is stale: its volume has been resampled again, or closed")
        return r.ctx

    def image(self):
        """The result as a NumPy array shaped like the label image."""
        ctx = self._current()
        flat = ctx.resample_get()
        axes = ctx.memory_axes()
        mshape = tuple(self.shape[a] for a in axes)
        return np.ascontiguousarray(np.transpose(flat.reshape(mshape), np.argsort(axes)))

    def tensor(self):
        """A torch view of the device buffer in the labels' memory layout (uint8, or int16 / int32 storage holding uint16 / uint32
        values); the object it belongs to keeps the buffer alive."""
        import torch
        ctx = self._current()
        ptr, itemsize = ctx.resample_device()
        axes = ctx.memory_axes()
        mshape = tuple(self.shape[a] for a in axes)
        typestr = {1: "|u1", 2: "<i2", 4: "<i4"}[itemsize]
        holder = type("_DeviceArray", (object,), {})()
        holder.__cuda_array_interface__ = dict(shape=mshape, typestr=typestr, data=(int(ptr), False), version=2, strides=None)
        holder.owner = self
        t = torch.as_tensor(holder, device="cuda:%d" % ctx.device)
        t._resampled_owner = self
        return t.permute(*[int(i) for i in np.argsort(axes)])


def resident_resample(resident, source, matrix, order=0, fill=0):
    """One gather pass onto the grid of the volume resident in `resident` (a ResidentVolume): `source` a NumPy array or CUDA
    tensor of uint8 / uint16 / uint32 and any shape, `matrix` the 3 x 4 index matrix (`index_matrix`), order 0 (nearest
    neighbour; labels) or 1 (trilinear; uint8 / uint16 signals), `fill` the value of voxels that fall outside the source."""
    if order not in (0, 1):
        raise ValueError("order must be 0 (nearest neighbour) or 1 (trilinear); higher orders are not built")
    ctx = resident.ctx
    itemsize = _set_source(ctx, source)
    ctx.resample_extract(matrix, _capi.RS_LINEAR if order else _capi.RS_NEAREST, fill)
    resident._resample_serial = getattr(resident, "_resample_serial", 0) + 1
    return Resampled(resident, order, _DTYPES[itemsize])


class OnGrid(object):
    """A signal image on another grid together with its index matrix: what the signal passes take in place of an array when the
    image is to be resampled onto the labels' grid on the device (`ResidentVolume.signal(signal, matrix=...)`)."""

    def __init__(self, resident, source, matrix, order=1, fill=0):
        self.resident, self.source, self.matrix, self.order, self.fill = resident, source, matrix, order, fill
        if _cuda_tensor(source):        # (int16 storage holds uint16 values, as for label tensors)
            dt = np.dtype(_DTYPES.get(0 if source.is_floating_point() else source.element_size(), np.float64))
        else:
            dt = np.asarray(source).dtype
        if dt not in _capi.SIGNAL_DTYPES:
            raise TypeError("signal images must be uint8 or uint16, not %s" % dt)
        self.dtype = dt
        self.last = None

    def adopt_as_signal(self, ctx):
        self.last = resident_resample(self.resident, self.source, self.matrix, self.order, self.fill)
        ctx.resample_as_signal()
        return self.dtype.itemsize
