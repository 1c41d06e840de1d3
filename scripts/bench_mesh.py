#!/usr/bin/env python3
"""Cell-mesh throughput (include/tissue_scan_mesh.h): one JSON line per configuration.

    python scripts/bench_mesh.py [--reps 10] [--configs C4,512^3] [--no-cpu] [--out FILE]

  device_ms        median over --reps extractions of ta_mesh_timing: the count kernels + the emit / sort / resolve kernels
                   (the one read-back of the totals between them is not counted)
  vertices, triangles, cells
  out_bytes        the mesh held on the device: corners u64[V] + triangles u32[T][3] + cell, neighbour u32[T]
  model_bytes      bytes read plus written by all kernels (byte model below); frac_8tbs = model_bytes / device_ms against 8 TB/s
Configurations: C4 (1024^3 uint32, 50k seeds) and 512^3 uint16 (5k seeds), each at sub_factor 1 and 4 and a labels subset of
1 % at sub_factor 1; and, for context, the NumPy restatement (tests/mesh_reference.py) on the central 256^3 crop of C4 on one CPU core."""
import ctypes
import os
import statistics
import sys
import time

import numpy as np

import featbench as fb
from tissue_analysis_amd import _capi

CASES = (("all cells", 1, None), ("all cells", 4, None), ("1% of cells", 1, 0.01))
CROP = []                       # C4's central 256^3, for the CPU line


def byte_model(dims, s, L, F, V, key_bits):
    """Bytes the kernels must move, by kernel (labels read once per pass that reads them; neighbours come from the caches)."""
    m = [-(-int(n) // s) for n in dims]
    nw = m[0] * m[1] * m[2]
    ng = (m[0] + 1) * (m[1] + 1) * (m[2] + 1)
    waves_f, waves_c = -(-nw // 1024), -(-ng // 1024)
    passes = -(-key_bits // 10)
    return dict(
        face_count=nw * L + 4 * waves_f,
        corner_count=nw * L + 4 * waves_c,
        scans=12 * (waves_f + waves_c),
        corner_emit=nw * L + 8 * waves_c + 16 * V,                 # corner u64 | key u32 | index u32
        corner_sort=passes * 20 * V,                             # per pass: histogram reads keys; scatter reads and writes keys + values
        corner_bounds_gather=4 * V + 4 * V + 8 * V + 8 * V,      # keys; perm, corner (gathered), vertex corners
        face_emit=nw * L + 8 * waves_f + 20 * F,                 # record u64 | neighbour u32 | key u32 | index u32
        face_sort=passes * 20 * F,
        face_bounds=4 * F,
        resolve=F * (4 + 4 + 8 + 4 + 4 * 8 + 2 * 12 + 2 * 8),   # key, perm, record, neighbour, 4 vertex look-ups (last probe); 2 triangles
    )


def run(cfg, a):
    with fb.resident(cfg) as (ctx, vol, L):
        ctx.extract(_capi.F_ALL, L)
        count = ctx.labels()[0]
        present = np.flatnonzero(count)
        key_bits = max(1, int(L).bit_length())
        for what, s, frac in CASES:
            wanted = None
            nreq = present.size
            if frac is not None:
                pick = present[1::max(1, int(round(1 / frac)))]
                wanted = np.zeros(L + 1, dtype=np.uint8)
                wanted[pick] = 1
                nreq = pick.size
            ms = fb.timed(lambda: _check_extract(ctx, s, wanted), ctx.mesh_timing, a.reps, warmup=2)
            C, V, T = _size(ctx)
            F = T // 2
            model = byte_model(cfg.dims, s, cfg.dtype.itemsize, F, V, key_bits)
            mb = sum(model.values())
            yield dict(config=cfg.name, what=what, dims=list(cfg.dims), labels=cfg.dtype.name, sub_factor=s, cells_requested=int(nreq),
                       cells=int(C), vertices=int(V), triangles=int(T), **fb.spread("device_ms", ms, ("min",)), reps=a.reps,
                       out_bytes=int(8 * V + 12 * T + 8 * T), model_bytes=int(mb),
                       frac_8tbs=round(mb / (statistics.median(ms) * 1e-3) / fb.TBS, 4), model_by_kernel=model)
        if cfg.name == "C4":
            CROP[:] = [vol[384:640, 384:640, 384:640].cpu().numpy().view(cfg.dtype)]


def _check_extract(ctx, s, wanted):
    """ta_mesh_extract alone (Context.mesh would also copy the whole mesh to the host)."""
    keep = None if wanted is None else np.ascontiguousarray(wanted, dtype=np.uint8)
    _capi._check(ctx._lib.ta_mesh_extract(ctx._h, int(s), None if keep is None else keep.ctypes.data))


def _size(ctx):
    C, V, T = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    _capi._check(ctx._lib.ta_mesh_size(ctx._h, ctypes.byref(C), ctypes.byref(V), ctypes.byref(T)))
    return C.value, V.value, T.value


def cpu_line(a):
    if not CROP or a.no_cpu:
        return []
    sys.path.insert(0, os.path.join(fb.ROOT, "tests"))
    import mesh_reference
    crop = CROP.pop()                                 # taken: a later call in this process starts without a crop
    labels = np.unique(crop)[1:]
    t0 = time.perf_counter()
    r = mesh_reference.mesh(crop, labels=labels)
    cpu = (time.perf_counter() - t0) * 1e3
    return dict(config="C4 central crop 256^3", what="NumPy restatement (tests/mesh_reference.py), 1 CPU core",
                cells=int(labels.size), triangles=int(len(r["triangles"])), cpu_ms=round(cpu, 1))


def main():
    fb.main(run, reps=10, configs="C4,512^3", out=None, mode="w", after=cpu_line,
            extra_args=[("--no-cpu", dict(action="store_true"))])


if __name__ == "__main__":
    main()
