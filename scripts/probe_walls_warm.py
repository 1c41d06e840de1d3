"""The wall-voxel kernels on a resident volume with the chip at its sustained clock (what bench.py's secondary.wall_voxels_c2
reports): python scripts/probe_walls_warm.py [C2|C3]"""
import sys
import time

import numpy as np

import featbench as fb

name = sys.argv[1] if len(sys.argv) > 1 else "C2"
cfg = fb.config(name)
with fb.resident(cfg) as (ctx, vol, max_label):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:                  # settle the clock with the sweep
        ctx.extract(0x0f, max_label)
    best = None
    for _ in range(4):
        lo, hi, coords, ms = ctx.wall_voxels()
        best = ms if best is None else min(best, ms)
alg = float(np.prod(cfg.dims)) * cfg.dtype.itemsize + 20.0 * lo.size
print("%s: %d records, count + scan + fetch kernels best %.4f ms = %.1f%% of 8 TB/s" % (name, lo.size, best, alg / best / 1e6 / 80.0), flush=True)
