"""Time the label lookup-table sweep on a resident volume: python scripts/probe_relabel.py [C4]"""
import sys
import time

import numpy as np
import torch

import featbench as fb

name = sys.argv[1] if len(sys.argv) > 1 else "C4"
cfg = fb.config(name)
with fb.resident(cfg) as (ctx, vol, max_label):
    lut = np.arange(max_label + 1, dtype=np.uint32)
    lut[2::3] = 0                                  # erase a third of the cells
    nbytes = 2.0 * np.prod(cfg.dims) * cfg.dtype.itemsize  # one read + one write per voxel
    for it in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.relabel(lut)                           # includes the table upload and a stream sync
        dt = time.perf_counter() - t0
        print("%s relabel %.3f ms  %.0f GB/s (read+write) = %.1f%% of 8 TB/s" % (name, dt * 1e3, nbytes / dt / 1e9, nbytes / dt / 8e10), flush=True)
