#!/usr/bin/env python3
"""Overlap-pass throughput (include/tissue_scan_overlap.h): one JSON line per configuration, also written to
profiles/overlap_bench.jsonl.

    python scripts/bench_overlap.py [--reps 30] [--out profiles/overlap_bench.jsonl]

  kernel_ms        median of the pass kernel's HIP-event durations (ta_overlap_timing) over --reps passes
  compact_ms       median of count + scan + emit + sort + unpack (ta_overlap_timing_compaction)
  pairs            rows of the table; passes: runs of the pass kernel the last table took (1 = no capacity re-run)
  bytes            algorithmic bytes: voxels x (itemsize of A + itemsize of B)
  frac_8tbs        bytes / kernel_ms against 8 TB/s
  frac_read_probe  ... against what ta_read_probe reaches on A's buffer in this run
Configurations: C4 (1024^3 uint32, 50k seeds) against a second frame of the same generator with another seed (uint32), C4
against itself (the diagonal), 512^3 uint16 against uint16; and, for context, np.unique on a 256^3 crop on one CPU core."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tissue_analysis_amd import synth  # noqa: E402
from tissue_analysis_amd import device as dev  # noqa: E402

TBS = 8e12


def run(name, dims, dtype_a, dtype_b, n_cells, seed_a, seed_b, reps):
    import torch
    dtype_a, dtype_b = np.dtype(dtype_a), np.dtype(dtype_b)
    ctx = dev.torch_context(0)
    va, _ = dev.synth_slab(ctx, dims, dtype_a, n_cells, seed_a)
    vb = va if seed_b is None else dev.synth_slab(ctx, dims, dtype_b, n_cells, seed_b)[0]
    torch.cuda.synchronize()
    ctx.set_volume_device(va.data_ptr(), dtype_a.itemsize, va.shape, keep=va)
    ctx.set_overlap_device(vb.data_ptr(), dtype_b.itemsize, keep=vb)
    probe_ms = ctx.read_probe(va.data_ptr(), va.numel() * va.element_size(), repeats=5)
    probe_bps = va.numel() * va.element_size() / (probe_ms * 1e-3)
    nbytes = int(np.prod(dims)) * (dtype_a.itemsize + dtype_b.itemsize)
    for _ in range(3):
        ctx.overlap_extract()
        ctx.overlap_size()
    ms, post = [], []
    for _ in range(reps):
        ctx.overlap_extract()
        pairs = ctx.overlap_size()
        ms.append(ctx.overlap_timing())
        p, passes = ctx.overlap_timing_compaction()
        post.append(p)
    k = statistics.median(ms)
    bps = nbytes / (k * 1e-3)
    line = dict(config=name, dims=list(dims), a=dtype_a.name, b=dtype_b.name, kernel_ms=round(k, 4), kernel_ms_min=round(min(ms), 4),
                kernel_ms_max=round(max(ms), 4), compact_ms=round(statistics.median(post), 4), pairs=int(pairs), passes=passes,
                reps=reps, bytes=nbytes, tb_per_s=round(bps / 1e12, 3), frac_8tbs=round(bps / TBS, 4),
                read_probe_tbs=round(probe_bps / 1e12, 3), frac_read_probe=round(bps / probe_bps, 4))
    crop = None
    if seed_b is not None and dtype_a.itemsize == 4:
        o = [(d - 256) // 2 for d in dims]                 # the centre: cells, not the background around the tissue
        crop = tuple(v[o[0]:o[0] + 256, o[1]:o[1] + 256, o[2]:o[2] + 256].cpu().numpy().view(t) for v, t in ((va, dtype_a), (vb, dtype_b)))
    ctx.close()
    del va, vb
    torch.cuda.empty_cache()
    return line, crop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlap_bench.jsonl"))
    a = ap.parse_args()
    c4, c2 = synth.CONFIGS["C4"], synth.CONFIGS["C2"]
    lines = []
    line, crop = run("C4 x second frame", c4["dims"], c4["dtype"], "uint32", c4["n_cells"], c4["seed"], c4["seed"] + 100, a.reps)
    lines.append(line)
    lines.append(run("C4 x itself", c4["dims"], c4["dtype"], c4["dtype"], c4["n_cells"], c4["seed"], None, a.reps)[0])
    lines.append(run("512^3", c2["dims"], "uint16", "uint16", c2["n_cells"], c2["seed"], c2["seed"] + 100, a.reps)[0])
    A, B = crop
    t0 = time.perf_counter()
    keys = (A.astype(np.uint64).reshape(-1) << np.uint64(32)) | B.astype(np.uint64).reshape(-1)
    u = np.unique(keys, return_counts=True)[0]
    cpu = (time.perf_counter() - t0) * 1e3
    lines.append(dict(config="C4 centre crop 256^3", what="np.unique on a << 32 | b, 1 CPU core", pairs=int(u.size), cpu_ms=round(cpu, 1)))
    with open(a.out, "w") as f:
        for d in lines:
            print(json.dumps(d))
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
