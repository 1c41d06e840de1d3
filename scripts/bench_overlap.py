#!/usr/bin/env python3
"""Overlap-pass throughput (include/tissue_scan_overlap.h): one JSON line per configuration, also written to
profiles/overlap_bench.jsonl.

    python scripts/bench_overlap.py [--reps 30] [--configs C4,512^3] [--out profiles/overlap_bench.jsonl]

  kernel_ms        median of the pass kernel's HIP-event durations (ta_overlap_timing) over --reps passes
  compact_ms       median of count + scan + emit + sort + unpack (ta_overlap_timing_compaction)
  pairs            rows of the table; passes: runs of the pass kernel the last table took (1 = no capacity re-run)
  bytes            algorithmic bytes: voxels x (itemsize of A + itemsize of B)
  frac_8tbs        bytes / kernel_ms against 8 TB/s
  frac_read_probe  ... against what ta_read_probe reaches on A's buffer in this run
Configurations: C4 (1024^3 uint32, 50k seeds) against a second frame of the same generator with another seed (uint32), C4
against itself (the diagonal), 512^3 uint16 against uint16; and, for context, np.unique on a 256^3 crop on one CPU core."""
import statistics
import time

import numpy as np

import featbench as fb
from tissue_analysis_amd import device as dev

CROP = []                       # C4's central 256^3 of both frames, for the CPU line


def one(name, cfg, seed_b, reps):
    """cfg's volume against a second frame of the same generator (seed_b), or against itself (seed_b None)."""
    import torch
    with fb.resident(cfg) as (ctx, va, _):
        vb = va if seed_b is None else dev.synth_slab(ctx, cfg.dims, cfg.dtype, cfg.n_cells, seed_b)[0]
        torch.cuda.synchronize()
        ctx.set_overlap_device(vb.data_ptr(), cfg.dtype.itemsize, keep=vb)
        _, probe_bps = fb.read_probe(ctx, va)
        nbytes = int(np.prod(cfg.dims)) * 2 * cfg.dtype.itemsize
        last = {}

        def overlap():
            ctx.overlap_extract()
            last["pairs"] = ctx.overlap_size()

        def timing():
            return ctx.overlap_timing(), ctx.overlap_timing_compaction()

        ms, post = zip(*fb.timed(overlap, timing, reps))
        passes = post[-1][1]
        if seed_b is not None and cfg.name == "C4":
            o = [(d - 256) // 2 for d in cfg.dims]             # the centre: cells, not the background around the tissue
            CROP[:] = [v[o[0]:o[0] + 256, o[1]:o[1] + 256, o[2]:o[2] + 256].cpu().numpy().view(cfg.dtype) for v in (va, vb)]
    bps = nbytes / (statistics.median(ms) * 1e-3)
    return dict(config=name, dims=list(cfg.dims), a=cfg.dtype.name, b=cfg.dtype.name, **fb.spread("kernel_ms", ms),
                compact_ms=round(statistics.median([p for p, _ in post]), 4), pairs=int(last["pairs"]), passes=passes, reps=reps,
                bytes=nbytes, tb_per_s=round(bps / 1e12, 3), frac_8tbs=round(bps / fb.TBS, 4),
                read_probe_tbs=round(probe_bps / 1e12, 3), frac_read_probe=round(bps / probe_bps, 4))


def run(cfg, a):
    if cfg.name != "C4":
        return one(cfg.name, cfg, cfg.seed + 100, a.reps)
    return (one(name, cfg, seed_b, a.reps) for name, seed_b in (("C4 x second frame", cfg.seed + 100), ("C4 x itself", None)))


def cpu_line(a):
    if not CROP:
        return []
    B, A = CROP.pop(), CROP.pop()                     # taken: a later call in this process starts without a crop
    t0 = time.perf_counter()
    keys = (A.astype(np.uint64).reshape(-1) << np.uint64(32)) | B.astype(np.uint64).reshape(-1)
    u = np.unique(keys, return_counts=True)[0]
    cpu = (time.perf_counter() - t0) * 1e3
    return dict(config="C4 centre crop 256^3", what="np.unique on a << 32 | b, 1 CPU core", pairs=int(u.size), cpu_ms=round(cpu, 1))


def main():
    fb.main(run, reps=30, configs="C4,512^3", out="profiles/overlap_bench.jsonl", mode="w", after=cpu_line)


if __name__ == "__main__":
    main()
