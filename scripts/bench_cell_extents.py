#!/usr/bin/env python3
"""Extent pass throughput (include/tissue_scan_extents.h): one JSON line per configuration, appended to
profiles/extents_bench.jsonl.

    python scripts/bench_cell_extents.py [--reps 30] [--configs C4,512^3] [--out profiles/extents_bench.jsonl]

  kernel_ms        median of the pass kernel's HIP-event durations (ta_extents_timing) over --reps passes, with every label's
                   principal axes as its directions; kernel_ms_min, kernel_ms_p25, kernel_ms_p75: the spread over the same passes
  sigmom_ms        the yardstick, in the same process on the same volume, its passes alternating with the extent passes: the
                   signal-moment pass (ta_sigmom_timing) with a random signal; _min, _p25, _p75 likewise
  ratio            kernel_ms / sigmom_ms
  bytes            algorithmic bytes of the extent pass: voxels x label itemsize (the yardstick reads the signal too: sigmom_bytes)
  frac_read_probe  bytes / kernel_ms against what ta_read_probe reaches on the same label buffer in this run
  spills           records that missed a workgroup's LDS table (ta_extents_debug); tiles_per_group, groups: its launch plan
Configurations: C4 (1024^3 uint32, 50k seeds; uint16 signal for the yardstick); 512^3 uint16 labels (uint8 signal)."""
import statistics

import numpy as np

import featbench as fb
from tissue_analysis_amd import _capi
from tissue_analysis_amd.cell_extents import extent_weights, principal_frames
from tissue_analysis_amd.extraction import Extraction

QUARTILES = ("min", "p25", "p75")


def run(cfg, a):
    import torch
    sdtype = fb.signal_dtype(cfg)
    nvox = int(np.prod(cfg.dims))
    with fb.resident(cfg) as (ctx, vol, L):
        sig = fb.random_signal(cfg.dims, sdtype.itemsize, torch.Generator(device="cuda").manual_seed(cfg.seed))
        torch.cuda.synchronize()
        ctx.set_signal_device(sig.data_ptr(), sdtype.itemsize, keep=sig)
        ctx.extract(_capi.F_ALL, L)
        ctx.adjacency_size()
        count, bbox, sum1, sum2 = ctx.labels()
        none = np.zeros(0, dtype=np.uint32)
        x = Extraction(tuple(cfg.dims), L, count, bbox, sum1, sum2, none, none, np.zeros((0, 3), dtype=np.uint64))
        weights = extent_weights(principal_frames(x), perm=ctx.memory_axes())
        _, probe_bps = fb.read_probe(ctx, vol)
        k, s = fb.alternating_ms([(lambda: ctx.extents_extract(weights), ctx.extents_timing), (ctx.sigmom_extract, ctx.sigmom_timing)], a.reps)
        debug, sdebug = ctx.extents_debug(), ctx.sigmom_debug()
        lo, hi = ctx.extents_rows()
    nbytes = nvox * cfg.dtype.itemsize
    km, sm = statistics.median(k), statistics.median(s)
    return dict(config=cfg.name, dims=list(cfg.dims), labels=cfg.dtype.name, signal=sdtype.name, reps=a.reps, rows=int(L) + 1,
                rows_with_voxels=int(np.isfinite(lo[:, 0]).sum()), **fb.spread("kernel_ms", k, QUARTILES),
                **fb.spread("sigmom_ms", s, QUARTILES), ratio=round(km / sm, 3), bytes=nbytes,
                sigmom_bytes=nvox * (cfg.dtype.itemsize + sdtype.itemsize), read_probe_tbs=round(probe_bps / 1e12, 3),
                frac_read_probe=round(nbytes / (km * 1e-3) / probe_bps, 4), spills=debug["spills"],
                tiles_per_group=debug["tiles_per_group"], groups=debug["groups"], sigmom_spills=sdebug["spills"])


def main():
    fb.main(run, reps=30, configs="C4,512^3", out="profiles/extents_bench.jsonl", mode="a")


if __name__ == "__main__":
    main()
