#!/usr/bin/env python3
"""Signal-moment pass throughput (include/tissue_scan_sigmoments.h): one JSON line per configuration, appended to
profiles/sigmoments_bench.jsonl.

    python scripts/bench_signal_moments.py [--reps 30] [--configs C4,512^3] [--out profiles/sigmoments_bench.jsonl]

  kernel_ms        median of the pass kernel's HIP-event durations (ta_sigmom_timing) over --reps passes
  signal_ms        the yardstick, in the same process on the same volume and signal: the labels-only signal pass
                   (ta_signal_timing of TA_SIG_LABELS), median over --reps passes
  ratio            kernel_ms / signal_ms
  bytes            algorithmic bytes: voxels x (label itemsize + signal itemsize)
  frac_read_probe  bytes / kernel_ms against what ta_read_probe reaches on the same label buffer in this run
  spills           records that missed a workgroup's LDS table (ta_sigmom_debug); tiles_per_group, groups: its launch plan
Configurations: C4 (1024^3 uint32, 50k seeds) with a uint16 signal; 512^3 uint16 labels with a uint8 signal."""
import statistics

import numpy as np

import featbench as fb
from tissue_analysis_amd import _capi


def run(cfg, a):
    import torch
    sdtype = fb.signal_dtype(cfg)
    nbytes = int(np.prod(cfg.dims)) * (cfg.dtype.itemsize + sdtype.itemsize)
    with fb.resident(cfg) as (ctx, vol, L):
        sig = fb.random_signal(cfg.dims, sdtype.itemsize, torch.Generator(device="cuda").manual_seed(cfg.seed))
        torch.cuda.synchronize()
        ctx.set_signal_device(sig.data_ptr(), sdtype.itemsize, keep=sig)
        ctx.extract(_capi.F_ALL, L)
        ctx.adjacency_size()
        _, probe_bps = fb.read_probe(ctx, vol)
        ms = fb.timed(ctx.sigmom_extract, ctx.sigmom_timing, a.reps)
        debug = ctx.sigmom_debug()
        sms = fb.timed(lambda: ctx.signal_extract(_capi.SIG_LABELS), ctx.signal_timing, a.reps)
        sdebug = ctx.signal_debug()
    k, s = statistics.median(ms), statistics.median(sms)
    return dict(config=cfg.name, dims=list(cfg.dims), labels=cfg.dtype.name, signal=sdtype.name, reps=a.reps,
                **fb.spread("kernel_ms", ms, ("min",)), **fb.spread("signal_ms", sms, ("min",)), ratio=round(k / s, 3), bytes=nbytes,
                read_probe_tbs=round(probe_bps / 1e12, 3), frac_read_probe=round(nbytes / (k * 1e-3) / probe_bps, 4),
                signal_frac_read_probe=round(nbytes / (s * 1e-3) / probe_bps, 4), spills=debug["spills"],
                tiles_per_group=debug["tiles_per_group"], groups=debug["groups"], signal_label_spills=sdebug["label_spills"])


def main():
    fb.main(run, reps=30, configs="C4,512^3", out="profiles/sigmoments_bench.jsonl", mode="a")


if __name__ == "__main__":
    main()
