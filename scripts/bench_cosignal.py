#!/usr/bin/env python3
"""Two-channel pass throughput (include/tissue_scan_cosignal.h): one JSON line per configuration, appended to
profiles/cosignal_bench.jsonl.

    python scripts/bench_cosignal.py [--reps 30] [--configs C4,512^3] [--out profiles/cosignal_bench.jsonl]

  kernel_ms        median of the pass kernel's HIP-event durations (ta_cosignal_timing) over --reps passes after 3 warm-ups
  signal_a_ms, signal_b_ms   the yardstick, in the same process on the same buffers: the labels-only signal pass
                   (ta_signal_timing of TA_SIG_LABELS) with channel A, then with channel B as the context's signal, median each
  signal_ms        their mean: one labels-only signal pass; the two sums and the two sums of squares cost two of them before
                   this pass existed
  ratio            kernel_ms / signal_ms; the pass is meant to stay at or below 2.0, the two passes it replaces
  bytes            algorithmic bytes: voxels x (label itemsize + both channel itemsizes)
  frac_read_probe  bytes / kernel_ms against what ta_read_probe reaches on the same label buffer in this run
  spills           records that missed a workgroup's LDS table (ta_cosignal_debug); tiles_per_group, groups: its launch plan
Configurations: C4 (1024^3 uint32, 50k seeds) with two uint16 channels; 512^3 uint16 labels with two uint8 channels."""
import statistics

import numpy as np

import featbench as fb
from tissue_analysis_amd import _capi


def run(cfg, a):
    import torch
    sdtype = fb.signal_dtype(cfg)
    top = 1 << (8 * sdtype.itemsize)
    nvox = int(np.prod(cfg.dims))
    nbytes = nvox * (cfg.dtype.itemsize + 2 * sdtype.itemsize)
    with fb.resident(cfg) as (ctx, vol, L):
        g = torch.Generator(device="cuda").manual_seed(cfg.seed)
        chan_a = fb.random_signal(cfg.dims, sdtype.itemsize, g)
        chan_b = fb.random_signal(cfg.dims, sdtype.itemsize, g)
        torch.cuda.synchronize()
        ctx.extract(_capi.F_ALL, L)
        ctx.adjacency_size()
        _, probe_bps = fb.read_probe(ctx, vol)
        labels_only = lambda: ctx.signal_extract(_capi.SIG_LABELS)
        ctx.set_signal_device(chan_b.data_ptr(), sdtype.itemsize, keep=chan_b)
        sb = fb.timed(labels_only, ctx.signal_timing, a.reps)
        ctx.set_signal_device(chan_a.data_ptr(), sdtype.itemsize, keep=chan_a)
        sa = fb.timed(labels_only, ctx.signal_timing, a.reps)
        sdebug = ctx.signal_debug()
        ctx.set_cosignal_device(chan_b.data_ptr(), sdtype.itemsize, keep=chan_b)
        thr = top // 2
        ms = fb.timed(lambda: ctx.cosignal_extract(thr, thr), ctx.cosignal_timing, a.reps)
        debug = ctx.cosignal_debug()
    k, sa_ms, sb_ms = statistics.median(ms), statistics.median(sa), statistics.median(sb)
    s = (sa_ms + sb_ms) / 2
    return dict(config=cfg.name, dims=list(cfg.dims), labels=cfg.dtype.name, channels=sdtype.name, reps=a.reps,
                **fb.spread("kernel_ms", ms, ("min",)), signal_a_ms=round(sa_ms, 4), signal_b_ms=round(sb_ms, 4), signal_ms=round(s, 4),
                signal_ms_min=round((min(sa) + min(sb)) / 2, 4), ratio=round(k / s, 3), bytes=nbytes,
                signal_bytes=2 * nvox * (cfg.dtype.itemsize + sdtype.itemsize), read_probe_tbs=round(probe_bps / 1e12, 3),
                frac_read_probe=round(nbytes / (k * 1e-3) / probe_bps, 4), spills=debug["spills"],
                tiles_per_group=debug["tiles_per_group"], groups=debug["groups"], signal_label_spills=sdebug["label_spills"])


def main():
    fb.main(run, reps=30, configs="C4,512^3", out="profiles/cosignal_bench.jsonl", mode="a")


if __name__ == "__main__":
    main()
