#!/usr/bin/env python3
"""Signal-pass throughput (include/tissue_scan_signal.h): one JSON line per configuration.

    python scripts/bench_signal.py [--reps 30] [--configs C4,512^3] [--out FILE]

  kernel_ms        median of the pass kernel's HIP-event durations (ta_signal_timing) over --reps passes
  bytes            algorithmic bytes: voxels x (label itemsize + signal itemsize)
  frac_8tbs        bytes / kernel_ms against 8 TB/s
  frac_read_probe  ... against what ta_read_probe reaches on the same label buffer in this run
Configurations: C4 (1024^3 uint32, 50k seeds) with a uint16 signal -- labels only, walls only, both; 512^3 uint16 labels
with a uint8 signal (both); and, for context, scipy.ndimage.mean on a 256^3 crop of C4 on one CPU core."""
import statistics
import time

import numpy as np

import featbench as fb
from tissue_analysis_amd import _capi

CROP = {}                       # C4's 256^3 corner of labels and signal, for the CPU line


def run(cfg, a):
    import torch
    B, W = _capi.SIG_LABELS, _capi.SIG_WALLS
    whats = (("labels", B), ("walls", W), ("both", B | W)) if cfg.name == "C4" else (("both", B | W),)
    sdtype = fb.signal_dtype(cfg)
    with fb.resident(cfg) as (ctx, vol, L):
        sig = fb.random_signal(cfg.dims, sdtype.itemsize, torch.Generator(device="cuda").manual_seed(cfg.seed))
        torch.cuda.synchronize()
        ctx.set_signal_device(sig.data_ptr(), sdtype.itemsize, keep=sig)
        ctx.extract(_capi.F_ALL, L)
        ctx.adjacency_size()
        _, probe_bps = fb.read_probe(ctx, vol)
        nbytes = int(np.prod(cfg.dims)) * (cfg.dtype.itemsize + sdtype.itemsize)
        for label, what in whats:
            ms = fb.timed(lambda: ctx.signal_extract(what), ctx.signal_timing, a.reps)
            bps = nbytes / (statistics.median(ms) * 1e-3)
            yield dict(config=cfg.name, what=label, dims=list(cfg.dims), labels=cfg.dtype.name, signal=sdtype.name,
                       **fb.spread("kernel_ms", ms, ("min",)), reps=a.reps, bytes=nbytes, frac_8tbs=round(bps / fb.TBS, 4),
                       read_probe_tbs=round(probe_bps / 1e12, 3), frac_read_probe=round(bps / probe_bps, 4))
        if cfg.name == "C4":
            CROP.update(labels=vol[:256, :256, :256].cpu().numpy().view(cfg.dtype), signal=sig[:256, :256, :256].cpu().numpy().view(sdtype))


def cpu_line(a):
    if not CROP:
        return []
    from scipy import ndimage
    labels, signal = CROP.pop("labels"), CROP.pop("signal")           # taken: a later call in this process starts without a crop
    idx = np.unique(labels)
    t0 = time.perf_counter()
    ndimage.mean(signal, labels, idx)
    cpu = (time.perf_counter() - t0) * 1e3
    return dict(config="C4 crop 256^3", what="scipy.ndimage.mean, 1 CPU core", labels=int(idx.size), cpu_ms=round(cpu, 1))


def main():
    fb.main(run, reps=30, configs="C4,512^3", out=None, mode="w", after=cpu_line)


if __name__ == "__main__":
    main()
