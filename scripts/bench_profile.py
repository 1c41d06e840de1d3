#!/usr/bin/env python3
"""Distance-shell profile throughput (include/tissue_scan_profile.h): one JSON line per configuration, with and without a uint16
signal, also written to profiles/profile_bench.jsonl.

    python scripts/bench_profile.py [--reps 10] [--configs C4,512^3] [--out profiles/profile_bench.jsonl]

  pass_ms          median of the HIP-event time of the pass kernel (ta_profile_timing) over K = 8 shells of the own-wall distance
                   map, with its range
  read_probe_ms    the sum of ta_read_probe over the buffers the pass must read, in this run: the labels, a float64 buffer of the
                   size of the D2 image (the image itself has no public device pointer; the stand-in is freed before the passes
                   are timed) and, with a signal, the signal
  bytes            what the pass must move: labels + 8 bytes of D2 (+ 2 of signal) a voxel
  pass_over_probe  pass_ms / read_probe_ms
  signal_pass_ms   median of the labels-only signal pass (ta_signal_timing, TA_SIG_LABELS) on the same volume and signal in this run;
                   pass_over_signal = pass_ms / signal_pass_ms
  spills           records that found no slot in a workgroup's LDS table (ta_profile_debug)"""
import statistics

import numpy as np

import featbench as fb
from tissue_analysis_amd import _capi

EDGES = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, np.inf])          # distances in voxels: K = 8


def run(cfg, a):
    import torch
    item = cfg.dtype.itemsize
    with fb.resident(cfg) as (ctx, v, _):
        nvox = v.numel()
        sig = torch.randint(-32768, 32767, tuple(v.shape), dtype=torch.int16, device=v.device)           # every uint16 bit pattern
        stand_in = torch.zeros((nvox,), dtype=torch.float64, device=v.device)
        torch.cuda.synchronize()
        probe = dict(labels=fb.read_probe(ctx, v)[0], d2=fb.read_probe(ctx, stand_in)[0], signal=fb.read_probe(ctx, sig)[0])
        del stand_in
        torch.cuda.empty_cache()
        ctx.set_signal_device(sig.data_ptr(), 2, keep=sig)
        ctx.extract(_capi.F_VOLUME, ctx.max_label())
        labels_only = lambda: ctx.signal_extract(_capi.SIG_LABELS)
        labels_only()
        ctx.signal_timing()
        signal_ms = statistics.median(fb.timed(labels_only, ctx.signal_timing, a.reps, warmup=0))
        ctx.distance_extract(_capi.DIST_OWN_WALL, 0, (1.0, 1.0, 1.0), 0)
        for with_signal in (False, True):
            profile = lambda: ctx.profile_extract(np.square(EDGES), with_signal)
            profile()
            ctx.profile_timing()
            ms = fb.timed(profile, ctx.profile_timing, a.reps, warmup=0)
            n = ctx.profile_get()[0]
            debug = ctx.profile_debug()
            k = statistics.median(ms)
            probe_ms = probe["labels"] + probe["d2"] + (probe["signal"] if with_signal else 0.0)
            nbytes = nvox * (item + 8 + (2 if with_signal else 0))
            yield dict(config=cfg.name, dims=list(cfg.dims), labels_dtype=cfg.dtype.name, signal_dtype="uint16" if with_signal else None,
                       shells=int(EDGES.size - 1), **fb.spread("pass_ms", ms), reps=a.reps, bytes=nbytes, bytes_per_voxel=nbytes // nvox,
                       pass_tbs=round(nbytes / (k * 1e-3) / 1e12, 3), read_probe_ms=round(probe_ms, 4),
                       read_probe_tbs=round(nbytes / (probe_ms * 1e-3) / 1e12, 3), pass_over_probe=round(k / probe_ms, 3),
                       signal_pass_ms=round(signal_ms, 4), pass_over_signal=round(k / signal_ms, 3), counted_voxels=int(n.sum()),
                       voxels=nvox, keys_in_use=int((n > 0).sum()), spills=debug["spills"], tiles_per_group=debug["tiles_per_group"],
                       groups=debug["groups"])


def main():
    fb.main(run, reps=10, configs="C4,512^3", out="profiles/profile_bench.jsonl", mode="w")


if __name__ == "__main__":
    main()
