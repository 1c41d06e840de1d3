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
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tissue_analysis_amd import _capi, synth  # noqa: E402
from tissue_analysis_amd import device as dev  # noqa: E402

EDGES = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, np.inf])          # distances in voxels: K = 8


def run(name, dims, dtype, n_cells, seed, reps):
    import torch
    dtype = np.dtype(dtype)
    ctx = dev.torch_context(0)
    v, _ = dev.synth_slab(ctx, dims, dtype, n_cells, seed)
    torch.cuda.synchronize()
    ctx.set_volume_device(v.data_ptr(), dtype.itemsize, v.shape, keep=v)
    nvox = v.numel()
    sig = torch.randint(-32768, 32767, tuple(v.shape), dtype=torch.int16, device=v.device)           # every uint16 bit pattern
    stand_in = torch.zeros((nvox,), dtype=torch.float64, device=v.device)
    torch.cuda.synchronize()
    probe = dict(labels=ctx.read_probe(v.data_ptr(), nvox * dtype.itemsize, repeats=5),
                 d2=ctx.read_probe(stand_in.data_ptr(), nvox * 8, repeats=5),
                 signal=ctx.read_probe(sig.data_ptr(), nvox * 2, repeats=5))
    del stand_in
    torch.cuda.empty_cache()
    ctx.set_signal_device(sig.data_ptr(), 2, keep=sig)
    ctx.extract(_capi.F_VOLUME, ctx.max_label())
    ctx.signal_extract(_capi.SIG_LABELS)
    ctx.signal_timing()
    signal_ms = []
    for _ in range(reps):
        ctx.signal_extract(_capi.SIG_LABELS)
        signal_ms.append(ctx.signal_timing())
    signal_ms = statistics.median(signal_ms)
    ctx.distance_extract(_capi.DIST_OWN_WALL, 0, (1.0, 1.0, 1.0), 0)
    lines = []
    for with_signal in (False, True):
        ctx.profile_extract(np.square(EDGES), with_signal)
        ctx.profile_timing()
        ms = []
        for _ in range(reps):
            ctx.profile_extract(np.square(EDGES), with_signal)
            ms.append(ctx.profile_timing())
        n = ctx.profile_get()[0]
        debug = ctx.profile_debug()
        k = statistics.median(ms)
        probe_ms = probe["labels"] + probe["d2"] + (probe["signal"] if with_signal else 0.0)
        nbytes = nvox * (dtype.itemsize + 8 + (2 if with_signal else 0))
        lines.append(dict(config=name, dims=list(dims), labels_dtype=dtype.name, signal_dtype="uint16" if with_signal else None,
                          shells=int(EDGES.size - 1), pass_ms=round(k, 4), pass_ms_min=round(min(ms), 4), pass_ms_max=round(max(ms), 4),
                          reps=reps, bytes=nbytes, bytes_per_voxel=nbytes // nvox, pass_tbs=round(nbytes / (k * 1e-3) / 1e12, 3),
                          read_probe_ms=round(probe_ms, 4), read_probe_tbs=round(nbytes / (probe_ms * 1e-3) / 1e12, 3),
                          pass_over_probe=round(k / probe_ms, 3), signal_pass_ms=round(signal_ms, 4),
                          pass_over_signal=round(k / signal_ms, 3), counted_voxels=int(n.sum()), voxels=nvox,
                          keys_in_use=int((n > 0).sum()), spills=debug["spills"], tiles_per_group=debug["tiles_per_group"],
                          groups=debug["groups"]))
    ctx.close()
    del v, sig
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--configs", default="C4,512^3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "profile_bench.jsonl"))
    a = ap.parse_args()
    lines = []
    for name in a.configs.split(","):
        if name == "C4":
            c = synth.CONFIGS["C4"]
            new = run(name, c["dims"], c["dtype"], c["n_cells"], c["seed"], a.reps)
        else:
            c = synth.CONFIGS["C2"]
            new = run("512^3", c["dims"], "uint16", c["n_cells"], c["seed"], a.reps)
        for d in new:
            print(json.dumps(d), flush=True)
        lines += new
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
