#!/usr/bin/env python3
"""Signal-moment pass throughput (include/tissue_scan_sigmoments.h): one JSON line per configuration, appended to
profiles/sigmoments_bench.jsonl.

    python scripts/bench_signal_moments.py [--reps 30] [--out profiles/sigmoments_bench.jsonl]

  kernel_ms        median of the pass kernel's HIP-event durations (ta_sigmom_timing) over --reps passes
  signal_ms        the yardstick, in the same process on the same volume and signal: the labels-only signal pass
                   (ta_signal_timing of TA_SIG_LABELS), median over --reps passes
  ratio            kernel_ms / signal_ms
  bytes            algorithmic bytes: voxels x (label itemsize + signal itemsize)
  frac_read_probe  bytes / kernel_ms against what ta_read_probe reaches on the same label buffer in this run
  spills           records that missed a workgroup's LDS table (ta_sigmom_debug); tiles_per_group, groups: its launch plan
Configurations: C4 (1024^3 uint32, 50k seeds) with a uint16 signal; 512^3 uint16 labels with a uint8 signal."""
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


def median_ms(enqueue, timing, reps):
    for _ in range(3):
        enqueue()
    ms = []
    for _ in range(reps):
        enqueue()
        ms.append(timing())
    return statistics.median(ms), min(ms)


def run(name, dims, ldtype, n_cells, seed, sdtype, reps):
    import torch
    ldtype, sdtype = np.dtype(ldtype), np.dtype(sdtype)
    ctx = dev.torch_context(0)
    vol, L = dev.synth_slab(ctx, dims, ldtype, n_cells, seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    sig = torch.randint(0, 1 << (8 * sdtype.itemsize), tuple(dims), generator=g, device="cuda", dtype=torch.int32).to(
        torch.uint8 if sdtype.itemsize == 1 else torch.int16)
    torch.cuda.synchronize()
    ctx.set_volume_device(vol.data_ptr(), ldtype.itemsize, vol.shape, keep=vol)
    ctx.set_signal_device(sig.data_ptr(), sdtype.itemsize, keep=sig)
    ctx.extract(_capi.F_ALL, L)
    ctx.adjacency_size()
    probe_ms = ctx.read_probe(vol.data_ptr(), vol.numel() * vol.element_size(), repeats=5)
    probe_bps = vol.numel() * vol.element_size() / (probe_ms * 1e-3)
    nbytes = int(np.prod(dims)) * (ldtype.itemsize + sdtype.itemsize)
    k, kmin = median_ms(ctx.sigmom_extract, ctx.sigmom_timing, reps)
    debug = ctx.sigmom_debug()
    s, smin = median_ms(lambda: ctx.signal_extract(_capi.SIG_LABELS), ctx.signal_timing, reps)
    sdebug = ctx.signal_debug()
    ctx.close()
    del vol, sig
    torch.cuda.empty_cache()
    return dict(config=name, dims=list(dims), labels=ldtype.name, signal=sdtype.name, reps=reps, kernel_ms=round(k, 4),
                kernel_ms_min=round(kmin, 4), signal_ms=round(s, 4), signal_ms_min=round(smin, 4), ratio=round(k / s, 3),
                bytes=nbytes, read_probe_tbs=round(probe_bps / 1e12, 3), frac_read_probe=round(nbytes / (k * 1e-3) / probe_bps, 4),
                signal_frac_read_probe=round(nbytes / (s * 1e-3) / probe_bps, 4), spills=debug["spills"],
                tiles_per_group=debug["tiles_per_group"], groups=debug["groups"], signal_label_spills=sdebug["label_spills"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sigmoments_bench.jsonl"))
    a = ap.parse_args()
    c4, c2 = synth.CONFIGS["C4"], synth.CONFIGS["C2"]
    lines = [run("C4", c4["dims"], c4["dtype"], c4["n_cells"], c4["seed"], np.uint16, a.reps),
             run("512^3", c2["dims"], "uint16", c2["n_cells"], c2["seed"], np.uint8, a.reps)]
    with open(a.out, "a") as f:
        for d in lines:
            print(json.dumps(d))
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
