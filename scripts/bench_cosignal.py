#!/usr/bin/env python3
"""Two-channel pass throughput (include/tissue_scan_cosignal.h): one JSON line per configuration, appended to
profiles/cosignal_bench.jsonl.

    python scripts/bench_cosignal.py [--reps 30] [--out profiles/cosignal_bench.jsonl]

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
    top = 1 << (8 * sdtype.itemsize)
    ctx = dev.torch_context(0)
    vol, L = dev.synth_slab(ctx, dims, ldtype, n_cells, seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    tdtype = torch.uint8 if sdtype.itemsize == 1 else torch.int16
    chan_a = torch.randint(0, top, tuple(dims), generator=g, device="cuda", dtype=torch.int32).to(tdtype)
    chan_b = torch.randint(0, top, tuple(dims), generator=g, device="cuda", dtype=torch.int32).to(tdtype)
    torch.cuda.synchronize()
    ctx.set_volume_device(vol.data_ptr(), ldtype.itemsize, vol.shape, keep=vol)
    ctx.extract(_capi.F_ALL, L)
    ctx.adjacency_size()
    probe_ms = ctx.read_probe(vol.data_ptr(), vol.numel() * vol.element_size(), repeats=5)
    probe_bps = vol.numel() * vol.element_size() / (probe_ms * 1e-3)
    nvox = int(np.prod(dims))
    nbytes = nvox * (ldtype.itemsize + 2 * sdtype.itemsize)
    labels_only = lambda: ctx.signal_extract(_capi.SIG_LABELS)
    ctx.set_signal_device(chan_b.data_ptr(), sdtype.itemsize, keep=chan_b)
    sb, sbmin = median_ms(labels_only, ctx.signal_timing, reps)
    ctx.set_signal_device(chan_a.data_ptr(), sdtype.itemsize, keep=chan_a)
    sa, samin = median_ms(labels_only, ctx.signal_timing, reps)
    sdebug = ctx.signal_debug()
    ctx.set_cosignal_device(chan_b.data_ptr(), sdtype.itemsize, keep=chan_b)
    thr = top // 2
    k, kmin = median_ms(lambda: ctx.cosignal_extract(thr, thr), ctx.cosignal_timing, reps)
    debug = ctx.cosignal_debug()
    ctx.close()
    del vol, chan_a, chan_b
    torch.cuda.empty_cache()
    s = (sa + sb) / 2
    return dict(config=name, dims=list(dims), labels=ldtype.name, channels=sdtype.name, reps=reps, kernel_ms=round(k, 4),
                kernel_ms_min=round(kmin, 4), signal_a_ms=round(sa, 4), signal_b_ms=round(sb, 4), signal_ms=round(s, 4),
                signal_ms_min=round((samin + sbmin) / 2, 4), ratio=round(k / s, 3), bytes=nbytes,
                signal_bytes=2 * nvox * (ldtype.itemsize + sdtype.itemsize), read_probe_tbs=round(probe_bps / 1e12, 3),
                frac_read_probe=round(nbytes / (k * 1e-3) / probe_bps, 4), spills=debug["spills"],
                tiles_per_group=debug["tiles_per_group"], groups=debug["groups"], signal_label_spills=sdebug["label_spills"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cosignal_bench.jsonl"))
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
