#!/usr/bin/env python3
"""Signal-pass throughput (include/tissue_scan_signal.h): one JSON line per configuration.

    python scripts/bench_signal.py [--reps 30]

  kernel_ms        median of the pass kernel's HIP-event durations (ta_signal_timing) over --reps passes
  bytes            algorithmic bytes: voxels x (label itemsize + signal itemsize)
  frac_8tbs        bytes / kernel_ms against 8 TB/s
  frac_read_probe  ... against what ta_read_probe reaches on the same label buffer in this run
Configurations: C4 (1024^3 uint32, 50k seeds) with a uint16 signal -- labels only, walls only, both; 512^3 uint16 labels
with a uint8 signal (both); and, for context, scipy.ndimage.mean on a 256^3 crop of C4 on one CPU core."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tissue_analysis_amd import _capi, synth  # noqa: E402
from tissue_analysis_amd import device as dev  # noqa: E402

TBS = 8e12


def run(name, dims, ldtype, n_cells, seed, sdtype, reps, whats):
    import torch
    ldtype, sdtype = np.dtype(ldtype), np.dtype(sdtype)
    ctx = dev.torch_context(0)
    vol, L = dev.synth_slab(ctx, dims, ldtype, n_cells, seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    hi = 1 << (8 * sdtype.itemsize)
    sig = torch.randint(0, hi, tuple(dims), generator=g, device="cuda", dtype=torch.int32).to(
        torch.uint8 if sdtype.itemsize == 1 else torch.int16)
    torch.cuda.synchronize()
    ctx.set_volume_device(vol.data_ptr(), ldtype.itemsize, vol.shape, keep=vol)
    ctx.set_signal_device(sig.data_ptr(), sdtype.itemsize, keep=sig)
    ctx.extract(_capi.F_ALL, L)
    ctx.adjacency_size()
    probe_ms = ctx.read_probe(vol.data_ptr(), vol.numel() * vol.element_size(), repeats=5)
    probe_bps = vol.numel() * vol.element_size() / (probe_ms * 1e-3)
    nvox = int(np.prod(dims))
    nbytes = nvox * (ldtype.itemsize + sdtype.itemsize)
    out = []
    for label, what in whats:
        for _ in range(3):
            ctx.signal_extract(what)
        ms = []
        for _ in range(reps):
            ctx.signal_extract(what)
            ms.append(ctx.signal_timing())
        k = statistics.median(ms)
        bps = nbytes / (k * 1e-3)
        out.append(dict(config=name, what=label, dims=list(dims), labels=ldtype.name, signal=sdtype.name, kernel_ms=round(k, 4),
                        kernel_ms_min=round(min(ms), 4), reps=reps, bytes=nbytes, frac_8tbs=round(bps / TBS, 4),
                        read_probe_tbs=round(probe_bps / 1e12, 3), frac_read_probe=round(bps / probe_bps, 4)))
    host = vol[:256, :256, :256].cpu().numpy().view(ldtype) if name == "C4" else None
    shost = sig[:256, :256, :256].cpu().numpy().view(sdtype) if name == "C4" else None
    ctx.close()
    del vol, sig
    torch.cuda.empty_cache()
    return out, host, shost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    B, W = _capi.SIG_LABELS, _capi.SIG_WALLS
    c4 = synth.CONFIGS["C4"]
    lines, crop, scrop = run("C4", c4["dims"], c4["dtype"], c4["n_cells"], c4["seed"], np.uint16, a.reps,
                             (("labels", B), ("walls", W), ("both", B | W)))
    c2 = synth.CONFIGS["C2"]
    more, _, _ = run("512^3", c2["dims"], "uint16", c2["n_cells"], c2["seed"], np.uint8, a.reps, (("both", B | W),))
    for d in lines + more:
        print(json.dumps(d))
    from scipy import ndimage
    idx = np.unique(crop)
    t0 = time.perf_counter()
    ndimage.mean(scrop, crop, idx)
    cpu = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(config="C4 crop 256^3", what="scipy.ndimage.mean, 1 CPU core", labels=int(idx.size), cpu_ms=round(cpu, 1))))


if __name__ == "__main__":
    main()
