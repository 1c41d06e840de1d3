#!/usr/bin/env python3
"""Extent pass throughput (include/tissue_scan_extents.h): one JSON line per configuration, appended to
profiles/extents_bench.jsonl.

    python scripts/bench_cell_extents.py [--reps 30] [--out profiles/extents_bench.jsonl]

  kernel_ms        median of the pass kernel's HIP-event durations (ta_extents_timing) over --reps passes, with every label's
                   principal axes as its directions; kernel_ms_min, kernel_ms_p25, kernel_ms_p75: the spread over the same passes
  sigmom_ms        the yardstick, in the same process on the same volume, its passes alternating with the extent passes: the
                   signal-moment pass (ta_sigmom_timing) with a random signal; _min, _p25, _p75 likewise
  ratio            kernel_ms / sigmom_ms
  bytes            algorithmic bytes of the extent pass: voxels x label itemsize (the yardstick reads the signal too: sigmom_bytes)
  frac_read_probe  bytes / kernel_ms against what ta_read_probe reaches on the same label buffer in this run
  spills           records that missed a workgroup's LDS table (ta_extents_debug); tiles_per_group, groups: its launch plan
Configurations: C4 (1024^3 uint32, 50k seeds; uint16 signal for the yardstick); 512^3 uint16 labels (uint8 signal)."""
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
from tissue_analysis_amd.cell_extents import extent_weights, principal_frames  # noqa: E402
from tissue_analysis_amd.extraction import Extraction  # noqa: E402


def alternating_ms(passes, reps):
    """passes: [(enqueue, timing)]; three warm-up rounds, then `reps` rounds that run each pass once, in turn.  One list of
    milliseconds per pass."""
    for _ in range(3):
        for enqueue, _ in passes:
            enqueue()
    ms = [[] for _ in passes]
    for _ in range(reps):
        for i, (enqueue, timing) in enumerate(passes):
            enqueue()
            ms[i].append(timing())
    return ms


def spread(prefix, ms):
    q = statistics.quantiles(ms, n=4)
    return {prefix: round(statistics.median(ms), 4), prefix + "_min": round(min(ms), 4), prefix + "_p25": round(q[0], 4),
            prefix + "_p75": round(q[2], 4)}


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
    count, bbox, sum1, sum2 = ctx.labels()
    none = np.zeros(0, dtype=np.uint32)
    x = Extraction(tuple(dims), L, count, bbox, sum1, sum2, none, none, np.zeros((0, 3), dtype=np.uint64))
    weights = extent_weights(principal_frames(x), perm=ctx.memory_axes())
    probe_ms = ctx.read_probe(vol.data_ptr(), vol.numel() * vol.element_size(), repeats=5)
    probe_bps = vol.numel() * vol.element_size() / (probe_ms * 1e-3)
    nbytes = int(np.prod(dims)) * ldtype.itemsize
    k, s = alternating_ms([(lambda: ctx.extents_extract(weights), ctx.extents_timing), (ctx.sigmom_extract, ctx.sigmom_timing)], reps)
    debug, sdebug = ctx.extents_debug(), ctx.sigmom_debug()
    lo, hi = ctx.extents_rows()
    ctx.close()
    del vol, sig
    torch.cuda.empty_cache()
    out = dict(config=name, dims=list(dims), labels=ldtype.name, signal=sdtype.name, reps=reps, rows=int(L) + 1,
               rows_with_voxels=int(np.isfinite(lo[:, 0]).sum()))
    out.update(spread("kernel_ms", k))
    out.update(spread("sigmom_ms", s))
    km, sm = statistics.median(k), statistics.median(s)
    out.update(ratio=round(km / sm, 3), bytes=nbytes, sigmom_bytes=int(np.prod(dims)) * (ldtype.itemsize + sdtype.itemsize),
               read_probe_tbs=round(probe_bps / 1e12, 3), frac_read_probe=round(nbytes / (km * 1e-3) / probe_bps, 4),
               spills=debug["spills"], tiles_per_group=debug["tiles_per_group"], groups=debug["groups"], sigmom_spills=sdebug["spills"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extents_bench.jsonl"))
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
