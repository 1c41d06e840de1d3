#!/usr/bin/env python3
"""Nearest-label throughput (include/tissue_scan_nearest.h) beside the distance pass on the same volume: one JSON line per
configuration, also appended to profiles/nearest_bench.jsonl.

    python scripts/bench_nearest.py [--reps 10] [--configs C4,512^3] [--erase 10] [--out profiles/nearest_bench.jsonl]

The volume is the benchmark's tissue with every `--erase`-th cell label erased to 0 (about 10 % of them); the nearest-label pass
fills the voxels of 0 from all others, the distance pass is ta_distance_extract in mode 1 from the background, in the same session.

  pass_ms            median of the HIP-event time of the row pass and the two column passes (ta_nearest_timing), with its range
  after_ms           median of the counting pass, with its range
  distance_pass_ms   the same of ta_distance_timing's three passes; distance_after_ms: its two table passes
  pass_over_distance pass_ms / distance_pass_ms.  The distance pass moves 20-byte stack entries and 8 bytes a voxel beside the
                     labels, this one 24-byte entries and 12 bytes a voxel and does not read the labels in its column passes
  filled, remaining  the two totals; erased_labels: how many labels were erased
The split between the row pass and the column passes needs a kernel trace; this script does not make one."""
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


def spread(values, name):
    return {name: round(statistics.median(values), 4), name + "_min": round(min(values), 4), name + "_max": round(max(values), 4)}


def run(name, dims, dtype, n_cells, seed, reps, erase):
    import torch
    dtype = np.dtype(dtype)
    ctx = dev.torch_context(0)
    v, _ = dev.synth_slab(ctx, dims, dtype, n_cells, seed)
    torch.cuda.synchronize()
    ctx.set_volume_device(v.data_ptr(), dtype.itemsize, v.shape, keep=v)
    top = ctx.max_label()
    lut = np.arange(top + 1, dtype=np.uint32)
    gone = np.arange(synth.BACKGROUND + 1, top + 1)[::erase]
    lut[gone] = 0
    ctx.relabel(lut)
    ctx.extract(_capi.F_VOLUME, top)
    unit = (1.0, 1.0, 1.0)
    ctx.nearest_extract(0, None, unit)
    ctx.nearest_timing()
    passes, after = [], []
    for _ in range(reps):
        ctx.nearest_extract(0, None, unit)
        a, b = ctx.nearest_timing()
        passes.append(a)
        after.append(b)
    gained, filled, remaining = ctx.nearest_get()
    launched = ctx.nearest_debug()
    ctx.distance_extract(_capi.DIST_FROM_LABEL, synth.BACKGROUND, unit, 0)
    ctx.distance_timing()
    d_passes, d_after = [], []
    for _ in range(reps):
        ctx.distance_extract(_capi.DIST_FROM_LABEL, synth.BACKGROUND, unit, 0)
        a, b = ctx.distance_timing()
        d_passes.append(a)
        d_after.append(b)
    line = dict(config=name, dims=list(dims), labels_dtype=dtype.name, reps=reps, erased_labels=int(gone.size), filled=filled,
                remaining=remaining, labels_that_gained=int(np.count_nonzero(gained)), column_launches=launched["column_launches"])
    line.update(spread(passes, "pass_ms"))
    line.update(spread(after, "after_ms"))
    line.update(spread(d_passes, "distance_pass_ms"))
    line.update(spread(d_after, "distance_after_ms"))
    line["pass_over_distance"] = round(line["pass_ms"] / line["distance_pass_ms"], 3)
    ctx.close()
    del v
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--configs", default="C4,512^3")
    ap.add_argument("--erase", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_bench.jsonl"))
    a = ap.parse_args()
    for name in a.configs.split(","):
        c = synth.CONFIGS["C4" if name == "C4" else "C2"]
        line = run(name, c["dims"], c["dtype"] if name == "C4" else "uint16", c["n_cells"], c["seed"], a.reps, a.erase)
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
