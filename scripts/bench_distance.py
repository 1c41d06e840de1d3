#!/usr/bin/env python3
"""Distance-map throughput (include/tissue_scan_distance.h): one JSON line per configuration and mode, also written to
profiles/distance_bench.jsonl.

    python scripts/bench_distance.py [--reps 10] [--configs C4,C4-tissue,512^3] [--batch 0] [--out profiles/distance_bench.jsonl]

  pass_ms          median of the HIP-event time of the row pass and the two column passes (ta_distance_timing), with its range
  after_ms         median of the two table passes, with its range
  read_probe_ms    ta_read_probe on the same label buffer in this run (one read of every label)
  pass_over_probe  pass_ms / read_probe_ms
  bytes_rows / bytes_columns / bytes_table
                   what the row pass, ONE column pass and the two table passes move by their loads and stores of labels and
                   float64 distances; the envelope stacks of the column passes (up to 20 bytes written per voxel and pass, read back
                   only where an entry is popped or used) are not in it
  batches          launches of the two column passes (the work buffer of the envelope stacks is capped, ta_distance.h);
                   batch_columns: --batch, the columns of a launch handed to ta_distance_set_batch (0 = the cap decides)
The split between the row pass, the column passes and the table passes needs a kernel trace; this script does not make one.
C4-tissue is C4's volume without the ellipsoid mask: cells everywhere, no background around them."""
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

WORK_CAP, STACK_ENTRY = 1 << 30, 20            # DIST_WORK_CAP, DIST_STACK_ENTRY of csrc/ta_distance.h


def batches(dims, batch=0):
    n0, n1, n2 = dims
    total = 0
    for length, columns in ((n1, n0 * n2), (n0, n1 * n2)):
        per = -(-batch // 64) * 64 if batch else max(64, WORK_CAP // (length * STACK_ENTRY) // 64 * 64)
        total += -(-columns // per)
    return total


def run(name, dims, dtype, n_cells, seed, reps, ellipsoid=True, batch=0):
    import torch
    dtype = np.dtype(dtype)
    ctx = dev.torch_context(0)
    v, _ = dev.synth_slab(ctx, dims, dtype, n_cells, seed, ellipsoid=ellipsoid)
    torch.cuda.synchronize()
    ctx.set_volume_device(v.data_ptr(), dtype.itemsize, v.shape, keep=v)
    nvox = v.numel()
    vol_bytes = nvox * v.element_size()
    probe_ms = ctx.read_probe(v.data_ptr(), vol_bytes, repeats=5)
    ctx.extract(_capi.F_VOLUME, ctx.max_label())
    ctx.distance_set_batch(batch)
    lines = []
    for mode, mode_name in ((_capi.DIST_OWN_WALL, "own_wall"), (_capi.DIST_FROM_LABEL, "from_label")):
        ctx.distance_extract(mode, synth.BACKGROUND, (1.0, 1.0, 1.0), 0)
        ctx.distance_timing()
        passes, after = [], []
        for _ in range(reps):
            ctx.distance_extract(mode, synth.BACKGROUND, (1.0, 1.0, 1.0), 0)
            a, b = ctx.distance_timing()
            passes.append(a)
            after.append(b)
        min2, max2, pole = ctx.distance_get()
        present = pole[:, 0] >= 0
        finite = present & np.isfinite(max2)
        k = statistics.median(passes)
        lines.append(dict(config=name, mode=mode_name, dims=list(dims), labels_dtype=dtype.name, pass_ms=round(k, 4),
                          pass_ms_min=round(min(passes), 4), pass_ms_max=round(max(passes), 4), after_ms=round(statistics.median(after), 4),
                          after_ms_min=round(min(after), 4), after_ms_max=round(max(after), 4), reps=reps, labels=int(present.sum()),
                          largest_radius=float(np.sqrt(max2[finite].max())) if finite.any() else None,
                          read_probe_ms=round(probe_ms, 4), read_probe_tbs=round(vol_bytes / (probe_ms * 1e-3) / 1e12, 3),
                          pass_over_probe=round(k / probe_ms, 3), bytes_rows=nvox * (2 * dtype.itemsize + 24),
                          bytes_columns=nvox * (2 * dtype.itemsize + 32), bytes_table=nvox * 2 * (dtype.itemsize + 8),
                          batches=batches(dims, batch), batch_columns=batch))
    ctx.close()
    del v
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--configs", default="C4,C4-tissue,512^3")
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_bench.jsonl"))
    a = ap.parse_args()
    lines = []
    for name in a.configs.split(","):
        if name in ("C4", "C4-tissue"):
            c = synth.CONFIGS["C4"]
            new = run(name, c["dims"], c["dtype"], c["n_cells"], c["seed"], a.reps, ellipsoid=name == "C4", batch=a.batch)
        else:
            c = synth.CONFIGS["C2"]
            new = run("512^3", c["dims"], "uint16", c["n_cells"], c["seed"], a.reps, batch=a.batch)
        for d in new:
            print(json.dumps(d), flush=True)
        lines += new
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
