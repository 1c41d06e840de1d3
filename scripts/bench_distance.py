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
import statistics

import numpy as np

import featbench as fb
from tissue_analysis_amd import _capi, synth

WORK_CAP, STACK_ENTRY = 1 << 30, 20            # DIST_WORK_CAP, DIST_STACK_ENTRY of csrc/ta_distance.h


def batches(dims, batch=0):
    n0, n1, n2 = dims
    total = 0
    for length, columns in ((n1, n0 * n2), (n0, n1 * n2)):
        per = -(-batch // 64) * 64 if batch else max(64, WORK_CAP // (length * STACK_ENTRY) // 64 * 64)
        total += -(-columns // per)
    return total


def run(cfg, a):
    with fb.resident(cfg) as (ctx, v, _):
        nvox, item = v.numel(), cfg.dtype.itemsize
        probe_ms, probe_bps = fb.read_probe(ctx, v)
        ctx.extract(_capi.F_VOLUME, ctx.max_label())
        ctx.distance_set_batch(a.batch)
        for mode, mode_name in ((_capi.DIST_OWN_WALL, "own_wall"), (_capi.DIST_FROM_LABEL, "from_label")):
            distance = lambda: ctx.distance_extract(mode, synth.BACKGROUND, (1.0, 1.0, 1.0), 0)
            distance()
            ctx.distance_timing()
            passes, after = zip(*fb.timed(distance, ctx.distance_timing, a.reps, warmup=0))
            min2, max2, pole = ctx.distance_get()
            present = pole[:, 0] >= 0
            finite = present & np.isfinite(max2)
            yield dict(config=cfg.name, mode=mode_name, dims=list(cfg.dims), labels_dtype=cfg.dtype.name, **fb.spread("pass_ms", passes),
                       **fb.spread("after_ms", after), reps=a.reps, labels=int(present.sum()),
                       largest_radius=float(np.sqrt(max2[finite].max())) if finite.any() else None,
                       read_probe_ms=round(probe_ms, 4), read_probe_tbs=round(probe_bps / 1e12, 3),
                       pass_over_probe=round(statistics.median(passes) / probe_ms, 3), bytes_rows=nvox * (2 * item + 24),
                       bytes_columns=nvox * (2 * item + 32), bytes_table=nvox * 2 * (item + 8),
                       batches=batches(cfg.dims, a.batch), batch_columns=a.batch)


def main():
    fb.main(run, reps=10, configs="C4,C4-tissue,512^3", out="profiles/distance_bench.jsonl", mode="w",
            extra_args=[("--batch", dict(type=int, default=0))])


if __name__ == "__main__":
    main()
