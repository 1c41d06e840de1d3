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
import numpy as np

import featbench as fb
from tissue_analysis_amd import _capi, synth


def run(cfg, a):
    unit = (1.0, 1.0, 1.0)
    with fb.resident(cfg) as (ctx, v, _):
        top = ctx.max_label()
        lut = np.arange(top + 1, dtype=np.uint32)
        gone = np.arange(synth.BACKGROUND + 1, top + 1)[::a.erase]
        lut[gone] = 0
        ctx.relabel(lut)
        ctx.extract(_capi.F_VOLUME, top)
        nearest = lambda: ctx.nearest_extract(0, None, unit)
        nearest()
        ctx.nearest_timing()
        passes, after = zip(*fb.timed(nearest, ctx.nearest_timing, a.reps, warmup=0))
        gained, filled, remaining = ctx.nearest_get()
        launched = ctx.nearest_debug()
        distance = lambda: ctx.distance_extract(_capi.DIST_FROM_LABEL, synth.BACKGROUND, unit, 0)
        distance()
        ctx.distance_timing()
        d_passes, d_after = zip(*fb.timed(distance, ctx.distance_timing, a.reps, warmup=0))
    line = dict(config=cfg.name, dims=list(cfg.dims), labels_dtype=cfg.dtype.name, reps=a.reps, erased_labels=int(gone.size),
                filled=filled, remaining=remaining, labels_that_gained=int(np.count_nonzero(gained)),
                column_launches=launched["column_launches"], **fb.spread("pass_ms", passes), **fb.spread("after_ms", after),
                **fb.spread("distance_pass_ms", d_passes), **fb.spread("distance_after_ms", d_after))
    line["pass_over_distance"] = round(line["pass_ms"] / line["distance_pass_ms"], 3)
    return line


def main():
    fb.main(run, reps=10, configs="C4,512^3", out="profiles/nearest_bench.jsonl", mode="a",
            extra_args=[("--erase", dict(type=int, default=10))])


if __name__ == "__main__":
    main()
