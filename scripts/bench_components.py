#!/usr/bin/env python3
"""Component-pass throughput (include/tissue_scan_components.h): one JSON line per configuration, also written to
profiles/components_bench.jsonl.

    python scripts/bench_components.py [--reps 10] [--configs C4,C4-tissue,512^3] [--out profiles/components_bench.jsonl]

  pass_ms          median of the HIP-event time of the kernels that walk the volume (local pass, seams, flatten and count, emit,
                   statistics; ta_components_timing)
  after_ms         median of everything after them: the scan of the counts, the sort keys, the radix sort, the table (it spans the
                   host's read of the slot count)
  components       rows of the table; labels: distinct labels among them; fragmented: labels of more than one component
  junction_walks_ms  the junction pass's two walks over the same buffer in this run (ta_junctions_timing): the other kernel
                   of this library that walks every voxel without the sweep's tables
  read_probe_ms    ta_read_probe on the same buffer in this run (one read of every label)
  pass_over_probe  pass_ms / read_probe_ms
C4-tissue is C4's volume without the ellipsoid mask: cells everywhere, no background around them."""
import statistics

import numpy as np

import featbench as fb


def run(cfg, a):
    with fb.resident(cfg) as (ctx, v, _):
        vol_bytes = v.numel() * v.element_size()
        probe_ms, probe_bps = fb.read_probe(ctx, v)
        last = {}

        def junctions():
            ctx.junctions_extract()
            ctx.junctions_size()

        def components():
            ctx.components_extract()
            last["rows"] = ctx.components_size()

        walks = [t[0] for t in fb.timed(junctions, ctx.junctions_timing, 3, warmup=0)]
        passes, after = zip(*fb.timed(components, ctx.components_timing, a.reps, warmup=1))
        label, n, first, bbox, sum1 = ctx.components_get()
    uniq, per = np.unique(label, return_counts=True)
    k = statistics.median(passes)
    return dict(config=cfg.name, dims=list(cfg.dims), labels_dtype=cfg.dtype.name, **fb.spread("pass_ms", passes),
                after_ms=round(statistics.median(after), 4), reps=a.reps, components=int(last["rows"]), labels=int(uniq.size),
                fragmented=int((per > 1).sum()), voxels=int(n.sum()), largest=int(n.max()),
                junction_walks_ms=round(statistics.median(walks), 4), read_probe_ms=round(probe_ms, 4),
                read_probe_tbs=round(probe_bps / 1e12, 3), pass_over_probe=round(k / probe_ms, 3),
                pass_over_junction_walks=round(k / statistics.median(walks), 3))


def main():
    fb.main(run, reps=10, configs="C4,C4-tissue,512^3", out="profiles/components_bench.jsonl", mode="w")


if __name__ == "__main__":
    main()
