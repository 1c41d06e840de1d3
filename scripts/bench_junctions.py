#!/usr/bin/env python3
"""Junction-pass throughput (include/tissue_scan_junctions.h): one JSON line per configuration, also written to
profiles/junctions_bench.jsonl.

    python scripts/bench_junctions.py [--reps 30] [--configs C4,512^3] [--out profiles/junctions_bench.jsonl]

  pass_ms          median of the HIP-event time of the two walks over the volume (counting + emitting; ta_junctions_timing)
  after_ms         median of everything after them: scans, sorts, row bounds, segmented reduce (it spans the host's read of the
                   row counts)
  records3/4       blocks of order 3 / 4 (one record each); edges / vertices: rows of the tables; degenerate: blocks of order >= 5
  bytes            algorithmic bytes of the pass: every label read once per walk, two walks
  frac_8tbs        bytes / pass_ms against 8 TB/s
  read_probe_ms    ta_read_probe on the same buffer in this run (one read of every label: the ceiling of ONE walk);
  pass_over_probe  pass_ms / read_probe_ms (2.0 would be two walks at the speed of the probe)
The parent's implementation of the same 2 x 2 x 2 walk is the corner-count kernel of the mesh extraction: take its time from
    rocprofv3 --kernel-trace --stats -- python scripts/bench_mesh.py --configs C4 --reps 3 --no-cpu
in a process of its own."""
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
            last["size"] = ctx.junctions_size()

        walks, after = zip(*fb.timed(junctions, ctx.junctions_timing, a.reps))
        E, V, degenerate = last["size"]
        (el, en, es), (vl, vn, vs), _ = ctx.junctions_get()
    k = statistics.median(walks)
    nbytes = 2 * vol_bytes
    blocks = int(np.prod([max(int(d) - 1, 1) for d in cfg.dims]))
    return dict(config=cfg.name, dims=list(cfg.dims), labels=cfg.dtype.name, **fb.spread("pass_ms", walks),
                after_ms=round(statistics.median(after), 4), reps=a.reps, blocks=blocks, records3=int(en.sum()), records4=int(vn.sum()),
                edges=int(E), vertices=int(V), degenerate=int(degenerate), bytes=nbytes, tb_per_s=round(nbytes / (k * 1e-3) / 1e12, 3),
                frac_8tbs=round(nbytes / (k * 1e-3) / fb.TBS, 4), read_probe_ms=round(probe_ms, 4),
                read_probe_tbs=round(probe_bps / 1e12, 3), pass_over_probe=round(k / probe_ms, 3))


def main():
    fb.main(run, reps=30, configs="C4,512^3", out="profiles/junctions_bench.jsonl", mode="w")


if __name__ == "__main__":
    main()
