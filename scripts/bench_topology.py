#!/usr/bin/env python3
"""Euler-number pass throughput (include/tissue_scan_topology.h): one JSON line per configuration, also written to
profiles/topology_bench.jsonl.

    python scripts/bench_topology.py [--reps 30] [--configs C2,C4] [--out profiles/topology_bench.jsonl]

  pass_ms            median of the HIP-event time of the pass kernel (ta_topology_timing)
  mvoxel_per_s       voxels / pass_ms
  bytes, frac_hbm    algorithmic bytes of the pass (every label read once) and bytes / pass_ms against the 6.29 TB/s a float4 copy
                     reaches on the MI355X
  mixed, spills      blocks of more than one label; records that missed a workgroup's LDS table
  junction_walk_ms   the yardstick, measured in the same run on the same buffer: half the median HIP-event time of the junction
                     pass's two walks over the same 2 x 2 x 2 blocks (counting + emitting; ta_junctions_timing)
  pass_over_walk     pass_ms / junction_walk_ms
  read_probe_ms      ta_read_probe on the same buffer (one read of every label)"""
import statistics

import featbench as fb
from tissue_analysis_amd import _capi


def run(cfg, a):
    with fb.resident(cfg) as (ctx, v, _):
        vol_bytes = v.numel() * v.element_size()
        probe_ms, _ = fb.read_probe(ctx, v)
        ctx.extract(_capi.F_VOLUME, ctx.max_label())
        ctx.labels()
        last = {}

        def topology():
            ctx.topology_extract()
            last["debug"] = ctx.topology_debug()

        def junctions():
            ctx.junctions_extract()
            ctx.junctions_size()

        ours, walks = fb.alternating_ms([(topology, ctx.topology_timing), (junctions, lambda: ctx.junctions_timing()[0])], a.reps)
        debug = last["debug"]
        n0 = ctx.topology_rows()[0]
        assert int(n0.sum()) == v.numel()
        k, w = statistics.median(ours), statistics.median(walks) / 2
        return dict(config=cfg.name, dims=list(cfg.dims), labels=cfg.dtype.name, **fb.spread("pass_ms", ours), reps=a.reps,
                    mvoxel_per_s=round(v.numel() / (k * 1e-3) / 1e6, 1), bytes=vol_bytes, tb_per_s=round(vol_bytes / (k * 1e-3) / 1e12, 3),
                    frac_hbm=round(vol_bytes / (k * 1e-3) / fb.FLOAT4_COPY_BPS, 4), mixed=debug["mixed"], spills=debug["spills"],
                    tiles_per_group=debug["tiles_per_group"], groups=debug["groups"], junction_walk_ms=round(w, 4),
                    pass_over_walk=round(k / w, 3), read_probe_ms=round(probe_ms, 4))


def main():
    fb.main(run, reps=30, configs="C2,C4", out="profiles/topology_bench.jsonl", mode="w")


if __name__ == "__main__":
    main()
