#!/usr/bin/env python3
"""Wall-geometry pass throughput (include/tissue_scan_wallgeo.h): one JSON line per configuration, also written to
profiles/wall_geometry_bench.jsonl.

    python scripts/bench_wall_geometry.py [--reps 30] [--rounds 2] [--configs C4,512^3] [--out profiles/wall_geometry_bench.jsonl]

The yardstick is the walls-only signal pass (ta_signal_extract(TA_SIG_WALLS), a uint8 signal): it finds the same faces and does
the same pair lookup, for 2 numbers a wall instead of 15.  The two passes and ta_read_probe take turns, `rounds` times, in
this one process on the same resident volume and extraction; every figure is a median of `reps` HIP-event timings.
  geo_ms           per round: median of ta_wallgeo_timing
  signal_walls_ms  per round: median of ta_signal_timing of the walls-only pass
  read_probe_ms    per round: ta_read_probe over the labels (one read of every label)
  ratio            median geo_ms / median signal_walls_ms
  spread           (max - min) / median of each pass's per-round medians
  pairs, faces     rows of the table, faces they hold; spills: records that missed the LDS table in the last pass"""
import statistics

import featbench as fb
from tissue_analysis_amd import _capi


def run(cfg, a):
    import torch
    with fb.resident(cfg) as (ctx, vol, L):
        sig = fb.random_signal(cfg.dims, 1, torch.Generator(device="cuda").manual_seed(cfg.seed))
        torch.cuda.synchronize()
        ctx.set_signal_device(sig.data_ptr(), 1, keep=sig)
        ctx.extract(_capi.F_ALL, L)
        pairs = ctx.adjacency_size()
        vol_bytes = vol.numel() * vol.element_size()
        geo, walls, probe = [], [], []
        for _ in range(a.rounds):
            geo.append(statistics.median(fb.timed(ctx.wallgeo_extract, ctx.wallgeo_timing, a.reps)))
            walls.append(statistics.median(fb.timed(lambda: ctx.signal_extract(_capi.SIG_WALLS), ctx.signal_timing, a.reps)))
            probe.append(fb.read_probe(ctx, vol)[0])
        spills = ctx.wallgeo_spills()
        fwd, rev, _, _ = ctx.wallgeo_get()
    k, w = statistics.median(geo), statistics.median(walls)
    return dict(config=cfg.name, dims=list(cfg.dims), labels=cfg.dtype.name, reps=a.reps, rounds=a.rounds,
                geo_ms=[round(v, 4) for v in geo], signal_walls_ms=[round(v, 4) for v in walls],
                read_probe_ms=[round(v, 4) for v in probe], geo_ms_median=round(k, 4), signal_walls_ms_median=round(w, 4),
                ratio=round(k / w, 3), geo_spread=round((max(geo) - min(geo)) / k, 4), signal_spread=round((max(walls) - min(walls)) / w, 4),
                pairs=int(pairs), faces=int(fwd.sum() + rev.sum()), spills=int(spills), bytes=vol_bytes,
                frac_8tbs=round(vol_bytes / (k * 1e-3) / fb.TBS, 4), geo_over_probe=round(k / statistics.median(probe), 3))


def main():
    fb.main(run, reps=30, configs="C4,512^3", out="profiles/wall_geometry_bench.jsonl", mode="w",
            extra_args=[("--rounds", dict(type=int, default=2))])


if __name__ == "__main__":
    main()
