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

TBS = 8e12


def run(name, dims, dtype, n_cells, seed, reps, rounds):
    import torch
    dtype = np.dtype(dtype)
    ctx = dev.torch_context(0)
    vol, L = dev.synth_slab(ctx, dims, dtype, n_cells, seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    sig = torch.randint(0, 256, tuple(dims), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
    torch.cuda.synchronize()
    ctx.set_volume_device(vol.data_ptr(), dtype.itemsize, vol.shape, keep=vol)
    ctx.set_signal_device(sig.data_ptr(), 1, keep=sig)
    ctx.extract(_capi.F_ALL, L)
    pairs = ctx.adjacency_size()
    vol_bytes = vol.numel() * vol.element_size()
    geo, walls, probe = [], [], []
    for _ in range(rounds):
        for _ in range(3):
            ctx.wallgeo_extract()
        ms = []
        for _ in range(reps):
            ctx.wallgeo_extract()
            ms.append(ctx.wallgeo_timing())
        geo.append(statistics.median(ms))
        for _ in range(3):
            ctx.signal_extract(_capi.SIG_WALLS)
        ms = []
        for _ in range(reps):
            ctx.signal_extract(_capi.SIG_WALLS)
            ms.append(ctx.signal_timing())
        walls.append(statistics.median(ms))
        probe.append(ctx.read_probe(vol.data_ptr(), vol_bytes, repeats=5))
    spills = ctx.wallgeo_spills()
    fwd, rev, _, _ = ctx.wallgeo_get()
    k, w = statistics.median(geo), statistics.median(walls)
    line = dict(config=name, dims=list(dims), labels=dtype.name, reps=reps, rounds=rounds,
                geo_ms=[round(v, 4) for v in geo], signal_walls_ms=[round(v, 4) for v in walls],
                read_probe_ms=[round(v, 4) for v in probe], geo_ms_median=round(k, 4), signal_walls_ms_median=round(w, 4),
                ratio=round(k / w, 3), geo_spread=round((max(geo) - min(geo)) / k, 4), signal_spread=round((max(walls) - min(walls)) / w, 4),
                pairs=int(pairs), faces=int(fwd.sum() + rev.sum()), spills=int(spills), bytes=vol_bytes,
                frac_8tbs=round(vol_bytes / (k * 1e-3) / TBS, 4), geo_over_probe=round(k / statistics.median(probe), 3))
    ctx.close()
    del vol, sig
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--configs", default="C4,512^3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wall_geometry_bench.jsonl"))
    a = ap.parse_args()
    lines = []
    for name in a.configs.split(","):
        if name == "C4":
            c = synth.CONFIGS["C4"]
            lines.append(run("C4", c["dims"], c["dtype"], c["n_cells"], c["seed"], a.reps, a.rounds))
        else:
            c = synth.CONFIGS["C2"]
            lines.append(run("512^3", c["dims"], "uint16", c["n_cells"], c["seed"], a.reps, a.rounds))
        print(json.dumps(lines[-1]), flush=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
