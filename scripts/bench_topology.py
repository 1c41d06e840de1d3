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

HBM = 6.29e12


def run(name, dims, dtype, n_cells, seed, reps):
    import torch
    dtype = np.dtype(dtype)
    ctx = dev.torch_context(0)
    v, _ = dev.synth_slab(ctx, dims, dtype, n_cells, seed)
    torch.cuda.synchronize()
    ctx.set_volume_device(v.data_ptr(), dtype.itemsize, v.shape, keep=v)
    vol_bytes = v.numel() * v.element_size()
    probe_ms = ctx.read_probe(v.data_ptr(), vol_bytes, repeats=5)
    ctx.extract(_capi.F_VOLUME, ctx.max_label())
    ctx.labels()
    for _ in range(3):
        ctx.topology_extract()
        ctx.topology_debug()
        ctx.junctions_extract()
        ctx.junctions_size()
    ours, walks = [], []
    for _ in range(reps):                                     # the two passes take turns
        ctx.topology_extract()
        debug = ctx.topology_debug()
        ours.append(ctx.topology_timing())
        ctx.junctions_extract()
        ctx.junctions_size()
        walks.append(ctx.junctions_timing()[0])
    n0 = ctx.topology_rows()[0]
    assert int(n0.sum()) == v.numel()
    k, w = statistics.median(ours), statistics.median(walks) / 2
    line = dict(config=name, dims=list(dims), labels=dtype.name, pass_ms=round(k, 4), pass_ms_min=round(min(ours), 4),
                pass_ms_max=round(max(ours), 4), reps=reps, mvoxel_per_s=round(v.numel() / (k * 1e-3) / 1e6, 1), bytes=vol_bytes,
                tb_per_s=round(vol_bytes / (k * 1e-3) / 1e12, 3), frac_hbm=round(vol_bytes / (k * 1e-3) / HBM, 4),
                mixed=debug["mixed"], spills=debug["spills"], tiles_per_group=debug["tiles_per_group"], groups=debug["groups"],
                junction_walk_ms=round(w, 4), pass_over_walk=round(k / w, 3), read_probe_ms=round(probe_ms, 4))
    ctx.close()
    del v
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--configs", default="C2,C4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topology_bench.jsonl"))
    a = ap.parse_args()
    lines = []
    for name in a.configs.split(","):
        c = synth.CONFIGS[name]
        lines.append(run(name, c["dims"], c["dtype"], c["n_cells"], c["seed"], a.reps))
        print(json.dumps(lines[-1]), flush=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
