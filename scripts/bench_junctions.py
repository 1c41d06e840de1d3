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
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tissue_analysis_amd import synth  # noqa: E402
from tissue_analysis_amd import device as dev  # noqa: E402

TBS = 8e12


def run(name, dims, dtype, n_cells, seed, reps):
    import torch
    dtype = np.dtype(dtype)
    ctx = dev.torch_context(0)
    v, _ = dev.synth_slab(ctx, dims, dtype, n_cells, seed)
    torch.cuda.synchronize()
    ctx.set_volume_device(v.data_ptr(), dtype.itemsize, v.shape, keep=v)
    vol_bytes = v.numel() * v.element_size()
    probe_ms = ctx.read_probe(v.data_ptr(), vol_bytes, repeats=5)
    for _ in range(3):
        ctx.junctions_extract()
        ctx.junctions_size()
    walks, after = [], []
    for _ in range(reps):
        ctx.junctions_extract()
        E, V, degenerate = ctx.junctions_size()
        a, b = ctx.junctions_timing()
        walks.append(a)
        after.append(b)
    (el, en, es), (vl, vn, vs), _ = ctx.junctions_get()
    k = statistics.median(walks)
    nbytes = 2 * vol_bytes
    blocks = int(np.prod([max(int(d) - 1, 1) for d in dims]))
    line = dict(config=name, dims=list(dims), labels=dtype.name, pass_ms=round(k, 4), pass_ms_min=round(min(walks), 4),
                pass_ms_max=round(max(walks), 4), after_ms=round(statistics.median(after), 4), reps=reps, blocks=blocks,
                records3=int(en.sum()), records4=int(vn.sum()), edges=int(E), vertices=int(V), degenerate=int(degenerate),
                bytes=nbytes, tb_per_s=round(nbytes / (k * 1e-3) / 1e12, 3), frac_8tbs=round(nbytes / (k * 1e-3) / TBS, 4),
                read_probe_ms=round(probe_ms, 4), read_probe_tbs=round(vol_bytes / (probe_ms * 1e-3) / 1e12, 3),
                pass_over_probe=round(k / probe_ms, 3))
    ctx.close()
    del v
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--configs", default="C4,512^3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "junctions_bench.jsonl"))
    a = ap.parse_args()
    lines = []
    for name in a.configs.split(","):
        if name == "C4":
            c = synth.CONFIGS["C4"]
            lines.append(run("C4", c["dims"], c["dtype"], c["n_cells"], c["seed"], a.reps))
        else:
            c = synth.CONFIGS["C2"]
            lines.append(run("512^3", c["dims"], "uint16", c["n_cells"], c["seed"], a.reps))
        print(json.dumps(lines[-1]), flush=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
