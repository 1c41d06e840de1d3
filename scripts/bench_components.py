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


def run(name, dims, dtype, n_cells, seed, reps, ellipsoid=True):
    import torch
    dtype = np.dtype(dtype)
    ctx = dev.torch_context(0)
    v, _ = dev.synth_slab(ctx, dims, dtype, n_cells, seed, ellipsoid=ellipsoid)
    torch.cuda.synchronize()
    ctx.set_volume_device(v.data_ptr(), dtype.itemsize, v.shape, keep=v)
    vol_bytes = v.numel() * v.element_size()
    probe_ms = ctx.read_probe(v.data_ptr(), vol_bytes, repeats=5)
    walks = []
    for _ in range(3):
        ctx.junctions_extract()
        ctx.junctions_size()
        walks.append(ctx.junctions_timing()[0])
    ctx.components_extract()
    ctx.components_size()
    passes, after = [], []
    for _ in range(reps):
        ctx.components_extract()
        R = ctx.components_size()
        a, b = ctx.components_timing()
        passes.append(a)
        after.append(b)
    label, n, first, bbox, sum1 = ctx.components_get()
    uniq, per = np.unique(label, return_counts=True)
    k = statistics.median(passes)
    line = dict(config=name, dims=list(dims), labels_dtype=dtype.name, pass_ms=round(k, 4), pass_ms_min=round(min(passes), 4),
                pass_ms_max=round(max(passes), 4), after_ms=round(statistics.median(after), 4), reps=reps, components=int(R),
                labels=int(uniq.size), fragmented=int((per > 1).sum()), voxels=int(n.sum()), largest=int(n.max()),
                junction_walks_ms=round(statistics.median(walks), 4), read_probe_ms=round(probe_ms, 4),
                read_probe_tbs=round(vol_bytes / (probe_ms * 1e-3) / 1e12, 3), pass_over_probe=round(k / probe_ms, 3),
                pass_over_junction_walks=round(k / statistics.median(walks), 3))
    ctx.close()
    del v
    torch.cuda.empty_cache()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--configs", default="C4,C4-tissue,512^3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.jsonl"))
    a = ap.parse_args()
    lines = []
    for name in a.configs.split(","):
        if name in ("C4", "C4-tissue"):
            c = synth.CONFIGS["C4"]
            lines.append(run(name, c["dims"], c["dtype"], c["n_cells"], c["seed"], a.reps, ellipsoid=name == "C4"))
        else:
            c = synth.CONFIGS["C2"]
            lines.append(run("512^3", c["dims"], "uint16", c["n_cells"], c["seed"], a.reps))
        print(json.dumps(lines[-1]), flush=True)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
