#!/usr/bin/env python3
"""Resample-pass throughput (include/tissue_scan_resample.h): one JSON line per configuration and map, also written to
profiles/resample_bench.jsonl.

    python scripts/bench_resample.py [--reps 20] [--lut-stats kernel_stats.csv] [--out profiles/resample_bench.jsonl]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_resample.py --lut-only

  kernel_ms        median of the gather kernel's HIP-event durations (ta_resample_timing) over --reps passes, after 3 warm-up passes
  bytes            output bytes + source bytes (what the issue calls "one read, one write"; a zoom reads less, a rotation more lines)
  gb_per_s         bytes / kernel_ms
  lut_sweep_ms     the yardstick: ta_volume_map's kernel (map_kernel) on the same volume and type, one read and one write of the
                   same bytes.  ta_volume_map has no event timing of its own (it allocates, sweeps and copies to the host in one
                   call), so its kernel time comes from a kernel trace of `--lut-only` (the second command above, the mean of its
                   launches), handed in with --lut-stats; without it the fields are null.
  ratio_to_lut     kernel_ms / lut_sweep_ms
  read_probe_ms    ta_read_probe on the label buffer in this run (read only), for context
Configurations: 512^3 uint16 and 1024^3 uint32 targets from equal-size sources (a second frame of the synthetic tissue), nearest
neighbour; identity, a 10 degree rotation about each axis through the centre, a 2 x zoom; 512^3 also trilinear (uint16)."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tissue_analysis_amd import _capi, synth  # noqa: E402
from tissue_analysis_amd import device as dev  # noqa: E402

CONFIGS = (("512^3", "C2", "uint16"), ("1024^3", "C4", "uint32"))


def about_centre(linear, dims):
    """s = L (i - c) + c as a 3 x 4 index matrix, c the centre of the volume."""
    c = (np.asarray(dims, dtype=np.float64) - 1.0) / 2.0
    A = np.zeros((3, 4))
    A[:, :3] = linear
    A[:, 3] = c - linear @ c
    return A


def rotation(axis, degrees):
    t = np.deg2rad(degrees)
    c, s = np.cos(t), np.sin(t)
    R = np.eye(3)
    i, j = [k for k in range(3) if k != axis]
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def maps(dims):
    yield "identity", about_centre(np.eye(3), dims)
    for axis in range(3):
        yield "rotation 10 deg about axis %d" % axis, about_centre(rotation(axis, 10.0), dims)
    yield "zoom 2x", about_centre(0.5 * np.eye(3), dims)


def lut_stats(path):
    """{label type name: mean milliseconds of map_kernel<T, T>} from a rocprofv3 kernel_stats.csv."""
    out = {}
    if not path:
        return out
    for row in csv.DictReader(open(path)):
        name = row["Name"]
        for ctype, dtype in (("unsigned short", "uint16"), ("unsigned int", "uint32")):
            if "map_kernel<%s, %s>" % (ctype, ctype) in name:
                out[dtype] = dict(ms=float(row["AverageNs"]) * 1e-6, calls=int(row["Calls"]))
    return out


def volumes(cfg, dtype):
    import torch
    c = synth.CONFIGS[cfg]
    ctx = dev.torch_context(0)
    labels, _ = dev.synth_slab(ctx, c["dims"], dtype, c["n_cells"], c["seed"])
    torch.cuda.synchronize()
    ctx.set_volume_device(labels.data_ptr(), np.dtype(dtype).itemsize, labels.shape, keep=labels)
    return ctx, labels, c


def lut_only(reps):
    """The LUT sweep alone, `reps` calls a configuration: for a kernel trace around this process."""
    for name, cfg, dtype in CONFIGS:
        ctx, labels, c = volumes(cfg, dtype)
        lut = np.arange(c["n_cells"] + 2, dtype=dtype)
        like = np.empty(tuple(c["dims"]), dtype=dtype)
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.map_labels(lut, 0, like)
            wall.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(config=name, what="ta_volume_map, whole call (allocation, sweep, copy to the host)", wall_ms=round(min(wall), 2))))
        ctx.close()
        del labels


def run(name, cfg, dtype, order, reps, lut):
    import torch
    dtype = np.dtype(dtype)
    ctx, labels, c = volumes(cfg, dtype)
    dims = tuple(c["dims"])
    src, _ = dev.synth_slab(ctx, dims, dtype, c["n_cells"], c["seed"] + 100)
    torch.cuda.synchronize()
    nbytes_vol = int(np.prod(dims)) * dtype.itemsize
    probe_ms = ctx.read_probe(labels.data_ptr(), nbytes_vol, repeats=5)
    ctx.set_resample_source_device(src.data_ptr(), dtype.itemsize, dims, keep=src)
    y = lut.get(dtype.name)
    lines = []
    for what, A in maps(dims):
        for _ in range(3):
            ctx.resample_extract(A, order)
            ctx.synchronize()
        ms = []
        for _ in range(reps):
            ctx.resample_extract(A, order)
            ms.append(ctx.resample_timing())
        k = statistics.median(ms)
        d = ctx.resample_debug()
        lines.append(dict(config=name, dtype=dtype.name, mode="linear" if order else "nearest", map=what, kernel_ms=round(k, 4),
                          kernel_ms_min=round(min(ms), 4), kernel_ms_max=round(max(ms), 4), reps=reps, outside=ctx.resample_outside(),
                          bytes=2 * nbytes_vol, gb_per_s=round(2 * nbytes_vol / (k * 1e-3) / 1e9, 1),
                          lut_sweep_ms=None if y is None else round(y["ms"], 4), lut_sweep_calls=None if y is None else y["calls"],
                          ratio_to_lut=None if y is None else round(k / y["ms"], 3), read_probe_ms=round(probe_ms, 4),
                          tiles_per_group=d["tiles_per_group"], groups=d["groups"], vector=d["vector"]))
        print(json.dumps(lines[-1]), flush=True)
    ctx.close()
    del labels, src
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lut-only", action="store_true")
    ap.add_argument("--lut-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.jsonl"))
    a = ap.parse_args()
    if a.lut_only:
        lut_only(min(a.reps, 5))
        return
    lut = lut_stats(a.lut_stats)
    lines = []
    for name, cfg, dtype in CONFIGS:
        lines += run(name, cfg, dtype, _capi.RS_NEAREST, a.reps, lut)
    lines += run("512^3", "C2", "uint16", _capi.RS_LINEAR, a.reps, lut)
    with open(a.out, "w") as f:
        for d in lines:
            f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
