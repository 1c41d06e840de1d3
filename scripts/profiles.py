#!/usr/bin/env python3
"""Kernel statistics and hardware counters of one workload, each in a run of its own:

    python scripts/profiles.py OUT TAG [sweep] [--dry-run]
    python scripts/profiles.py OUT TAG walls [CONFIG] [--dry-run]

OUT is the directory of the results.  sweep (the default): the default benchmark -> OUT/prof_TAG_{stats,fetch,write,bench_sq,
bench_sq2}, prof_TAG_kernel_stats.csv and prof_TAG_pmc.txt.  walls: the wall-voxel kernels of CONFIG (default C2) through
scripts/probe_walls.py -> OUT/wall_TAG_* likewise, with the probe's own output first.  The `--kernel-trace --stats` run is one
step, every counter set another (scripts/pmc.py's counter_run), the summary and the copy of the statistics are steps as well.
The kernels' times are in the copied CSV, sorted by total time; no table of them is printed."""
import argparse
import os
import sys

import steps
from pmc import PY, ROOT, counter_run, summary
from steps import Step

COPY = "import glob, shutil, sys; shutil.copy(glob.glob(sys.argv[1] + '/**/*kernel_stats.csv', recursive=True)[0], sys.argv[2])"
ENV = {"PYTHONPATH": ROOT}
BENCH = [PY, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--no-secondary"]
WORKLOADS = {       # kind -> (prefix, program of the trace, program of the counter runs, counter sets, kernels of the summary)
    "sweep": ("prof", BENCH + ["--steps", "20", "--warmup", "3"], BENCH + ["--steps", "5", "--warmup", "1"],
              ("fetch", "write", "bench_sq", "bench_sq2"),
              "scan_kernel|scan_wide_kernel|scan_two_rows_kernel|scan_noadj_kernel|init_kernel|pairs_collect|read_probe"),
    "walls": ("wall", None, None, ("wall_sq", "wall_sq2", "fetch", "write"), "wall_cells|wall_copy"),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", help="the directory of the results")
    ap.add_argument("tag")
    ap.add_argument("kind", nargs="?", default="sweep", choices=sorted(WORKLOADS))
    ap.add_argument("config", nargs="?", default=None, help="walls only (default C2)")
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    if a.config and a.kind != "walls":
        ap.error("CONFIG goes with walls; sweep profiles the default benchmark")
    out = os.path.abspath(a.out)
    prefix, traced, counted, sets, kernels = WORKLOADS[a.kind]
    base = os.path.join(out, "%s_%s_" % (prefix, a.tag))
    todo, env = [], ENV
    if a.kind == "walls":
        env = {**ENV, "TA_WALL_VERBOSE": "1"}
        traced = counted = [PY, os.path.join(ROOT, "scripts", "probe_walls.py"), a.config or "C2"]
        todo.append(Step(os.path.basename(base) + "probe", 200, traced, env, ROOT))
    todo.append(Step(os.path.basename(base) + "stats", 300,
                     ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", base + "stats", "--"] + traced,
                     {**env, "TMPDIR": "/tmp"}, "/tmp"))
    todo.append(Step(os.path.basename(base) + "copy_stats", 60, [PY, "-c", COPY, base + "stats", base + "kernel_stats.csv"]))
    todo += [counter_run(base + s, s, counted, env) for s in sets]
    todo.append(summary(out, os.path.basename(base) + "pmc", kernels, [base + s for s in sets]))
    return steps.main(todo, out, a.dry_run)


if __name__ == "__main__":
    sys.exit(main())
