#!/usr/bin/env python3
"""Same-call comparison of variant libraries: differences below 3 % are decided only here, never across calls.

    python scripts/ab.py OUT.txt NAME ... [--shape 0|1|both] [--probe sweep|walls] [--dry-run]

NAME `base` is the product library, any other scratch/libNAME.so (scripts/build_variant.py); the names run in the order given,
so `base x base x` alternates.  --probe sweep (the default) times C4 (7 iterations) and the tissue-filled C4 (5 iterations) with
scripts/probe_impls.py, mask 0x1f, no parity check (ablations are wrong by construction; real candidates go through the test
suite); --shape forces the tile shape, `both` runs all names with shape 1 and then with shape 0.  --probe walls times the grouped
wall-voxel fetch of C2 and C3 with scripts/probe_walls.py.  OUT gets a `== NAME` header per run and the probes' result lines
under it (appended: one file can collect several calls); with --shape both, a `# shape N` line stands before each of the two
rounds.  The probes' whole output is kept beside OUT, one log a step."""
import argparse
import collections
import os
import sys

import steps
from pmc import PY, ROOT, variant_env
from steps import Step

# one program of a comparison: its arguments and time limit, and which of its output lines go to OUT: those that hold one of
# `kept`, cut to `width` columns, behind `prefix`
Probe = collections.namedtuple("Probe", "what argv limit kept width prefix")
IMPLS = [PY, os.path.join(ROOT, "scripts", "probe_impls.py"), "C4", "--impl", "0", "--feat", "0x1f", "--no-check"]
WALLS = [PY, os.path.join(ROOT, "scripts", "probe_walls.py")]
SWEEP_LINES = ("impl=0", "Error", "error")
PROBES = {"sweep": [Probe("c4", IMPLS + ["--iters", "7"], 300, SWEEP_LINES, 160, ""),
                    Probe("filled", IMPLS + ["--iters", "5", "--no-ellipsoid"], 300, SWEEP_LINES, 160, "filled ")],
          "walls": [Probe("c2", WALLS + ["C2"], 200, ("grouped",), 60, ""),
                    Probe("c3", WALLS + ["C3"], 300, ("grouped",), 61, "C3 ")]}


def result_lines(step, probe):
    """The lines of a finished step's log that go to OUT; none if the step did not run."""
    if not os.path.exists(step.log):
        return []
    return [probe.prefix + line.rstrip("\n")[:probe.width] + "\n" for line in open(step.log, errors="replace")
            if any(k in line for k in probe.kept)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("names", nargs="+")
    ap.add_argument("--shape", choices=("0", "1", "both"), default=None)
    ap.add_argument("--probe", choices=sorted(PROBES), default="sweep")
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    if a.shape and a.probe != "sweep":
        ap.error("--shape is the sweep's tile shape")
    out = os.path.abspath(a.out)
    directory, stem = os.path.dirname(out), os.path.splitext(os.path.basename(out))[0]
    todo, report = [], []               # report: (header lines, step, probe) in the order of OUT
    for shape in ["1", "0"] if a.shape == "both" else [a.shape]:
        header = ["# shape %s\n" % shape] if a.shape == "both" else []
        for v in a.names:
            header.append("== %s\n" % v)
            for probe in PROBES[a.probe]:
                name = "%s.%02d_%s_%s" % (stem, len(todo) + 1, v, probe.what)
                todo.append(Step(name, probe.limit, probe.argv + (["--shape", shape] if shape else []), variant_env(v), ROOT,
                                 os.path.join(directory, name + ".log")))
                report.append((header, todo[-1], probe))
                header = []
    if a.dry_run:
        return steps.main(todo, directory, True)
    for step in todo:                   # no log of an earlier call is taken for this one's
        if os.path.exists(step.log):
            os.remove(step.log)
    status = steps.run(todo, directory)
    with open(out, "a") as f:           # what finished, also after a failure
        for header, step, probe in report:
            f.writelines(header + result_lines(step, probe))
    print(open(out).read(), end="")
    return status


if __name__ == "__main__":
    sys.exit(main())
