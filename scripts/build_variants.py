#!/usr/bin/env python3
"""Build several variant libraries (scripts/build_variant.py), three at a time, on the CPU:

    python scripts/build_variants.py "NAME -DFLAG ..." ["NAME2 -D..." ...]     ->  scratch/libNAME.so, scratch/build_NAME.log

A spec that names an ablation or debug switch (ABL, DBG) is built with --no-pin-check: its results are wrong by construction.
A failed build is reported with the end of its log and makes the exit status 1.  scripts/build_ladder_variants.sh is the list
of the sweep's ablation and instrumentation builds."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRATCH = os.path.join(ROOT, "scratch")


def command(spec):
    extra = ["--no-pin-check"] if "ABL" in spec or "DBG" in spec else []
    return [sys.executable, os.path.join(ROOT, "scripts", "build_variant.py")] + spec.split() + extra


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("specs", nargs="+", metavar='"NAME -DFLAG ..."')
    specs = ap.parse_args().specs
    os.makedirs(SCRATCH, exist_ok=True)
    failed = []
    for i in range(0, len(specs), 3):
        logs = [os.path.join(SCRATCH, "build_%s.log" % spec.split()[0]) for spec in specs[i:i + 3]]
        running = [subprocess.Popen(command(spec), cwd=ROOT, stdout=open(log, "w"), stderr=subprocess.STDOUT)
                   for spec, log in zip(specs[i:i + 3], logs)]
        for spec, log, p in zip(specs[i:i + 3], logs, running):
            if p.wait():
                failed.append(spec)
                print("FAILED %s\n%s" % (spec.split()[0], "".join(open(log).readlines()[-5:])), end="", flush=True)
    print("\n".join(sorted(f for f in os.listdir(SCRATCH) if f.startswith("lib") and f.endswith(".so"))))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
