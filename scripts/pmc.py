#!/usr/bin/env python3
"""Hardware counters of the sweep kernel under variant libraries: one `rocprofv3 --pmc` run per (variant, counter set), counters
only, each summarised by scripts/pmc_summary.py; the summaries end up in OUT/pmc_TAG.txt, OUT being
the directory the caller names, as scripts/ab.py is given its file.

    python scripts/pmc.py OUT TAG [--set NAME ... | --counters "A B C" ...] [--kernel REGEX] [probe_impls.py arguments] -- NAME ...

NAME `base` is the product library, any other scratch/libNAME.so (scripts/build_variant.py).  The program is
scripts/probe_impls.py on C4 (mask 0x1f, 4 iterations, no parity check) with the extra arguments, `--shape 1` say.
--dry-run prints the steps and runs nothing."""
import argparse
import os
import shutil
import sys

import steps
from steps import Step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PY = "python3"
SETS = {
    # instruction mix, waits and LDS traffic of the sweep, with the queue levels
    "sq_cycles": "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS",
    "sq_insts": "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SMEM SQ_INSTS_BRANCH SQ_WAIT_INST_LDS SQ_ACTIVE_INST_VMEM",
    "sq_lds": "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT SQ_INSTS_LDS_ATOMIC SQ_INST_LEVEL_VMEM SQ_INST_LEVEL_LDS SQ_INST_CYCLES_VMEM_RD SQ_IFETCH",
    "sq_levels": "SQ_INST_LEVEL_SMEM SQ_LDS_CMD_FIFO_FULL SQ_LDS_DATA_FIFO_FULL SQ_VMEM_TA_ADDR_FIFO_FULL SQ_VMEM_TA_CMD_FIFO_FULL SQ_IFETCH_LEVEL SQ_LEVEL_WAVES SQ_CYCLES",
    # the three passes that compare a build with its ablations, record by record
    "abl_cycles": "SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS",
    "abl_insts": "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_SMEM SQ_INSTS_BRANCH SQ_WAIT_INST_LDS SQ_INSTS_LDS_ATOMIC",
    "abl_lds": "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_ADDR_CONFLICT SQ_BUSY_CYCLES",
    "fetch": "FETCH_SIZE",
    "write": "WRITE_SIZE",
    # scripts/profiles.py: the benchmark, and the wall-voxel kernels
    "bench_sq": "SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS",
    "bench_sq2": "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS_ATOMIC SQ_INSTS_BRANCH SQ_INSTS_VMEM_RD SQ_BUSY_CYCLES",
    "wall_sq": "SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM",
    "wall_sq2": "SQ_INSTS_BRANCH SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_INST_CYCLES_SALU SQ_WAIT_INST_LDS",
}
SWEEP_KERNELS = "scan_two_rows_kernel|scan_kernel|scan_wide_kernel"


def variant_env(name):
    """The environment that selects a variant library; the tree is importable from any working directory."""
    env = {"PYTHONPATH": ROOT}
    if name != "base":
        env["TISSUE_SCAN_LIB"] = os.path.join(ROOT, "scratch", "lib%s.so" % name)
    return env


def counter_run(directory, counters, program, env, limit=300):
    """One rocprofv3 run that collects `counters` (a set's name, or the counters themselves) and nothing else, into `directory`;
    it works in /tmp, as rocprofv3's scratch files do."""
    return Step(os.path.basename(directory), limit,
                ["rocprofv3", "--pmc"] + SETS.get(counters, counters).split() + ["--output-format", "csv", "-d", directory, "--"] + program,
                {**env, "TMPDIR": "/tmp"}, "/tmp", directory + ".log")


def summary(out, name, kernel, directories):
    """pmc_summary.py over the directories of finished runs; its output is the step's log, out/NAME.txt."""
    return Step(name, 60, [PY, os.path.join(ROOT, "scripts", "pmc_summary.py"), "--kernel", kernel] + directories, {}, None,
                os.path.join(out, name + ".txt"))


def main():
    argv = sys.argv[1:]
    cut = argv.index("--") if "--" in argv else len(argv)
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", help="the directory of the results")
    ap.add_argument("tag")
    ap.add_argument("--set", nargs="+", default=[], choices=sorted(SETS))
    ap.add_argument("--counters", nargs="+", default=[])
    ap.add_argument("--kernel", default=SWEEP_KERNELS)
    ap.add_argument("--dry-run", action="store_true")
    a, probe_args = ap.parse_known_args(argv[:cut])
    out = os.path.abspath(a.out)
    todo, parts = [], []
    for v in argv[cut + 1:] or ["base"]:
        for counters in (a.set + a.counters) or ["abl_cycles", "abl_insts", "abl_lds"]:
            i = len(parts) + 1
            d = os.path.join(out, "pmc_%s_%d_%s" % (a.tag, i, v))
            todo.append(counter_run(d, counters, [PY, os.path.join(ROOT, "scripts", "probe_impls.py"), "C4", "--impl", "0", "--feat", "0x1f",
                                                  "--iters", "4", "--no-check"] + probe_args, variant_env(v)))
            todo.append(summary(out, "pmc_%s_%d_%s_summary" % (a.tag, i, v), a.kernel, [d]))
            parts.append(("## %s %s" % (v, counters), d, todo[-1].log))
    if a.dry_run:
        return steps.main(todo, out, True)
    for _, _, text in parts:                         # no summary of an earlier call is taken for this one's
        if os.path.exists(text):
            os.remove(text)
    status = steps.run(todo, out)
    with open(os.path.join(out, "pmc_%s.txt" % a.tag), "w") as f:         # what finished, also after a failure
        for head, d, text in parts:
            if os.path.exists(text):
                f.write(head + "\n" + "".join(line for line in open(text) if not line.startswith("==")))
                shutil.rmtree(d, ignore_errors=True)
    print(open(f.name).read(), end="")
    return status


if __name__ == "__main__":
    sys.exit(main())
