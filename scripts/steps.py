"""The one way a script runs a sequence of GPU programs: each step a fresh child process under a time limit of its own, and
nothing is started after the first step that fails -- a card that faulted gets no further work.  Standard library only; the
parent never opens the GPU.  There is no retry, no way to continue after an error, and no two steps at a time."""
import collections
import os
import shlex
import subprocess
import time

Step = collections.namedtuple("Step", "name limit argv env cwd log", defaults=({}, None, None))    # limit in seconds; env: additions


def plan(steps):
    """One line per step: limit, environment additions, working directory, argv."""
    return ["%ds  env %s  cwd %s  %s" % (s.limit, " ".join("%s=%s" % kv for kv in sorted(s.env.items())) or "-", s.cwd or ".",
                                         shlex.join(s.argv)) for s in steps]


def run(steps, out_dir):
    """Run the steps in order; a step's output goes to its log (default out_dir/NAME.log) and one line (name, exit status,
    seconds) to out_dir/steps.log.  Returns 0, or the first non-zero status (124 / 137: the time limit, 134: abort, 139:
    segmentation fault, ...) after printing the step's name and the tail of its log; the steps behind it are not started."""
    os.makedirs(out_dir, exist_ok=True)
    for s in steps:
        log = s.log or os.path.join(out_dir, s.name + ".log")
        t0 = time.time()
        with open(log, "w") as f:
            status = subprocess.call(["timeout", "-k", "10", str(s.limit)] + list(s.argv), env={**os.environ, **s.env}, cwd=s.cwd,
                                     stdin=subprocess.DEVNULL, stdout=f, stderr=subprocess.STDOUT)
        status = 128 - status if status < 0 else status               # (timeout itself killed by a signal)
        with open(os.path.join(out_dir, "steps.log"), "a") as f:
            f.write("%s %d %.1f\n" % (s.name, status, time.time() - t0))
        if status:
            print("step %s: exit status %d; nothing after it was started.  The end of %s:" % (s.name, status, log), flush=True)
            print("".join(open(log, errors="replace").readlines()[-20:]), end="", flush=True)
            return status
    return 0


def main(steps, out_dir, dry_run):
    """What a tool does with its steps: print the plan, or run them."""
    if dry_run:
        print("\n".join(plan(steps)))
        return 0
    return run(steps, out_dir)
