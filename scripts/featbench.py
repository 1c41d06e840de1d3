"""What the feature benchmarks (scripts/bench_*.py) share: configurations by name, the resident volume, the timing loop and its
summary, the read probe, and the command line with its JSON writer.  A benchmark is a `run(cfg, args)` that returns or yields
its JSON lines, plus one `featbench.main(run, ...)` call; nothing here knows a feature.  torch is imported where it is used."""
import argparse
import collections
import contextlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tissue_analysis_amd import synth  # noqa: E402
from tissue_analysis_amd import device as dev  # noqa: E402

TBS = 8e12                      # the round figure the frac_8tbs fields compare against
FLOAT4_COPY_BPS = 6.29e12       # what a float4 copy reaches on the MI355X: bench_topology.py's frac_hbm

Config = collections.namedtuple("Config", "name dims dtype n_cells seed ellipsoid")
# name -> (entry of synth.CONFIGS, label type when it is not the entry's own, ellipsoid mask)
ALIASES = {"C4-tissue": ("C4", None, False),           # cells everywhere, no background around them
           "512^3": ("C2", "uint16", True)}


def config(name):
    base, dtype, ellipsoid = ALIASES.get(name, (name, None, True))
    c = synth.CONFIGS[base]
    return Config(name, tuple(c["dims"]), np.dtype(dtype or c["dtype"]), c["n_cells"], c["seed"], ellipsoid)


def signal_dtype(cfg):
    """The signal type the benchmarks pair with a label type: uint16 beside uint32 labels, uint8 beside uint16 labels."""
    return np.dtype(np.uint16 if cfg.dtype.itemsize == 4 else np.uint8)


def random_signal(dims, itemsize, generator):
    """Uniform over the whole uint8 / uint16 range, on the device (int16 storage holds the uint16 bit patterns)."""
    import torch
    return torch.randint(0, 1 << (8 * itemsize), tuple(dims), generator=generator, device="cuda", dtype=torch.int32).to(
        torch.uint8 if itemsize == 1 else torch.int16)


@contextlib.contextmanager
def resident(cfg):
    """A context on torch's stream with cfg's synthetic volume resident in it: yields (context, tensor, max label).  Leaving
    closes the context, also when the body raises, and empties torch's cache of what nothing refers to any more; the volume
    itself goes back to the cache when the caller's own names for it go, at the end of its run()."""
    import torch
    ctx = dev.torch_context(0)
    try:
        vol, top = dev.synth_slab(ctx, cfg.dims, cfg.dtype, cfg.n_cells, cfg.seed, ellipsoid=cfg.ellipsoid)
        torch.cuda.synchronize()
        ctx.set_volume_device(vol.data_ptr(), cfg.dtype.itemsize, vol.shape, keep=vol)
        yield ctx, vol, top
    finally:
        ctx.close()
        vol = None
        torch.cuda.empty_cache()


def read_probe(ctx, tensor):
    """ta_read_probe over a tensor's bytes: (milliseconds, bytes per second)."""
    nbytes = tensor.numel() * tensor.element_size()
    ms = ctx.read_probe(tensor.data_ptr(), nbytes, repeats=5)
    return ms, nbytes / (ms * 1e-3)


def timed(enqueue, timing, reps, warmup=3):
    """`warmup` untimed calls of enqueue(), then `reps` of enqueue() followed by timing(): the list of what timing() gave."""
    return alternating_ms([(enqueue, timing)], reps, warmup)[0]


def alternating_ms(passes, reps, warmup=3):
    """passes: [(enqueue, timing)]; `warmup` rounds, then `reps` rounds that run each pass once, in turn.  One list per pass."""
    for _ in range(warmup):
        for enqueue, _ in passes:
            enqueue()
    ms = [[] for _ in passes]
    for _ in range(reps):
        for i, (enqueue, timing) in enumerate(passes):
            enqueue()
            ms[i].append(timing())
    return ms


def spread(name, ms, fields=("min", "max")):
    """{name: median, name_min: ..., ...} rounded to four places; fields from min, max, p25, p75, in the order given."""
    q = statistics.quantiles(ms, n=4) if len(ms) > 1 else [ms[0]] * 3
    value = {"min": min(ms), "max": max(ms), "p25": q[0], "p75": q[2]}
    out = {name: round(statistics.median(ms), 4)}
    out.update((name + "_" + f, round(value[f], 4)) for f in fields)
    return out


def lines_of(result):
    """What a run() gave, as a list of lines: it may return one dict, a list of them, or yield them."""
    return [result] if isinstance(result, dict) else list(result)


def emit(lines, out, mode):
    """Print each line as soon as it exists (`lines` may be a generator), then write them to `out` ('a' appends, 'w' truncates);
    a run without lines (bench_resample.py --lut-only) leaves the file alone."""
    done = []
    for d in lines:
        print(json.dumps(d), flush=True)
        done.append(d)
    if out and done:
        with open(out, mode) as f:
            f.writelines(json.dumps(d) + "\n" for d in done)
    return done


def main(run, *, reps, configs, out, mode, extra_args=None, after=None, argv=None):
    """The command line of a feature benchmark.  reps, configs (comma-separated names), out (a path under the tree, or None for
    no file) are the script's defaults; mode says whether a rerun appends to `out` or truncates it; extra_args is a list of
    (flag, add_argument keywords); after(args) gives lines that follow all configurations (a CPU comparison, say)."""
    ap = argparse.ArgumentParser(description=sys.modules[run.__module__].__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--configs", default=configs, help="comma-separated: C1..C5, C4-tissue, 512^3")
    ap.add_argument("--out", default=os.path.join(ROOT, out) if out else None)
    for flag, kw in extra_args or ():
        ap.add_argument(flag, **kw)
    a = ap.parse_args(argv)

    def everything():
        for name in a.configs.split(","):
            yield from lines_of(run(config(name), a))
        if after:
            yield from lines_of(after(a))
    return emit(everything(), a.out, mode)
