#!/usr/bin/env python3
"""Signal histogram and median throughput (include/tissue_scan_sighist.h): one JSON line per configuration, signal type and
signal content, also written to profiles/sighist_bench.jsonl.

    python scripts/bench_sighist.py [--reps 10] [--configs C4,512^3] [--out profiles/sighist_bench.jsonl] [--variant NAME]

  hist_ms          median of the HIP-event time of the histogram pass (ta_sighist_timing) at 256 bins, with its range
  rank_ms          median of the HIP-event time of all kernels of ta_sigrank_extract for the median (the two ranks floor and
                   ceil of (n - 1) / 2 of every row): one digit pass and one select for uint8, two of each for uint16
  read_probe_ms    the sum of ta_read_probe over the buffers a pass must read, in this run: the labels and the signal
  bytes            what one pass must move: labels + signal
  hist_over_probe  hist_ms / read_probe_ms; rank_over_probe = rank_ms / read_probe_ms (a uint16 select reads everything twice)
  signal_pass_ms   median of the labels-only signal pass (ta_signal_timing, TA_SIG_LABELS) on the same buffers in this run;
                   hist_over_signal = hist_ms / signal_pass_ms, rank_over_signal likewise
  spills           counts that found no slot in a workgroup's LDS table (ta_sighist_debug) in the histogram pass; rank_spills in
                   the last digit pass of the select
  signal           'random': uniform over the type; 'constant': one value everywhere -- the two ends of the contention range
  variant          the library the numbers come from when it is not the product build (TISSUE_SCAN_LIB, scripts/build_variant.py)"""
import statistics

import numpy as np

import featbench as fb
from tissue_analysis_amd import _capi


def run(cfg, a):
    import torch
    with fb.resident(cfg) as (ctx, v, _):
        nvox = v.numel()
        ctx.extract(_capi.F_VOLUME, ctx.max_label())
        count = ctx.labels()[0]
        present = count > 0
        top = np.where(present, count - np.uint64(1), np.uint64(0))
        ranks = np.stack([top // np.uint64(2), (top + np.uint64(1)) // np.uint64(2)], axis=1)
        ranks[~present] = np.uint64(0xFFFFFFFFFFFFFFFF)
        probe_labels = fb.read_probe(ctx, v)[0]
        for sbytes in (1, 2):
            for content in ("random", "constant"):
                if sbytes == 1:
                    sig = (torch.randint(0, 256, tuple(v.shape), dtype=torch.uint8, device=v.device) if content == "random"
                           else torch.full(tuple(v.shape), 200, dtype=torch.uint8, device=v.device))
                else:
                    sig = (torch.randint(-32768, 32767, tuple(v.shape), dtype=torch.int16, device=v.device) if content == "random"
                           else torch.full(tuple(v.shape), 20000, dtype=torch.int16, device=v.device))
                torch.cuda.synchronize()
                probe_ms = probe_labels + fb.read_probe(ctx, sig)[0]
                ctx.set_signal_device(sig.data_ptr(), sbytes, keep=sig)
                labels_only = lambda: ctx.signal_extract(_capi.SIG_LABELS)
                labels_only()
                ctx.signal_timing()
                signal_ms = statistics.median(fb.timed(labels_only, ctx.signal_timing, a.reps, warmup=0))
                width = 8 * sbytes - 8
                ctx.sighist_extract(width)
                ctx.sighist_timing()
                hist = fb.timed(lambda: ctx.sighist_extract(width), lambda: ctx.sighist_timing()[0], a.reps, warmup=0)
                counts = ctx.sighist_get()
                hdebug = ctx.sighist_debug()
                assert np.array_equal(counts.sum(axis=1), count)
                ctx.sigrank_extract(ranks)
                ctx.sighist_timing()
                rank = fb.timed(lambda: ctx.sigrank_extract(ranks), lambda: ctx.sighist_timing()[1], a.reps, warmup=0)
                values = ctx.sigrank_get()
                rdebug = ctx.sighist_debug()
                assert (values[present] != _capi.SIGRANK_NONE).all()
                h, r = statistics.median(hist), statistics.median(rank)
                nbytes = nvox * (cfg.dtype.itemsize + sbytes)
                yield dict(config=cfg.name, dims=list(cfg.dims), labels_dtype=cfg.dtype.name, signal_dtype="uint%d" % (8 * sbytes),
                           signal=content, variant=a.variant, slots=_capi.SIGHIST_SLOTS if a.variant is None else None,
                           **fb.spread("hist_ms", hist), **fb.spread("rank_ms", rank), reps=a.reps, bytes=nbytes,
                           bytes_per_voxel=nbytes // nvox, hist_tbs=round(nbytes / (h * 1e-3) / 1e12, 3),
                           read_probe_ms=round(probe_ms, 4), read_probe_tbs=round(nbytes / (probe_ms * 1e-3) / 1e12, 3),
                           hist_over_probe=round(h / probe_ms, 3), rank_over_probe=round(r / probe_ms, 3),
                           signal_pass_ms=round(signal_ms, 4), hist_over_signal=round(h / signal_ms, 3),
                           rank_over_signal=round(r / signal_ms, 3), voxels=nvox, rows_in_use=int(present.sum()),
                           counters_in_use=int((counts > 0).sum()), spills=hdebug["spills"], rank_spills=rdebug["spills"],
                           tiles_per_group=hdebug["tiles_per_group"], groups=hdebug["groups"])
                del sig
                torch.cuda.empty_cache()


def main():
    fb.main(run, reps=10, configs="C4,512^3", out="profiles/sighist_bench.jsonl", mode="w",
            extra_args=[("--variant", dict(default=None, help="a name for the library under TISSUE_SCAN_LIB, recorded with every line"))])


if __name__ == "__main__":
    main()
