"""The sweep's diagnostic counters: record counts from a TA_RECCOUNT build, a workgroup's life from a TA_BARSTAMP build (GPU box):

    TISSUE_SCAN_LIB=$PWD/scratch/libreccount.so python scripts/probe_stamps.py [C4] [--no-ellipsoid]
"""
import sys

import featbench as fb
from tissue_analysis_amd import _capi

name = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else "C4"
cfg = fb.config(name)._replace(ellipsoid="--no-ellipsoid" not in sys.argv)
with fb.resident(cfg) as (ctx, vol, L):
    for a in sys.argv:                                   # --shape=0|1: TA_OPT_SWEEP_SHAPE
        if a.startswith("--shape="):
            ctx.set_option(_capi.OPT_SWEEP_SHAPE, int(a.split("=")[1]))
    for feats in (0x1f,):
        for _ in range(3):
            ctx.extract(feats, L)
            ctx.synchronize()
        t = ctx.timing()
        d = ctx.debug_counters()
        s = d.get("stamps")
        print("%s feat=0x%02x sweep %.3f ms  counters %s" % (name, feats, t["ms_sweep"], d))
        if s:                                      # (a TA_RECCOUNT build; a TA_BARSTAMP build's cycles are in the counters line)
            print("  records per launch: faces (axes 0, 1) %d, runs (with the axis-2 faces) %d, drains %d" % (s[0], s[1], s[2]))
