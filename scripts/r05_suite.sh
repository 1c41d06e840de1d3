#!/bin/bash
# usage (GPU box): RESULTS=DIR scripts/r05_suite.sh TAG  -- the whole GPU suite, then the default bench line with --full
TAG=$1
RESULTS=${RESULTS:?set RESULTS to the directory the results go to}; mkdir -p "$RESULTS"
R=$GRAFT_REPO_ROOT
cd $R; export PYTHONPATH=$R
timeout -k 10 1000 python3 -m pytest tests -x -q -m gpu > $RESULTS/${TAG}_suite.log 2>&1; echo "suite rc=$?" >> $RESULTS/${TAG}_suite.log
tail -5 $RESULTS/${TAG}_suite.log
python3 bench.py --full 2> $RESULTS/${TAG}_bench.err | tail -1 > $RESULTS/${TAG}_bench.json
python3 - <<PY
import json
d=json.load(open("$RESULTS/${TAG}_bench.json"))
r=d["roofline"]; s=d.get("secondary",{})
print("C4 kernel_ms", r["kernel_ms"], "frac", r["frac"], "kernel", r["kernel"], "ms_per_step", d["ms_per_step"], "frac50k", r.get("frac_50k_labels"))
for k in ("tissue_filled","c5_single_gpu","wall_voxels_c2","sparse_ids","two_steps_in_flight"):
    print(k, {a:b for a,b in s.get(k,{}).items() if a in ("kernel_ms","roofline_frac","ms_per_step","kernels_ms","census_ms","rank_copy_ms","skipped")})
PY
