#!/bin/bash
# the ablation / instrumentation builds of the sweep (switches: tissue_analysis_amd/csrc/ta_sweep_switches.h), for scripts/ab.py
# and scripts/pmc.py; CPU only.  tests/test_sweep_switches_cpu.py reads the -D flags here.
set -e
cd "$(dirname "$0")/.."
mkdir -p scratch
python3 scripts/build_variants.py "abl1 -DTA_ABLATE=1" "abl3 -DTA_ABLATE=3" "nf01 -DTA_ABL_NOFACE0 -DTA_ABL_NOFACE1" \
  "noflush -DTA_ABL_NOFLUSH" "hot1 -DTA_ABL_NOFLUSH -DTA_ABL_HOT=1" "hot2 -DTA_ABL_NOFLUSH -DTA_ABL_HOT=2" \
  "hot4 -DTA_ABL_NOFLUSH -DTA_ABL_HOT=4" "noslow -DTA_ABL_NOFLUSH -DTA_ABL_HOT=4 -DTA_ABL_NOSLOW" \
  "reccount -DTA_RECCOUNT" "barstamp -DTA_BARSTAMP" "nohalo1 -DTA_ABL_NOHALO=1"
hipcc --offload-arch=gfx950 -O2 scripts/pipes_bench.hip -o scratch/pipes_bench
