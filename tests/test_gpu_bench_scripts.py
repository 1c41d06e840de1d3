"""Every scripts/bench_*.py still produces its JSON lines: run() of each, in this process, on a volume of 40 x 10 x 520 (partial
plane, row and column blocks, rows of whole strips), two repetitions.  The keys of a line are pinned, in order, to what the
script wrote before it shared scripts/featbench.py: the last pass line of the feature's profiles/*_bench.jsonl where one is
committed, the script's own dict otherwise.  Times are not looked at."""
import argparse
import importlib
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import featbench as fb  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = {
    "bench_cell_extents": "config dims labels signal reps rows rows_with_voxels kernel_ms kernel_ms_min kernel_ms_p25 kernel_ms_p75 sigmom_ms "
                          "sigmom_ms_min sigmom_ms_p25 sigmom_ms_p75 ratio bytes sigmom_bytes read_probe_tbs frac_read_probe spills "
                          "tiles_per_group groups sigmom_spills",
    "bench_components": "config dims labels_dtype pass_ms pass_ms_min pass_ms_max after_ms reps components labels fragmented voxels largest "
                        "junction_walks_ms read_probe_ms read_probe_tbs pass_over_probe pass_over_junction_walks",
    "bench_cosignal": "config dims labels channels reps kernel_ms kernel_ms_min signal_a_ms signal_b_ms signal_ms signal_ms_min ratio bytes "
                      "signal_bytes read_probe_tbs frac_read_probe spills tiles_per_group groups signal_label_spills",
    "bench_distance": "config mode dims labels_dtype pass_ms pass_ms_min pass_ms_max after_ms after_ms_min after_ms_max reps labels "
                      "largest_radius read_probe_ms read_probe_tbs pass_over_probe bytes_rows bytes_columns bytes_table batches batch_columns",
    "bench_junctions": "config dims labels pass_ms pass_ms_min pass_ms_max after_ms reps blocks records3 records4 edges vertices degenerate "
                       "bytes tb_per_s frac_8tbs read_probe_ms read_probe_tbs pass_over_probe",
    "bench_mesh": "config what dims labels sub_factor cells_requested cells vertices triangles device_ms device_ms_min reps out_bytes "
                  "model_bytes frac_8tbs model_by_kernel",
    "bench_nearest": "config dims labels_dtype reps erased_labels filled remaining labels_that_gained column_launches pass_ms pass_ms_min "
                     "pass_ms_max after_ms after_ms_min after_ms_max distance_pass_ms distance_pass_ms_min distance_pass_ms_max "
                     "distance_after_ms distance_after_ms_min distance_after_ms_max pass_over_distance",
    "bench_overlap": "config dims a b kernel_ms kernel_ms_min kernel_ms_max compact_ms pairs passes reps bytes tb_per_s frac_8tbs "
                     "read_probe_tbs frac_read_probe",
    "bench_profile": "config dims labels_dtype signal_dtype shells pass_ms pass_ms_min pass_ms_max reps bytes bytes_per_voxel pass_tbs "
                     "read_probe_ms read_probe_tbs pass_over_probe signal_pass_ms pass_over_signal counted_voxels voxels keys_in_use spills "
                     "tiles_per_group groups",
    "bench_resample": "config dtype mode map kernel_ms kernel_ms_min kernel_ms_max reps outside bytes gb_per_s lut_sweep_ms lut_sweep_calls "
                      "ratio_to_lut read_probe_ms tiles_per_group groups vector",
    "bench_sighist": "config dims labels_dtype signal_dtype signal variant slots hist_ms hist_ms_min hist_ms_max rank_ms rank_ms_min "
                     "rank_ms_max reps bytes bytes_per_voxel hist_tbs read_probe_ms read_probe_tbs hist_over_probe rank_over_probe "
                     "signal_pass_ms hist_over_signal rank_over_signal voxels rows_in_use counters_in_use spills rank_spills "
                     "tiles_per_group groups",
    "bench_signal": "config what dims labels signal kernel_ms kernel_ms_min reps bytes frac_8tbs read_probe_tbs frac_read_probe",
    "bench_signal_moments": "config dims labels signal reps kernel_ms kernel_ms_min signal_ms signal_ms_min ratio bytes read_probe_tbs "
                            "frac_read_probe signal_frac_read_probe spills tiles_per_group groups signal_label_spills",
    "bench_topology": "config dims labels pass_ms pass_ms_min pass_ms_max reps mvoxel_per_s bytes tb_per_s frac_hbm mixed spills "
                      "tiles_per_group groups junction_walk_ms pass_over_walk read_probe_ms",
    "bench_wall_geometry": "config dims labels reps rounds geo_ms signal_walls_ms read_probe_ms geo_ms_median signal_walls_ms_median ratio "
                           "geo_spread signal_spread pairs faces spills bytes frac_8tbs geo_over_probe",
}
# fields that are null by design: the line without a signal, the product build, no kernel trace of the LUT sweep handed in
NULL = {"bench_profile": {"signal_dtype"}, "bench_sighist": {"variant"},
        "bench_resample": {"lut_sweep_ms", "lut_sweep_calls", "ratio_to_lut"}}
LINES = {"bench_distance": 2, "bench_profile": 2, "bench_sighist": 4, "bench_mesh": 3, "bench_resample": 5}          # of one run()

U16 = fb.Config("small", (40, 10, 520), np.dtype("uint16"), 200, 7, True)
U32 = fb.Config("small-u32", (40, 10, 515), np.dtype("uint32"), 200, 7, True)             # rows no vector load covers: scalar loads
CASES = [(script, U16) for script in sorted(KEYS)] + [("bench_signal", U32), ("bench_cell_extents", U32)]


def number(v):
    return isinstance(v, (int, float)) and math.isfinite(v)


def arguments(module, monkeypatch):
    """The script's own defaults for its extra arguments (CPU comparisons live outside run(); no LUT statistics), two repetitions."""
    given = {}
    monkeypatch.setattr(fb, "main", lambda run, **kw: given.update(kw))
    module.main()
    ap = argparse.ArgumentParser()
    for flag, kw in given.get("extra_args") or ():
        ap.add_argument(flag, **kw)
    return argparse.Namespace(reps=2, configs="small", out=None, **vars(ap.parse_args([])))


@pytest.mark.parametrize("script, cfg", CASES, ids=["%s-%s" % (s, c.dtype.name) for s, c in CASES])
def test_lines_keep_their_keys(script, cfg, monkeypatch):
    module = importlib.import_module(script)
    lines = fb.lines_of(module.run(cfg, arguments(module, monkeypatch)))
    assert len(lines) == LINES.get(script, 1)
    for line in lines:
        assert list(line) == KEYS[script].split()
        for key, v in line.items():
            if script == "bench_mesh" and key == "model_by_kernel":
                assert v and all(isinstance(n, int) for n in v.values())
            elif v is None:
                assert key in NULL.get(script, ()), key
            else:
                assert number(v) or isinstance(v, str) or (isinstance(v, list) and v and all(number(n) for n in v)), (key, v)
