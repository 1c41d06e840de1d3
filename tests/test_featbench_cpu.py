"""scripts/featbench.py: the configuration table, the summary of a list of timings, the writer -- and the defaults every
scripts/bench_*.py hands to featbench.main, which are the ones each script had before it shared the scaffold."""
import argparse
import glob
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import featbench as fb  # noqa: E402


@pytest.mark.parametrize("name, want", [
    ("C2", ((512, 512, 512), "uint16", 5000, 1, True)),
    ("C4", ((1024, 1024, 1024), "uint32", 50000, 2, True)),
    ("C4-tissue", ((1024, 1024, 1024), "uint32", 50000, 2, False)),
    ("512^3", ((512, 512, 512), "uint16", 5000, 1, True)),
])
def test_configuration_table(name, want):
    c = fb.config(name)
    assert (c.name, c.dims, c.dtype.name, c.n_cells, c.seed, c.ellipsoid) == (name,) + want
    assert isinstance(c.dtype, np.dtype) and isinstance(c.dims, tuple)


def test_unknown_configuration_is_an_error():
    with pytest.raises(KeyError):
        fb.config("C9")


def test_spread_fields_and_rounding():
    ms = [1.00004, 2.00016, 4.0, 8.123456, 3.0]
    assert fb.spread("k_ms", ms) == {"k_ms": 3.0, "k_ms_min": 1.0, "k_ms_max": 8.1235}
    assert list(fb.spread("k_ms", ms)) == ["k_ms", "k_ms_min", "k_ms_max"]
    assert fb.spread("k_ms", ms, ("min",)) == {"k_ms": 3.0, "k_ms_min": 1.0}
    q = fb.spread("k_ms", ms, ("min", "p25", "p75"))              # statistics.quantiles(n=4): 1.5001 and 6.061728
    assert list(q) == ["k_ms", "k_ms_min", "k_ms_p25", "k_ms_p75"]
    assert q == {"k_ms": 3.0, "k_ms_min": 1.0, "k_ms_p25": 1.5001, "k_ms_p75": 6.0617}
    assert fb.spread("k_ms", [1.23456789, 1.2]) == {"k_ms": 1.2173, "k_ms_min": 1.2, "k_ms_max": 1.2346}


def test_timed_and_alternating_order():
    calls = []
    ms = fb.timed(lambda: calls.append("e"), lambda: calls.append("t") or 1.5, 2, warmup=1)
    assert ms == [1.5, 1.5] and calls == ["e", "e", "t", "e", "t"]
    del calls[:]
    a, b = fb.alternating_ms([(lambda: calls.append("a"), lambda: 1.0), (lambda: calls.append("b"), lambda: 2.0)], 2, warmup=1)
    assert (a, b) == ([1.0, 1.0], [2.0, 2.0]) and calls == ["a", "b", "a", "b", "a", "b"]


@pytest.mark.parametrize("mode, kept", [("a", True), ("w", False)])
def test_writer_appends_or_truncates_and_prints_first(tmp_path, capsys, mode, kept):
    out = tmp_path / "lines.jsonl"
    out.write_text('{"old": 1}\n')
    seen = []

    def lines():
        for i in range(2):
            yield {"n": i}
            seen.append((capsys.readouterr().out, out.read_text()))          # after the line was taken: printed, file untouched

    fb.emit(lines(), str(out), mode)
    assert seen == [('{"n": 0}\n', '{"old": 1}\n'), ('{"n": 1}\n', '{"old": 1}\n')]
    assert out.read_text() == ('{"old": 1}\n' if kept else "") + '{"n": 0}\n{"n": 1}\n'


def test_main_resolves_configurations_and_takes_one_line_or_many(tmp_path, capsys):
    def run(cfg, a):
        return dict(config=cfg.name, reps=a.reps, erase=a.erase) if cfg.name == "C2" else [dict(config=cfg.name)] * 2

    out = tmp_path / "o.jsonl"
    got = fb.main(run, reps=7, configs="C2,C4-tissue", out=None, mode="w", extra_args=[("--erase", dict(type=int, default=10))],
                  after=lambda a: dict(config="after"), argv=["--out", str(out)])
    want = [dict(config="C2", reps=7, erase=10), dict(config="C4-tissue"), dict(config="C4-tissue"), dict(config="after")]
    assert got == want and [json.loads(line) for line in out.read_text().splitlines()] == want
    assert [json.loads(line) for line in capsys.readouterr().out.splitlines()] == want


# script -> (--reps, --configs, --out, mode) as each script had them before this module existed; a script without --configs ran
# the configurations listed here, one without --out wrote no file
DEFAULTS = {
    "bench_cell_extents": (30, "C4,512^3", "profiles/extents_bench.jsonl", "a"),
    "bench_components": (10, "C4,C4-tissue,512^3", "profiles/components_bench.jsonl", "w"),
    "bench_cosignal": (30, "C4,512^3", "profiles/cosignal_bench.jsonl", "a"),
    "bench_distance": (10, "C4,C4-tissue,512^3", "profiles/distance_bench.jsonl", "w"),
    "bench_junctions": (30, "C4,512^3", "profiles/junctions_bench.jsonl", "w"),
    "bench_mesh": (10, "C4,512^3", None, "w"),
    "bench_nearest": (10, "C4,512^3", "profiles/nearest_bench.jsonl", "a"),
    "bench_overlap": (30, "C4,512^3", "profiles/overlap_bench.jsonl", "w"),
    "bench_profile": (10, "C4,512^3", "profiles/profile_bench.jsonl", "w"),
    "bench_resample": (20, "512^3,C4", "profiles/resample_bench.jsonl", "w"),
    "bench_sighist": (10, "C4,512^3", "profiles/sighist_bench.jsonl", "w"),
    "bench_signal": (30, "C4,512^3", None, "w"),
    "bench_signal_moments": (30, "C4,512^3", "profiles/sigmoments_bench.jsonl", "a"),
    "bench_topology": (30, "C2,C4", "profiles/topology_bench.jsonl", "w"),
    "bench_wall_geometry": (30, "C4,512^3", "profiles/wall_geometry_bench.jsonl", "w"),
}
EXTRAS = {"bench_nearest": {"erase": 10}, "bench_wall_geometry": {"rounds": 2}, "bench_distance": {"batch": 0},
          "bench_sighist": {"variant": None}, "bench_mesh": {"no_cpu": False}, "bench_resample": {"lut_only": False, "lut_stats": None}}


def test_every_bench_script_is_in_the_table():
    assert sorted(DEFAULTS) == sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(ROOT, "scripts", "bench_*.py")))


@pytest.mark.parametrize("script", sorted(DEFAULTS))
def test_script_keeps_its_defaults(script, monkeypatch):
    module = importlib.import_module(script)
    given = {}
    monkeypatch.setattr(fb, "main", lambda run, **kw: given.update(kw, run=run))
    module.main()
    assert given["run"] is module.run
    assert (given["reps"], given["configs"], given["out"], given["mode"]) == DEFAULTS[script]
    ap = argparse.ArgumentParser()
    for flag, kw in given.get("extra_args") or ():
        ap.add_argument(flag, **kw)
    assert vars(ap.parse_args([])) == EXTRAS.get(script, {})
