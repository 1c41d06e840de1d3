"""scripts/steps.py stops a sequence at its first failing step, and the tools built on it plan what their usage says."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
sys.path.insert(0, SCRIPTS)
import steps  # noqa: E402
from steps import Step  # noqa: E402

PY = sys.executable


def touch(path, then=""):
    return [PY, "-c", "open(%r, 'w').close(); %s" % (str(path), then)]


def log_lines(tmp_path):
    return [line.split()[:2] for line in open(tmp_path / "steps.log")]


def test_nothing_runs_after_a_failing_step(tmp_path, capsys):
    todo = [Step("one", 20, touch(tmp_path / "one")), Step("two", 20, touch(tmp_path / "two", "print('two says no'); raise SystemExit(3)")),
            Step("three", 20, touch(tmp_path / "three"))]
    assert steps.run(todo, str(tmp_path)) == 3
    assert (tmp_path / "one").exists() and (tmp_path / "two").exists() and not (tmp_path / "three").exists()
    assert log_lines(tmp_path) == [["one", "0"], ["two", "3"]]
    said = capsys.readouterr().out
    assert "two" in said and "status 3" in said and "two says no" in said
    assert "two says no" in open(tmp_path / "two.log").read()


def test_a_step_past_its_time_limit_ends_the_sequence(tmp_path):
    todo = [Step("slow", 1, [PY, "-c", "import time; time.sleep(30)"]), Step("next", 20, touch(tmp_path / "next"))]
    assert steps.run(todo, str(tmp_path)) == 124
    assert not (tmp_path / "next").exists()
    assert log_lines(tmp_path) == [["slow", "124"]]


def test_a_segmentation_fault_status_is_reported_and_ends_the_sequence(tmp_path, capsys):
    todo = [Step("crash", 20, [PY, "-c", "import sys; sys.exit(139)"]), Step("next", 20, touch(tmp_path / "next"))]
    assert steps.run(todo, str(tmp_path)) == 139
    assert not (tmp_path / "next").exists()
    assert log_lines(tmp_path) == [["crash", "139"]]
    assert "crash" in capsys.readouterr().out


def test_environment_and_working_directory_reach_the_child(tmp_path, monkeypatch):
    monkeypatch.setenv("STEPS_TEST_PARENT", "from the parent")
    work = tmp_path / "work"
    work.mkdir()
    show = "import os; print(os.environ['STEPS_TEST_EXTRA'], '|', os.environ['STEPS_TEST_PARENT'], '|', os.getcwd())"
    log = tmp_path / "elsewhere.log"
    assert steps.run([Step("show", 20, [PY, "-c", show], {"STEPS_TEST_EXTRA": "added"}, str(work), str(log))], str(tmp_path)) == 0
    assert open(log).read().strip() == "added | from the parent | %s" % os.path.realpath(work)
    assert "STEPS_TEST_EXTRA" not in os.environ


def plan_of(tool, *args):
    done = subprocess.run([PY, os.path.join(SCRIPTS, tool), "--dry-run"] + list(args), capture_output=True, text=True, cwd=ROOT)
    assert done.returncode == 0, done.stderr
    return done.stdout.splitlines()


def expected(text):
    return [line.replace("ROOT", ROOT) for line in text.strip().splitlines()]


IMPLS = "python3 ROOT/scripts/probe_impls.py C4 --impl 0 --feat 0x1f --no-check"


def test_ab_plan():
    base, x = "env PYTHONPATH=ROOT", "env PYTHONPATH=ROOT TISSUE_SCAN_LIB=ROOT/scratch/libx.so"
    want = []
    for shape in "10":
        for env in (base, x, base):
            want.append("300s  %s  cwd ROOT  %s --iters 7 --shape %s" % (env, IMPLS, shape))
            want.append("300s  %s  cwd ROOT  %s --iters 5 --no-ellipsoid --shape %s" % (env, IMPLS, shape))
    assert plan_of("ab.py", "OUT", "base", "x", "base", "--shape", "both") == expected("\n".join(want))
    assert not os.path.exists(os.path.join(ROOT, "OUT"))
    assert plan_of("ab.py", "OUT", "x", "--probe", "walls") == expected("""
200s  env PYTHONPATH=ROOT TISSUE_SCAN_LIB=ROOT/scratch/libx.so  cwd ROOT  python3 ROOT/scripts/probe_walls.py C2
300s  env PYTHONPATH=ROOT TISSUE_SCAN_LIB=ROOT/scratch/libx.so  cwd ROOT  python3 ROOT/scripts/probe_walls.py C3""")


COUNTERS = "300s  env PYTHONPATH=ROOT%s TMPDIR=/tmp  cwd /tmp  rocprofv3 --pmc %s --output-format csv -d /o/%s -- %s"
SUMMARY = "60s  env -  cwd .  python3 ROOT/scripts/pmc_summary.py --kernel '%s' %s"
STATS = "300s  env PYTHONPATH=ROOT%s TMPDIR=/tmp  cwd /tmp  rocprofv3 --kernel-trace --stats --output-format csv -d /o/%s -- %s"
COPY = ("60s  env -  cwd .  python3 -c 'import glob, shutil, sys; shutil.copy(glob.glob(sys.argv[1] + '\"'\"'/**/*kernel_stats.csv'\"'\"', "
        "recursive=True)[0], sys.argv[2])' /o/%s /o/%s")


def test_pmc_plan():
    probe = "python3 ROOT/scripts/probe_impls.py C4 --impl 0 --feat 0x1f --iters 4 --no-check --shape 1"
    sweep = "scan_two_rows_kernel|scan_kernel|scan_wide_kernel"
    assert plan_of("pmc.py", "/o", "t", "--set", "fetch", "--shape", "1", "--", "base", "x") == expected("\n".join([
        COUNTERS % ("", "FETCH_SIZE", "pmc_t_1_base", probe), SUMMARY % (sweep, "/o/pmc_t_1_base"),
        COUNTERS % (" TISSUE_SCAN_LIB=ROOT/scratch/libx.so", "FETCH_SIZE", "pmc_t_2_x", probe), SUMMARY % (sweep, "/o/pmc_t_2_x")]))


def test_profiles_plans():
    walls, verbose = "python3 ROOT/scripts/probe_walls.py C3", " TA_WALL_VERBOSE=1"
    sets = (("wall_sq", "SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM"),
            ("wall_sq2", "SQ_INSTS_BRANCH SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_INST_CYCLES_SALU SQ_WAIT_INST_LDS"),
            ("fetch", "FETCH_SIZE"), ("write", "WRITE_SIZE"))
    assert plan_of("profiles.py", "/o", "w", "walls", "C3") == expected("\n".join(
        ["200s  env PYTHONPATH=ROOT TA_WALL_VERBOSE=1  cwd ROOT  " + walls, STATS % (verbose, "wall_w_stats", walls),
         COPY % ("wall_w_stats", "wall_w_kernel_stats.csv")] +
        [COUNTERS % (verbose, counters, "wall_w_" + name, walls) for name, counters in sets] +
        [SUMMARY % ("wall_cells|wall_copy", " ".join("/o/wall_w_" + name for name, _ in sets))]))
    bench = "python3 ROOT/bench.py --no-cpu-baseline --no-secondary --steps %d --warmup %d"
    sets = (("fetch", "FETCH_SIZE"), ("write", "WRITE_SIZE"),
            ("bench_sq", "SQ_WAVES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS"),
            ("bench_sq2", "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS_ATOMIC SQ_INSTS_BRANCH SQ_INSTS_VMEM_RD SQ_BUSY_CYCLES"))
    assert plan_of("profiles.py", "/o", "s") == expected("\n".join(
        [STATS % ("", "prof_s_stats", bench % (20, 3)), COPY % ("prof_s_stats", "prof_s_kernel_stats.csv")] +
        [COUNTERS % ("", counters, "prof_s_" + name, bench % (5, 1)) for name, counters in sets] +
        [SUMMARY % ("scan_kernel|scan_wide_kernel|scan_two_rows_kernel|scan_noadj_kernel|init_kernel|pairs_collect|read_probe",
                    " ".join("/o/prof_s_" + name for name, _ in sets))]))


def test_build_variants_takes_only_specs():
    done = subprocess.run([PY, os.path.join(SCRIPTS, "build_variants.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert done.returncode == 0 and "three at a time" in done.stdout
    assert subprocess.run([PY, os.path.join(SCRIPTS, "build_variants.py"), "--nothing"], capture_output=True, cwd=ROOT).returncode == 2
