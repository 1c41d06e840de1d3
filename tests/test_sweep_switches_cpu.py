"""ta_sweep_switches.h names every compile-time switch of the sweep, and only switches that exist."""
import glob, os, re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tissue_analysis_amd", "csrc")
SETTLED = ("TA_MASKED_STORES", "TA_PROBE_NORTN", "TA_PROLOGUE_OVERLAP", "TA_FLUSH_BOX_READ", "TA_FLUSH_TRANSPOSE", "TA_HOT_ADJ",
           "TA_DRAIN_ALL", "TA_DRAIN_ALL_U16", "TA_FDRAIN1", "TA_STAMPS")


def _read(*parts):
    return open(os.path.join(*parts)).read()


def _code(text):
    """The text without its comments (string literals hold no TA_ name in these files)."""
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


HEADER = _read(CSRC, "ta_sweep_switches.h")
DEFAULTED = set(re.findall(r"^#define (TA_\w+)", HEADER, re.M))
NAMED = set(re.findall(r"\bTA_\w+", HEADER.split("// ---- ablations", 1)[1])) | DEFAULTED     # + the ablation / instrumentation block
USERS = {f: _read(CSRC, f) for f in ("kernels_scan.hip", "ta_sweep_common.h")}


def test_every_default_is_used():
    used = set(re.findall(r"\bTA_\w+", "".join(_code(t) for t in USERS.values())))
    assert len(DEFAULTED) >= 12 and not DEFAULTED - used, sorted(DEFAULTED - used)


def test_every_switch_the_sources_read_is_named():
    for name, text in USERS.items():
        code = _code(text)
        own = set(re.findall(r"^\s*#\s*define (TA_\w+)\(", code, re.M))          # function-like macros of the file itself
        read = set(re.findall(r"\bTA_\w+", code)) - own
        assert read and not read - NAMED, (name, sorted(read - NAMED))


def test_every_define_of_the_ladder_builds_is_named():
    defines = set(re.findall(r"-D(TA_\w+)", _read(ROOT, "scripts", "build_ladder_variants.sh")))
    assert len(defines) >= 8 and not defines - NAMED, sorted(defines - NAMED)


def test_settled_switches_are_gone():
    files = glob.glob(os.path.join(CSRC, "*")) + glob.glob(os.path.join(ROOT, "scripts", "*"))
    assert len(files) > 40
    for path in (f for f in files if os.path.isfile(f)):
        found = set(re.findall(r"TA_[A-Z0-9_]+", open(path, errors="replace").read())) & set(SETTLED)      # (-DTA_... too: no \b)
        assert not found, (path, sorted(found))
