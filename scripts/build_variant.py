"""Build a VARIANT of libtissue_scan.so with extra -D flags (experiments, ablations, instrumentation) into scratch/:

    python scripts/build_variant.py NAME -DTA_RECCOUNT [-DTA_FCAP=128 ...]     ->  scratch/libNAME.so

Run anything against it with TISSUE_SCAN_LIB=$PWD/scratch/libNAME.so (the product never loads a variant by itself).
`--no-pin-check` skips the check that compiler-allocated registers stay clear of the hand-pinned ones (ablations whose
results are wrong by construction do not need it; anything timed AND compared must keep it).  A second build of the same
NAME with the same flags compiles nothing."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tissue_analysis_amd import build as B      # noqa: E402

name = sys.argv[1]
defs = [a for a in sys.argv[2:] if a.startswith("-D") or a.startswith("-m") or a.startswith("-f")]
out_dir = os.path.join(ROOT, "scratch", "variants", name)
lib = os.path.join(ROOT, "scratch", "lib%s.so" % name)


def keep_resource_usage(src, text):
    if src == "kernels_scan.hip":
        open(os.path.join(out_dir, "resource_usage.txt"), "w").write(text)


B.compile_and_link(B.CSRC, B.SOURCES, out_dir, lib, B.FLAGS, defines=defs,
                   extra_flags={} if "--no-extra-flags" in sys.argv else B.EXTRA_FLAGS,        # (e.g. machine LICM back on)
                   tail={"kernels_scan.hip": B.SAVE_TEMPS}, pin_check="--no-pin-check" not in sys.argv,
                   report=keep_resource_usage)
print(lib)
