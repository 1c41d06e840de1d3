"""Build recipe for libtissue_scan.so (hipcc, gfx950 only, in-tree).

    python -m tissue_analysis_amd.build [--force] [--save-temps]

hipcc cross-compiles without a GPU; the built .so is git-ignored but travels with the tree.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJDIR = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libtissue_scan.so")
SOURCES = ["ta_api.hip", "ta_api_walls.hip", "ta_api_sparse.hip", "ta_api_exchange.hip", "ta_api_signal.hip", "ta_api_mesh.hip", "ta_api_overlap.hip", "ta_api_junctions.hip", "ta_api_wallgeo.hip", "ta_api_components.hip", "ta_api_distance.hip", "ta_api_nearest.hip", "ta_api_profile.hip", "ta_api_sighist.hip", "ta_api_sigmoments.hip", "ta_api_topology.hip", "ta_api_extents.hip", "ta_api_resample.hip",
           "kernels_basic.hip", "kernels_scan.hip", "kernels_walls.hip", "kernels_wallsort.hip", "kernels_wallmedian.hip", "kernels_census.hip",
           "kernels_pairsort.hip", "kernels_signal.hip", "kernels_mesh.hip", "kernels_overlap.hip", "kernels_junctions.hip", "kernels_wallgeo.hip",
           "kernels_components.hip", "kernels_distance.hip", "kernels_nearest.hip", "kernels_profile.hip", "kernels_sighist.hip", "kernels_sigmoments.hip", "kernels_topology.hip", "kernels_extents.hip", "kernels_resample.hip"]
HEADERS = ["ta_ctx.h", "ta_parts.h", "ta_counted.h", "ta_device.h", "ta_range_plan.h", "ta_kernels.h", "ta_sweep_common.h", "ta_sweep_switches.h", "ta_pin_tables.inc", "ta_signal.h", "ta_mesh.h", "ta_overlap.h", "ta_junctions.h", "ta_wallgeo.h", "ta_components.h", "ta_distance.h", "ta_nearest.h", "ta_separable.h", "ta_profile.h", "ta_sighist.h", "ta_sigmoments.h", "ta_topology.h", "ta_extents.h", "ta_resample.h",
           os.path.join("..", "..", "include", "tissue_scan.h"), os.path.join("..", "..", "include", "tissue_scan_signal.h"),
           os.path.join("..", "..", "include", "tissue_scan_mesh.h"), os.path.join("..", "..", "include", "tissue_scan_overlap.h"),
           os.path.join("..", "..", "include", "tissue_scan_junctions.h"), os.path.join("..", "..", "include", "tissue_scan_wallgeo.h"),
           os.path.join("..", "..", "include", "tissue_scan_components.h"), os.path.join("..", "..", "include", "tissue_scan_distance.h"),
           os.path.join("..", "..", "include", "tissue_scan_nearest.h"),
           os.path.join("..", "..", "include", "tissue_scan_profile.h"), os.path.join("..", "..", "include", "tissue_scan_sighist.h"),
           os.path.join("..", "..", "include", "tissue_scan_sigmoments.h"), os.path.join("..", "..", "include", "tissue_scan_topology.h"),
           os.path.join("..", "..", "include", "tissue_scan_resample.h"), os.path.join("..", "..", "include", "tissue_scan_extents.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
         "-Wall", "-Wno-unused-function", "-DTA_BUILD"]
# Per-source extra flags.  (The sweep kernels live on a hand-set VGPR budget -- the plane in flight is pinned above it -- and
# machine LICM, which cannot see that, hoists constant materialisations for the drains' LDS atomics out of the plane loop:
# a build in which that breaks the budget is refused by _check_pinned; `-mllvm -disable-machine-licm` for kernels_scan.hip
# is the way out that was needed for one of round 4's variants and measured 0 - 2 % slower.  Not needed by the code as it is.)
# kernels_resample.hip: the rounding order of its coordinate arithmetic is part of the ABI (include/tissue_scan_resample.h), so
# nothing in it may be contracted into a fused multiply-add; the file says so itself with a pragma, the flag says it again.
# kernels_extents.hip: every projection is three products and two sums, each rounded on its own (include/tissue_scan_extents.h); neither
# the pragma nor __dmul_rn / __dadd_rn keeps -O3 from fusing them on gfx950, the flag does.
EXTRA_FLAGS = {"kernels_resample.hip": ["-ffp-contract=off"], "kernels_extents.hip": ["-ffp-contract=off"]}


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.sep not in cand or os.path.exists(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


ZONE_REGS = {"ROWS_HALO": 21, "ROWS": 16, "TWO_ROWS": 13, "WIDE": 25}      # registers of a landing zone, by the layout names of SCAN_VARIANTS
EDGE_LAST = ("scan_kernel", "scan_noadj_kernel", "scan_wide_kernel")       # entry points whose last template argument is EDGE


def read_variants(path=os.path.join(CSRC, "kernels_scan.hip")):
    """The rows of SCAN_VARIANTS in kernels_scan.hip: [(entry point, layout of its landing zone, first pinned register)]."""
    return [(n, z, int(b)) for n, z, b in re.findall(r"^\s*X\((scan_\w+),\s*(\w+),\s*(\d+)\)", open(path).read(), re.M)]


def _zones_of(sym, is_kernel, zones):
    """The register ranges [lo, hi) that compiler-allocated code of the function `sym` must stay clear of."""
    m = re.match(r"_ZN2ta(\d+)", sym)
    name, args = (sym[m.end():][:int(m.group(1))], sym[m.end() + int(m.group(1)):]) if m else (sym, "")
    if not (is_kernel and name.startswith("scan_")):
        return list(zones.values())      # a device function: callable from any of them
    if name not in zones:
        raise RuntimeError("kernel %s is in no row of SCAN_VARIANTS (kernels_scan.hip): its landing zone is unknown" % sym)
    if name in EDGE_LAST and args.split("EEEv")[0].endswith("Lb1"):
        return []                        # edge kernels issue no hand-pinned loads: any register is theirs
    return [zones[name]]


def pinned_violations(asm, variants):
    """kernels_scan.hip keeps the plane in flight in VGPRs it names itself, above an amdgpu_num_vgpr budget that the
    compiler treats as a request, not a limit.  Returns the lines of the assembly text `asm` (outside the inline asm
    that owns them) in which a pinned kernel names a register of its own landing zone, or a device function one of
    any zone; `variants` is what read_variants() returns."""
    unknown = [v for v in variants if v[1] not in ZONE_REGS]
    zones = {n: (b, b + ZONE_REGS[z]) for n, z, b in variants if z in ZONE_REGS}
    if len(zones) < 8 or unknown:
        raise RuntimeError("the table of pinned entry points (SCAN_VARIANTS in kernels_scan.hip) is incomplete: %d entry points "
                           "read, the sweep has eight; rows of unknown layout: %s" % (len(zones), unknown))
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    reg = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
    in_asm, func, ranges, bad = False, "", list(zones.values()), []
    for ln, line in enumerate(asm.split("\n"), 1):
        t = line.strip()
        if t.startswith(";;#ASMSTART"):
            in_asm = True
        elif t.startswith(";;#ASMEND"):
            in_asm = False
        else:
            m = re.match(r"^(_Z\w+):", line)
            if m:
                func = m.group(1)
                ranges = _zones_of(func, func in kernels, zones)
                continue
            if in_asm or not t or t[0] in ";.":
                continue
            for m in reg.finditer(t.split(";")[0]):
                lo = int(m.group(1) or m.group(2)); hi = int(m.group(1) or m.group(3))
                if any(hi >= a and lo < b for a, b in ranges):
                    bad.append("%s:%d: %s" % (func, ln, t))
                    break
    return bad


def _check_pinned(hipcc, verbose=False):
    """Refuse a build in which compiler-allocated code reaches the hand-pinned registers (pinned_violations)."""
    asm = os.path.join(OBJDIR, "kernels_scan.check.s")
    cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get("kernels_scan.hip", []) + ["--cuda-device-only", "-S", os.path.join(CSRC, "kernels_scan.hip"), "-o", asm]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=OBJDIR)
    bad = pinned_violations(open(asm).read(), read_variants())
    if bad:
        raise RuntimeError("compiler-allocated VGPRs reach the hand-pinned registers in kernels_scan.hip:\n  %s"
                           % "\n  ".join(bad[:10]))


def build(force=False, save_temps=False, verbose=False):
    """Compile every HIP source for gfx950 and link libtissue_scan.so. Returns its path."""
    hipcc = _hipcc()
    os.makedirs(OBJDIR, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    procs, objs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJDIR, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-c", s, "-o", o]
            if save_temps:
                cmd += ["-save-temps=obj", "-Rpass-analysis=kernel-resource-usage"]
            if verbose:
                print(" ".join(cmd))
            procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                                cwd=OBJDIR)))
    failed = False
    for src, p in procs:
        out = p.communicate()[0].decode(errors="replace")
        if p.returncode != 0:
            failed = True
            sys.stderr.write("hipcc failed on %s:\n%s\n" % (src, out))
        elif out.strip() and (verbose or save_temps):
            print(out)
    if failed:
        raise RuntimeError("hipcc compilation failed")
    stamp = os.path.join(OBJDIR, "kernels_scan.check.ok")       # (a failed check must not be skipped by the next call)
    if _stale(stamp, [os.path.join(OBJDIR, "kernels_scan.o")]):
        _check_pinned(hipcc, verbose)
        open(stamp, "w").write("ok\n")
    if force or procs or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return LIB


ASAN_DIR = os.path.join(OBJDIR, "asan")
ASAN_LIB = os.path.join(ASAN_DIR, "libtissue_scan_asan.so")


def sanitizer_runtime():
    """Path of the AddressSanitizer runtime hipcc's clang links with -shared-libsan (to LD_PRELOAD under python)."""
    clang = os.path.join(os.path.dirname(os.path.realpath(_hipcc())), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
    return subprocess.check_output([clang, "-print-file-name=libclang_rt.asan-x86_64.so"]).decode().strip()


def build_sanitized(force=False, verbose=False):
    """HOST side of the same SOURCES under -fsanitize=address,undefined (the device side cannot be
    instrumented on this pool and is compiled as usual): the library the CPU suite loads to walk the C ABI's
    argument checks and failure paths.  Never the product build."""
    hipcc = _hipcc()
    os.makedirs(ASAN_DIR, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    flags = [f for f in FLAGS if f != "-O3"] + ["-O1", "-g", "-fno-omit-frame-pointer",
                                                "-fsanitize=address,undefined", "-Wno-option-ignored"]
    procs, objs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(ASAN_DIR, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            cmd = [hipcc] + flags + EXTRA_FLAGS.get(src, []) + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=ASAN_DIR)))
    for src, p in procs:
        out = p.communicate()[0].decode(errors="replace")
        if p.returncode != 0:
            raise RuntimeError("hipcc (sanitized) failed on %s:\n%s" % (src, out))
    if force or procs or _stale(ASAN_LIB, objs):
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-fsanitize=address,undefined",
                               "-shared-libsan", "-o", ASAN_LIB] + objs)
    return ASAN_LIB


if __name__ == "__main__":
    if "--asan" in sys.argv:
        print(build_sanitized(force="--force" in sys.argv, verbose=True))
        sys.exit(0)
    print(build(force="--force" in sys.argv, save_temps="--save-temps" in sys.argv, verbose=True))
