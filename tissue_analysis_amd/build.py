"""Build recipe for libtissue_scan.so (hipcc, gfx950 only, in-tree).

    python -m tissue_analysis_amd.build [--force] [--save-temps]

hipcc cross-compiles without a GPU; the built .so is git-ignored but travels with the tree.

Every *.hip file of csrc/ is a source; build(), build_sanitized() and scripts/build_variant.py are calls of compile_and_link,
which says what makes an object current.  `--save-temps` is part of the recorded command like any flag: asking for it
recompiles everything, and so does the next plain build.  dependencies(source) answers why a change rebuilt an object.
"""
from __future__ import annotations

import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJDIR = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libtissue_scan.so")
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
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
SAVE_TEMPS = ["-save-temps=obj", "-Rpass-analysis=kernel-resource-usage"]      # after -o: intermediates and the resource-usage remarks


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


def _check_pinned(hipcc, objdir, flags, verbose=False):
    """Refuse a build in which compiler-allocated code reaches the hand-pinned registers (pinned_violations): kernels_scan.hip
    compiled to assembly in `objdir` with the `flags` its object there was made with."""
    asm = os.path.join(objdir, "kernels_scan.check.s")
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(CSRC, "kernels_scan.hip"), "-o", asm]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=objdir)
    bad = pinned_violations(open(asm).read(), read_variants())
    if bad:
        raise RuntimeError("compiler-allocated VGPRs reach the hand-pinned registers in kernels_scan.hip:\n  %s"
                           % "\n  ".join(bad[:10]))


def _jobs():
    """How many compilers run at a time: $MAX_JOBS, 16 by default and at the most."""
    try:
        return max(1, min(16, int(os.environ.get("MAX_JOBS", "16"))))
    except ValueError:
        return 16


def _current(target, record, argv, compiler, base):
    """Whether `record` says that `target` was made by exactly `argv` under this `compiler`, and nothing it was made from
    (paths relative to `base`) is missing or newer than it.  A target without a record is never current."""
    try:
        rec = json.load(open(record))
        t = os.path.getmtime(target)
    except (OSError, ValueError):
        return False
    deps = [os.path.join(base, d) for d in rec.get("deps", [])]
    return (rec.get("argv") == argv and rec.get("compiler") == compiler
            and all(os.path.exists(d) and os.path.getmtime(d) <= t for d in deps))


def _write_record(record, argv, compiler, deps):
    with open(record, "w") as f:
        json.dump({"argv": argv, "compiler": compiler, "deps": deps}, f, indent=1)


def _parse_deps(rule, cwd, base):
    """The prerequisites of the make rule that `-MM` printed when run in `cwd`, as paths relative to `base`."""
    words = re.split(r"(?<!\\)\s+", rule.replace("\\\n", " ").split(":", 1)[1].strip())
    return [os.path.relpath(os.path.join(cwd, w.replace("\\ ", " ")), base) for w in words if w]


def compile_and_link(srcdir, sources, objdir, lib, flags, link_flags=(), extra_flags=None, defines=(), tail=None,
                     force=False, verbose=False, pin_check=False, report=None):
    """Compile those of `sources` (names in `srcdir`) whose objects in `objdir` are not current, at most $MAX_JOBS at a time, and
    link `lib` from all of them if it is not current.  Returns the sources it compiled.

    A source's command is hipcc + flags + extra_flags[source] + defines + -c/-o + tail[source], run in `objdir`; the link's is
    hipcc --offload-arch=gfx950 -shared -fPIC + link_flags + -o lib + the objects in the order of `sources`.  Each object has a
    record beside it (NAME.o.json): that argv with the resolved compiler in front, the compiler's version, and the files the
    source was preprocessed from, which a `--cuda-host-only -MM` run with the same flags and defines names while the
    compile runs.  (Not -MMD on the compile itself: the compiler derives the HIP compilation-unit id from its command line, so
    that would change every object.)  An object is current when its record says what would run now and none of those files is
    missing or newer than it.  The record is removed before the compile and written after it succeeded, so a failed compile is
    never skipped by the next call.  The library's record, in `objdir` too, does the same for the link, which also runs whenever
    an object was compiled.  `report(source, text)` gets what each successful compile printed; `pin_check` runs _check_pinned
    on the kernels_scan.hip of CSRC."""
    hipcc = _hipcc()
    resolved = os.path.realpath(shutil.which(hipcc) or hipcc)
    version = subprocess.check_output([hipcc, "--version"]).decode(errors="replace")
    compiler = " / ".join(line.strip() for line in version.splitlines() if "version" in line)
    extra_flags, tail = extra_flags or {}, tail or {}
    os.makedirs(objdir, exist_ok=True)
    objs, todo = [], []
    for src in sources:
        s = os.path.join(srcdir, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(o)
        front = [hipcc] + list(flags) + extra_flags.get(src, []) + list(defines)
        cmd = front + ["-c", s, "-o", o] + tail.get(src, [])
        if force or not _current(o, o + ".json", [resolved] + cmd[1:], compiler, srcdir):
            todo.append((src, o, cmd, front + ["--cuda-host-only", "-MM", s]))
    failed = False
    with concurrent.futures.ThreadPoolExecutor(_jobs()) as pool:
        runs = []
        for src, o, cmd, deps_cmd in todo:
            if os.path.exists(o + ".json"):
                os.remove(o + ".json")
            if verbose:
                print(" ".join(cmd))
            runs.append((pool.submit(subprocess.run, cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=objdir),
                         pool.submit(subprocess.run, deps_cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=objdir)))
        for (src, o, cmd, _), (compiled, listed) in zip(todo, runs):
            compiled, listed = compiled.result(), listed.result()
            out = compiled.stdout.decode(errors="replace")
            if compiled.returncode or listed.returncode:
                failed = True
                said = out if compiled.returncode else listed.stderr.decode(errors="replace")
                sys.stderr.write("hipcc failed on %s:\n%s\n" % (src, said))
                continue
            _write_record(o + ".json", [resolved] + cmd[1:], compiler, _parse_deps(listed.stdout.decode(), objdir, srcdir))
            if report:
                report(src, out)
    if failed:
        raise RuntimeError("hipcc compilation failed")
    if pin_check:
        stamp = os.path.join(objdir, "kernels_scan.check.ok")       # (a failed check must not be skipped by the next call)
        if _stale(stamp, [os.path.join(objdir, "kernels_scan.o")]):
            _check_pinned(hipcc, objdir, list(flags) + extra_flags.get("kernels_scan.hip", []) + list(defines), verbose)
            open(stamp, "w").write("ok\n")
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + list(link_flags) + ["-o", lib] + objs
    record = os.path.join(objdir, os.path.basename(lib) + ".json")
    if force or todo or not _current(lib, record, [resolved] + cmd[1:], compiler, objdir):
        if os.path.exists(record):
            os.remove(record)
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        _write_record(record, [resolved] + cmd[1:], compiler, objs)
    return [src for src, _, _, _ in todo]


def build(force=False, save_temps=False, verbose=False):
    """Compile every HIP source for gfx950 and link libtissue_scan.so. Returns its path."""
    def show(src, out):
        if out.strip():
            print(out)
    compile_and_link(CSRC, SOURCES, OBJDIR, LIB, FLAGS, extra_flags=EXTRA_FLAGS,
                     tail={s: SAVE_TEMPS for s in SOURCES} if save_temps else None,
                     force=force, verbose=verbose, pin_check=True, report=show if verbose or save_temps else None)
    return LIB


def dependencies(source_name):
    """The files the product build's object of `source_name` was made from, as its record has them: paths relative to CSRC,
    the source itself first.  A change of any of them recompiles that source, and of nothing else but the command."""
    record = os.path.join(OBJDIR, source_name.replace(".hip", ".o") + ".json")
    if not os.path.exists(record):
        raise RuntimeError("%s has no build record: run build() first" % source_name)
    return json.load(open(record))["deps"]


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
    flags = [f for f in FLAGS if f != "-O3"] + ["-O1", "-g", "-fno-omit-frame-pointer",
                                                "-fsanitize=address,undefined", "-Wno-option-ignored"]
    compile_and_link(CSRC, SOURCES, ASAN_DIR, ASAN_LIB, flags, ["-fsanitize=address,undefined", "-shared-libsan"],
                     extra_flags=EXTRA_FLAGS, force=force, verbose=verbose)
    return ASAN_LIB


if __name__ == "__main__":
    if "--asan" in sys.argv:
        print(build_sanitized(force="--force" in sys.argv, verbose=True))
        sys.exit(0)
    print(build(force="--force" in sys.argv, save_temps="--save-temps" in sys.argv, verbose=True))
