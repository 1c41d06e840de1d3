#!/usr/bin/env python3
"""The sweep is only changed against identical assembly: this compares it.

    python scripts/compare_sweep_asm.py [--rev REV] [-DNAME[=V] ...]

tissue_analysis_amd/csrc of REV (default HEAD~1) is taken out of git into a temporary directory; kernels_scan.hip and
kernels_walls.hip (which includes ta_sweep_common.h) of that tree and of the working tree are compiled device-only to assembly
with build.FLAGS plus the given defines, and compared per symbol as profiles/refactor_sweep_variants_isa.txt describes: lines
that carry the random __hip_cuid_ symbol are dropped and the index of the function in its file is taken out of its local labels
(.LBB<n>_, BB<n>_, .Lfunc_end<n>); nothing else is normalised.  A function's text runs from its .section / .text line to the end
of its "Kernel info" block; a kernel's metadata entry is part of its verdict.  Exit status 1 on any difference.
"""
import concurrent.futures, hashlib, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("kernels_scan.hip", "kernels_walls.hip")
CSRC = "tissue_analysis_amd/csrc"
_LABEL = re.compile(r"(\.LBB|\bBB|\.Lfunc_end)\d+")
_FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def split_asm(text):
    """{symbol: normalised text of the function}, {kernel: its metadata entry}, the text outside both."""
    lines = [l for l in text.split("\n") if "__hip_cuid_" not in l]
    funcs, meta, outside, i, in_kernels = {}, {}, [], 0, False
    while i < len(lines):
        m = re.search(r"; -- Begin function (\S+)", lines[i + 1]) if i + 1 < len(lines) else None
        if m and re.match(r"\s*\.(section|text)\b", lines[i]):
            j = next(k for k in range(i, len(lines)) if ".AMDGPU.csdata" in lines[k]) + 1
            while j < len(lines) and lines[j].startswith(";"):
                j += 1
            funcs[m.group(1)] = _LABEL.sub(r"\1", "\n".join(lines[i:j]))
        elif in_kernels and lines[i].startswith("  - "):
            j = i + 1
            while j < len(lines) and lines[j].startswith("    "):
                j += 1
            entry = "\n".join(lines[i:j])
            meta[re.search(r"\.name:\s+(\S+)", entry).group(1)] = entry
        else:
            in_kernels = lines[i].startswith("amdhsa.kernels:")
            outside.append(lines[i])
            j = i + 1
        i = j
    return funcs, meta, "\n".join(outside)


def _resources(entry):
    return " ".join(re.search(re.escape(f) + r":\s+(\d+)", entry).group(1) for f in _FIELDS) if entry else "-"


def compare_texts(parent, branch):
    """The rows (symbol, resources parent, resources branch, hash parent, hash branch, verdict) of two assembly texts and
    whether everything -- symbol sets, every function, every metadata entry, the text outside them -- is identical."""
    (fa, ma, oa), (fb, mb, ob) = split_asm(parent), split_asm(branch)
    rows, same = [], set(fa) == set(fb) and oa == ob
    if oa != ob:
        rows.append(("(text outside the functions: header, trailer)", "-", "-", "", "", "differs"))
    for sym in sorted(set(fa) | set(fb)):
        ha, hb = ("missing" if sym not in f else hashlib.sha256(f[sym].encode()).hexdigest()[:16] for f in (fa, fb))
        ok = ha == hb and ma.get(sym) == mb.get(sym)
        same = same and ok
        rows.append((sym, _resources(ma.get(sym)), _resources(mb.get(sym)), ha, hb, "identical" if ok else "differs"))
    return rows, same


def report(name, parent, branch, out=sys.stdout):
    rows, same = compare_texts(parent, branch)
    out.write("## %s\n# symbol | vgpr sgpr lds scratch (parent) | (branch) | sha256[:16] of text parent | branch | verdict\n" % name)
    out.write("".join(" | ".join(r) + "\n" for r in rows))
    out.write("%s: %s\n" % (name, "every function's text and every kernel's metadata identical" if same else "DIFFERS"))
    return same


def main(argv):
    sys.path.insert(0, ROOT)
    from tissue_analysis_amd import build
    rev, defines, args = "HEAD~1", [], list(argv)
    while args:
        a = args.pop(0)
        if a == "--rev":
            rev = args.pop(0)
        elif a.startswith("-D"):
            defines.append(a)
        else:
            sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        trees = {"parent": os.path.join(tmp, CSRC), "branch": os.path.join(ROOT, CSRC)}

        def compile_one(job):
            tree, src = job
            out = os.path.join(tmp, "%s_%s.s" % (tree, src))
            cmd = [build._hipcc()] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + defines
            run = subprocess.run(cmd + ["--cuda-device-only", "-S", os.path.join(trees[tree], src), "-o", out], cwd=tmp,
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            if run.returncode:
                sys.exit("hipcc failed on the %s's %s:\n%s" % (tree, src, run.stdout.decode(errors="replace")))
            return job, open(out).read()
        with concurrent.futures.ThreadPoolExecutor(build._jobs()) as pool:
            asm = dict(pool.map(compile_one, [(t, s) for s in SOURCES for t in trees]))
    print("parent %s, flags: %s" % (rev, " ".join(build.FLAGS + defines + ["%s: %s" % (s, " ".join(f)) for s, f in build.EXTRA_FLAGS.items() if s in SOURCES])))
    return 0 if all([report(s, asm["parent", s], asm["branch", s]) for s in SOURCES]) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
