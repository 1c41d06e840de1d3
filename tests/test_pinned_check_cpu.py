"""The build's guard of the sweep's hand-pinned landing zones (build.pinned_violations) on short hand-written assembly: the
text is about register NUMBERS only -- which kernel may name which VGPR outside its own inline asm."""
import os
import re

import pytest

from tissue_analysis_amd import build as B

VARIANTS = B.read_variants()
ARGS = "EEEvNS_9SweepArgsENS_9ScanSplitEj"
TWO_ROWS = "_ZN2ta20scan_two_rows_kernelIjLi4ELi2ELb1" + ARGS                 # pins v82 .. v94
WIDE = "_ZN2ta16scan_wide_kernelIjLi8ELi2ELb1ELb0" + ARGS                     # pins v102 .. v126
EDGE = "_ZN2ta11scan_kernelItLi8ELi2ELb1ELb1" + ARGS                          # EDGE = true: pins nothing
HELPER = "_ZN2taL17pair_spill_globalENS_9PairTableEPjjjjj"                    # a device function that was not inlined


def asm(sym, body, kernel=True):
    return "\n".join(["\t.type\t%s,@function" % sym, "%s: ; @%s" % (sym, sym), "; %bb.0:", "\ts_load_dwordx2 s[0:1], s[4:5], 0x0",
                      body, "\ts_endpgm", ".Lfunc_end0:"] + (["\t.amdhsa_kernel %s" % sym, "\t.end_amdhsa_kernel"] if kernel else []))


def test_the_table_reads_as_written():
    assert VARIANTS == [("scan_kernel", "ROWS_HALO", 104), ("scan_pad_kernel", "ROWS_HALO", 120), ("scan_noadj_kernel", "ROWS", 76),
                        ("scan_noadj_pad_kernel", "ROWS", 80), ("scan_two_rows_kernel", "TWO_ROWS", 82),
                        ("scan_pad2_kernel", "TWO_ROWS", 112), ("scan_wide_kernel", "WIDE", 102), ("scan_wide_pad_kernel", "WIDE", 116)]
    assert B.ZONE_REGS == {"ROWS_HALO": 21, "ROWS": 16, "TWO_ROWS": 13, "WIDE": 25}


@pytest.mark.parametrize("sym, body, refused", [
    (TWO_ROWS, "\tv_add_u32_e32 v82, v1, v2", True),                          # the first register of its 13
    (TWO_ROWS, "\tv_add_u32_e32 v3, v94, v2", True),                          # the last
    (TWO_ROWS, "\tv_add_u32_e32 v95, v1, v2", False),                         # the first past the zone
    (TWO_ROWS, "\tv_add_u32_e32 v81, v1, v2", False),                         # the last of the compiler's own
    (TWO_ROWS, "\tglobal_load_dwordx4 v[80:83], v1, s[2:3]", True),           # a range that overlaps the zone from below
    (TWO_ROWS, "\t;;#ASMSTART\n\tglobal_load_dwordx4 v[80:83], v1, s[2:3]\n\t;;#ASMEND", False),      # ... in the inline asm that owns it
    (TWO_ROWS, "\t;;#ASMSTART\n\tglobal_load_dwordx4 v[82:85], v1, s[2:3]\n\t;;#ASMEND\n\tv_mov_b32_e32 v83, v1", True),   # ... and after it
    (WIDE, "\tv_mov_b32_e32 v126, v1", True),                                 # the 25th register
    (WIDE, "\tv_mov_b32_e32 v127, v1", False),
    (WIDE, "\tv_mov_b32_e32 v101, v1", False),
    (EDGE, "\tv_mov_b32_e32 v110, v1", False),                                # an edge kernel: any register is its own
    (EDGE.replace("Lb1ELb1" + ARGS, "Lb1ELb0" + ARGS), "\tv_mov_b32_e32 v110, v1", True),             # the interior one of the same entry point
    (HELPER, "\tv_mov_b32_e32 v76, v1", True),                                # a device function: clear of EVERY zone (here scan_noadj_kernel's)
    (HELPER, "\tv_mov_b32_e32 v75, v1", False),
])
def test_which_registers_compiler_code_may_name(sym, body, refused):
    bad = B.pinned_violations(asm(sym, body, kernel=sym != HELPER), VARIANTS)
    assert bool(bad) == refused
    if refused:
        assert len(bad) == 1 and bad[0].startswith(sym + ":") and bad[0].endswith(body.split("\n")[-1].strip())


def test_a_scan_kernel_outside_the_table_is_named():
    sym = "_ZN2ta17scan_extra_kernelIjLi4ELi2ELb1" + ARGS
    with pytest.raises(RuntimeError, match=sym + " is in no row of SCAN_VARIANTS"):
        B.pinned_violations(asm(sym, "\tv_mov_b32_e32 v1, v2"), VARIANTS)
    assert B.pinned_violations(asm(sym, "\tv_mov_b32_e32 v1, v2", kernel=False), VARIANTS) == []      # (a device function may have any name)


def test_an_incomplete_table_is_refused_as_such():
    text = asm(TWO_ROWS, "\tv_mov_b32_e32 v1, v2")
    for table in ([], VARIANTS[:7], VARIANTS[:7] + [("scan_wide_pad_kernel", "NO_SUCH_LAYOUT", 116)]):
        with pytest.raises(RuntimeError, match="SCAN_VARIANTS in kernels_scan.hip\\) is incomplete"):
            B.pinned_violations(text, table)


def test_the_table_and_the_entry_points_are_the_same_set():
    src = open(os.path.join(B.CSRC, "kernels_scan.hip")).read()
    entry = re.findall(r"__global__[^\n]*?\b(scan_\w+)\(", src)
    assert sorted(entry) == sorted(n for n, _, _ in VARIANTS) and len(set(entry)) == len(entry)
    for name in entry:                   # each asks for its own row's budget and lands the plane in its own row's zone
        assert re.search(r"amdgpu_num_vgpr\(CAP_%s\)\)\) %s\(SweepArgs[^\n]*\n(?:[^\n}]*\n)?[^\n}]*\bPIN_%s>\(A, sp, wg0\);" % (name, name, name), src), name
    assert set(B.EDGE_LAST) == set(re.findall(r"EDGE \? 0 : PIN_(scan_\w+)>", src))
