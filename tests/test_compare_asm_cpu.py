"""scripts/compare_sweep_asm.py: the per-symbol comparison, on small synthetic assembly texts."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import compare_sweep_asm as cmp_asm      # noqa: E402


def _function(sym, index, body="\tv_add_u32_e32 v0, 8, v0"):
    return "\n".join(["\t.section\t.text.%s,\"axG\",@progbits,%s,comdat" % (sym, sym),
                      "\t.protected\t%s ; -- Begin function %s" % (sym, sym), "%s: ; @%s" % (sym, sym),
                      "\ts_cbranch_execz .LBB%d_2" % index, body, ".LBB%d_2: ; in Loop: Header=BB%d_1 Depth=1" % (index, index),
                      "\ts_endpgm", ".Lfunc_end%d:" % index, "\t.size\t%s, .Lfunc_end%d-%s" % (sym, index, sym),
                      "\t.section\t.AMDGPU.csdata,\"\",@progbits", "; Kernel info:", "; NumVgprs: 95"])


def _meta(sym, vgprs=95):
    return "\n".join(["  - .agpr_count:     0", "    .group_segment_fixed_size: 29344", "    .name:           %s" % sym,
                      "    .private_segment_fixed_size: 112", "    .sgpr_count:     98", "    .vgpr_count:     %d" % vgprs])


def _file(functions, metas, cuid):
    return "\n".join(["\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\""] + functions +
                     ["\t.globl\t__hip_cuid_%s" % cuid, "\t.amdgpu_metadata", "---", "amdhsa.kernels:"] + metas +
                     ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "...", "\t.end_amdgpu_metadata", ""])


PARENT = _file([_function("_Zk1", 0), _function("_Zk2", 1)], [_meta("_Zk1"), _meta("_Zk2")], "aaaa")


def _verdicts(branch):
    rows, same = cmp_asm.compare_texts(PARENT, branch)
    return {r[0]: r[-1] for r in rows}, same


def test_swapped_order_and_renumbered_labels_are_identical():
    verdicts, same = _verdicts(_file([_function("_Zk2", 0), _function("_Zk1", 1)], [_meta("_Zk2"), _meta("_Zk1")], "bbbb"))
    assert same and verdicts == {"_Zk1": "identical", "_Zk2": "identical"}
    rows, _ = cmp_asm.compare_texts(PARENT, PARENT)
    assert rows[0][1] == "95 98 29344 112" and rows[0][3] == rows[0][4] and len(rows[0][3]) == 16


def test_one_changed_instruction_names_the_symbol():
    changed = _function("_Zk2", 1, body="\tv_add_u32_e32 v0, 4, v0")
    verdicts, same = _verdicts(_file([_function("_Zk1", 0), changed], [_meta("_Zk1"), _meta("_Zk2")], "aaaa"))
    assert not same and verdicts == {"_Zk1": "identical", "_Zk2": "differs"}
    verdicts, same = _verdicts(_file([_function("_Zk1", 0), _function("_Zk2", 1)], [_meta("_Zk1", vgprs=96), _meta("_Zk2")], "aaaa"))
    assert not same and verdicts == {"_Zk1": "differs", "_Zk2": "identical"}      # (the metadata entry is part of the verdict)


def test_missing_symbol_differs():
    verdicts, same = _verdicts(_file([_function("_Zk1", 0)], [_meta("_Zk1")], "aaaa"))
    assert not same and verdicts == {"_Zk1": "identical", "_Zk2": "differs"}
