"""Generate tissue_analysis_amd/csrc/ta_pin_tables.inc: the Pin<BASE> specialisations of kernels_scan.hip.

    python scripts/gen_pin_tables.py            # rewrite the .inc
    python scripts/gen_pin_tables.py --check    # exit 1 when the committed .inc differs (tests/test_capi_symbols.py runs this)

A Pin<BASE> names, by number, the VGPRs above a kernel's amdgpu_num_vgpr budget in which the plane in flight lands
(register numbers must be literals inside inline asm, so the tables are written out by this script rather than by hand).
Which tables exist -- one per row of SCAN_VARIANTS in kernels_scan.hip: the first pinned register and the layout of the
zone -- is read from there; how many registers a layout takes (the clobber lists below) from build.ZONE_REGS:
  ROWS_HALO: rows 0..3 of the wave tile = v[BASE .. BASE+15], the row above = v[BASE+16 .. BASE+19], the voxels left of the
    rows = v[BASE+20]; with two rows per wave (RB = 2) the row above is the third quad and the voxel v[BASE+12];
  ROWS: the rows only; TWO_ROWS: two rows per wave only; WIDE: two rows of eight uint32 voxels a lane."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tissue_analysis_amd.build import ZONE_REGS, read_variants      # noqa: E402

OUT = os.path.join(ROOT, "tissue_analysis_amd", "csrc", "ta_pin_tables.inc")


def clobbers(base, n):
    return '"memory", ' + ", ".join('"v%d"' % (base + i) for i in range(n))


def movs(base, n):
    return " ".join('"v_mov_b32 %%%d, v%d\\n"' % (i, base + i) for i in range(n))


def strips(fn, width, base, quads, c, note=()):
    """issue_strip<Q>: a 16-byte strip into quad Q; issue_half<Q>: an 8-byte strip (four voxels of a uint16 volume) into its first two registers."""
    o = ["    template <int Q> static __device__ __forceinline__ void %s(uint32_t voff, const void* sbase) {" % fn, *note]
    for q in range(quads):
        head = "if (Q == %d)" % q if q == 0 else ("else if (Q == %d)" % q if q < quads - 1 else "else")
        o.append('        %s asm volatile("global_load_dwordx%d v[%d:%d], %%0, %%1" :: "v"(voff), "s"(sbase) : %s);'
                 % (head, width, base + 4 * q, base + 4 * q + width - 1, c))
    return o + ["    }"]


def table(base, n):
    adj = n == 21
    c = clobbers(base, n)
    o = ["template <> struct Pin<%d> {" % base] + strips("issue_strip", 4, base, n // 4, c) + strips("issue_half", 2, base, n // 4, c)
    if adj:
        o.append("    template <typename T, int RB> static __device__ __forceinline__ void issue_voxel(uint32_t voff, const void* sbase) {")
        for wide, four, reg in ((True, True, base + 20), (True, False, base + 12), (False, True, base + 20), (False, False, base + 12)):
            o.append('        if (sizeof(T) %s 4 && RB %s 4) asm volatile("global_load_%s v%d, %%0, %%1" :: "v"(voff), "s"(sbase) : %s);'
                     % ("==" if wide else "!=", "==" if four else "!=", "dword" if wide else "ushort", reg, c))
        o.append("    }")
    else:
        o.append("    template <typename T, int RB> static __device__ __forceinline__ void issue_voxel(uint32_t, const void*) {}")
    o.append("    template <int RB> static __device__ __forceinline__ void landed(u32x4 (&raw)[RB], u32x4& upr, uint32_t& l) {")
    rows4 = ('"=&v"(raw[0].x), "=&v"(raw[0].y), "=&v"(raw[0].z), "=&v"(raw[0].w),\n'
             '                           "=&v"(raw[1].x), "=&v"(raw[1].y), "=&v"(raw[1].z), "=&v"(raw[1].w),\n'
             '                           "=&v"(raw[RB > 2 ? 2 : 0].x), "=&v"(raw[RB > 2 ? 2 : 0].y), "=&v"(raw[RB > 2 ? 2 : 0].z), "=&v"(raw[RB > 2 ? 2 : 0].w),\n'
             '                           "=&v"(raw[RB > 3 ? 3 : 0].x), "=&v"(raw[RB > 3 ? 3 : 0].y), "=&v"(raw[RB > 3 ? 3 : 0].z), "=&v"(raw[RB > 3 ? 3 : 0].w)')
    rows2 = ('"=&v"(raw[0].x), "=&v"(raw[0].y), "=&v"(raw[0].z), "=&v"(raw[0].w),\n'
             '                           "=&v"(raw[1].x), "=&v"(raw[1].y), "=&v"(raw[1].z), "=&v"(raw[1].w)')
    halo = ', "=&v"(upr.x), "=&v"(upr.y), "=&v"(upr.z), "=&v"(upr.w), "=&v"(l)' if adj else ""
    o.append("        if (RB == 4) {")
    o.append('            asm volatile("s_waitcnt vmcnt(0)\\n" %s' % movs(base, n))
    o.append("                         : %s%s" % (rows4, halo))
    o.append('                         :: "memory");')
    o.append("        } else {")
    o.append('            asm volatile("s_waitcnt vmcnt(0)\\n" %s' % movs(base, n - 8))
    o.append("                         : %s%s" % (rows2, halo))
    o.append('                         :: "memory");')
    o.append("        }")
    if not adj:
        o.append("        (void)upr; (void)l;")
    o.append("    }")
    o.append("};")
    return "\n".join(o)


def table_two_rows(base, n):
    c = clobbers(base, n)
    note = ["        // (Q > 2 is never issued with two rows per wave; the branch exists only because the caller's `if (RB > 2)` is not constexpr)"]
    o = ["template <> struct Pin<%d> {" % base] + strips("issue_strip", 4, base, 3, c, note) + strips("issue_half", 2, base, 3, c)
    o.append("    template <typename T, int RB> static __device__ __forceinline__ void issue_voxel(uint32_t voff, const void* sbase) {")
    o.append('        static_assert(RB == 2, "this budget holds two rows");')
    o.append('        if (sizeof(T) == 4) asm volatile("global_load_dword v%d, %%0, %%1" :: "v"(voff), "s"(sbase) : %s);' % (base + n - 1, c))
    o.append('        else asm volatile("global_load_ushort v%d, %%0, %%1" :: "v"(voff), "s"(sbase) : %s);' % (base + n - 1, c))
    o.append("    }")
    o.append("    template <int RB> static __device__ __forceinline__ void landed(u32x4 (&raw)[RB], u32x4& upr, uint32_t& l) {")
    o.append('        static_assert(RB == 2, "this budget holds two rows");')
    o.append('        asm volatile("s_waitcnt vmcnt(0)\\n" %s' % movs(base, n))
    o.append('                     : "=&v"(raw[0].x), "=&v"(raw[0].y), "=&v"(raw[0].z), "=&v"(raw[0].w),')
    o.append('                       "=&v"(raw[1].x), "=&v"(raw[1].y), "=&v"(raw[1].z), "=&v"(raw[1].w), "=&v"(upr.x), "=&v"(upr.y), "=&v"(upr.z), "=&v"(upr.w), "=&v"(l)')
    o.append('                     :: "memory");')
    o.append("    }")
    o.append("};")
    return "\n".join(o)


def table_wide(base, n):
    """Two rows of EIGHT uint32 voxels a lane: six quads (row 0 low / high half, row 1 low / high, the row above low / high)
    and the voxel to the left."""
    c = clobbers(base, n)
    o = ["template <> struct Pin<%d> {" % base] + strips("issue_strip", 4, base, 6, c)
    o.append("    template <typename T, int RB> static __device__ __forceinline__ void issue_voxel(uint32_t voff, const void* sbase) {")
    o.append('        static_assert(sizeof(T) == 4 && RB == 2, "this layout holds two rows of a uint32 volume");')
    o.append('        asm volatile("global_load_dword v%d, %%0, %%1" :: "v"(voff), "s"(sbase) : %s);' % (base + n - 1, c))
    o.append("    }")
    o.append("    static __device__ __forceinline__ void landed_wide(u32x4 (&q)[6], uint32_t& l) {")
    o.append('        asm volatile("s_waitcnt vmcnt(0)\\n" %s' % movs(base, n))
    outs = ["\"=&v\"(q[%d].x), \"=&v\"(q[%d].y), \"=&v\"(q[%d].z), \"=&v\"(q[%d].w)" % (k, k, k, k) for k in range(6)]
    o.append("                     : " + (",\n                       ").join(outs) + ', "=&v"(l)')
    o.append('                     :: "memory");')
    o.append("    }")
    o.append("};")
    return "\n".join(o)


def render():
    head = ("// ta_pin_tables.inc -- GENERATED by scripts/gen_pin_tables.py (do not edit; `--check` compares): the hand-pinned landing\n"
            "// registers of the sweep kernels, one Pin<BASE> per VGPR budget, BASE = the first register above amdgpu_num_vgpr.\n")
    write = {"ROWS_HALO": table, "ROWS": table, "TWO_ROWS": table_two_rows, "WIDE": table_wide}
    return head + "\n".join(write[zone](base, ZONE_REGS[zone]) for _, zone, base in read_variants()) + "\n"


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if os.path.exists(OUT) and open(OUT).read() == text else 1)
    open(OUT, "w").write(text)
    print(OUT)
