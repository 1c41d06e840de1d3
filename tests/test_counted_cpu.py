"""The layouts the count-then-emit passes share (csrc/ta_counted.h), compiled on their own as plain host C++ and run: the count/scan
block, the sort workspace behind other parts, and the views that follow a sort from one pair of buffers to the other.  The expected
numbers come from the formulas the code had before the header stated them once -- the scan's scratch and the place of its total
as kernels_walls.hip wrote them, the workspace as the `at += align16(size)` walk of test_parts_cpu.py -- never from the header."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "tissue_analysis_amd", "csrc")

SCAN_PER_BLOCK = 2048          # 256 threads x 8
align16 = lambda b: (b + 15) & ~15


def scan_scratch_bytes(n):
    """uint64_t scan_u32_scratch_bytes(uint64_t n) { return ((n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK + 1) * 8 + 16; }"""
    return ((n + SCAN_PER_BLOCK - 1) // SCAN_PER_BLOCK + 1) * 8 + 16


def scan_total_word(n):
    """uint64_t* scan_u32_total(void* scratch, uint64_t n) { return (uint64_t*)scratch + (n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK; }"""
    return (n + SCAN_PER_BLOCK - 1) // SCAN_PER_BLOCK


def sort_temp_bytes(n):
    """The stand-in of tests/native/counted.cpp for the radix sort's own temp size."""
    return 100 + 4 * (n // 7)


@pytest.fixture(scope="module")
def counted(tmp_path_factory):
    """tests/native/counted.cpp (its static_asserts are part of the test) built by the compiler of the build."""
    from tissue_analysis_amd import build as ta_build
    exe = str(tmp_path_factory.mktemp("counted") / "counted")
    subprocess.check_call([ta_build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(HERE, "native", "counted.cpp"), "-o", exe])

    def run(line):
        out = subprocess.run([exe], input=line + "\n", stdout=subprocess.PIPE, check=True, universal_newlines=True, timeout=60).stdout.split("\n")
        assert len(out) == 2 and out[1] == ""
        return out[0]
    return run


@pytest.mark.parametrize("from_", [0, 112])
@pytest.mark.parametrize("n", [0, 1, SCAN_PER_BLOCK - 1, SCAN_PER_BLOCK, SCAN_PER_BLOCK + 1, 2 * SCAN_PER_BLOCK + 1, (1 << 32) + 5])
def test_the_scan_block(counted, n, from_):
    c_at, c_bytes, o_at, o_bytes, s_at, s_bytes, end, total_word, per_block = (int(v) for v in counted("scan %d %d" % (n, from_)).split())
    assert per_block == SCAN_PER_BLOCK
    parts = [(c_at, c_bytes), (o_at, o_bytes), (s_at, s_bytes)]
    assert [b for _, b in parts] == [4 * n, 8 * n, scan_scratch_bytes(n)]                # counts u32[n] | offsets u64[n] | scratch
    assert all(at % 16 == 0 for at, _ in parts) and end % 16 == 0
    assert c_at >= from_ and all(parts[i][0] + parts[i][1] <= parts[i + 1][0] for i in range(2)) and s_at + s_bytes <= end   # no overlap
    assert end - from_ < 4 * n + 8 * n + scan_scratch_bytes(n) + 4 * 16                  # ... and nothing but padding between them
    blocks = -(-n // SCAN_PER_BLOCK)
    assert s_bytes == (blocks + 1) * 8 + 16                                              # ceil(n / SCAN_PER_BLOCK) + 1 words, 16 bytes of slack
    assert total_word == scan_total_word(n) == blocks and 8 * (total_word + 1) + 16 == s_bytes      # the total: the word behind the block sums


@pytest.mark.parametrize("key_bytes", [4, 8])
@pytest.mark.parametrize("n", [0, 1, 5, 1 << 31])
def test_the_sort_workspace_behind_other_parts(counted, n, key_bytes):
    at, want = 112, []
    for size in (n * key_bytes, n * key_bytes, n * 4, n * 4, sort_temp_bytes(n)):
        want.append(at)
        at += align16(size)
    got = [int(v) for v in counted("sort %d %d 112" % (n, key_bytes)).split()]
    assert got[5] == sort_temp_bytes(n)
    assert got[:5] == want and got[6] == at
    if (n, key_bytes) == (5, 8):
        assert got[6] == 112 + 48 + 48 + 32 + 32 + 112            # the numbers of test_parts_cpu.py::test_a_cursor_that_starts_inside_a_buffer


def test_views_follow_the_sort_from_pair_to_pair(counted):
    assert counted("views") == "ok"
