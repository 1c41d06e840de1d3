"""The cursor that lays out the parts of a device buffer (csrc/ta_parts.h), compiled on its own as plain host C++ and run:
offsets, alignment, empty parts, and the end behind an aligned tail.  The expected
numbers are worked out by hand, or by the two formulas the host layer used before the cursor: a part starts at the next multiple
of its alignment, and a buffer ends at the next multiple of its own."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "tissue_analysis_amd", "csrc")


@pytest.fixture(scope="module")
def parts_exe(tmp_path_factory):
    """tests/native/parts.cpp (its static_asserts are part of the test) built by the compiler of the build."""
    from tissue_analysis_amd import build as ta_build
    exe = str(tmp_path_factory.mktemp("parts") / "parts")
    subprocess.check_call([ta_build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "native", "parts.cpp"), "-o", exe])

    def run(from_, takes, end_align):
        text = "%d %d\n%s\n%d\n" % (from_, len(takes), " ".join("%d %d" % t for t in takes), end_align)
        out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, check=True, universal_newlines=True, timeout=60).stdout.split("\n")[:-1]
        assert len(out) == len(takes) + 1
        return [tuple(int(v) for v in line.split()) for line in out[:-1]], int(out[-1])
    return run


def test_parts_follow_each_other(parts_exe):
    parts, end = parts_exe(0, [(16, 1), (24, 1), (72, 1), (8, 1)], 1)
    assert parts == [(0, 16), (16, 24), (40, 72), (112, 8)] and end == 120


def test_a_part_starts_at_a_multiple_of_its_alignment(parts_exe):
    # flags | 65 doubles | then from multiples of 16 and of 256; an aligned offset stays where it is
    parts, end = parts_exe(0, [(16, 1), (520, 1), (48, 16), (16, 16), (4, 256), (1, 3)], 1)
    assert parts == [(0, 16), (16, 520), (544, 48), (592, 16), (768, 4), (774, 1)] and end == 775


def test_empty_parts_take_no_room_and_keep_their_place(parts_exe):
    parts, end = parts_exe(0, [(12, 1), (0, 1), (0, 16), (5, 1), (0, 1)], 1)
    assert parts == [(0, 12), (12, 0), (16, 0), (16, 5), (21, 0)] and end == 21
    assert parts_exe(0, [], 16) == ([], 0)


def test_the_end_pads_the_tail_not_the_cursor(parts_exe):
    parts, end = parts_exe(0, [(16, 1), (20, 16)], 16)
    assert parts == [(0, 16), (16, 20)] and end == 48                   # 36 bytes handed out, the buffer a multiple of 16
    assert parts_exe(0, [(16, 1), (20, 16)], 1)[1] == 36
    assert parts_exe(0, [(32, 16)], 16)[1] == 32                        # an aligned tail adds nothing


def test_a_cursor_that_starts_inside_a_buffer(parts_exe):
    # the sort workspace behind other parts: keys x 2, index x 2, temp, each padded to 16, as `at += align16(size)` laid them out
    align16 = lambda b: (b + 15) & ~15
    n, at, want = 5, 112, []
    for size in (n * 8, n * 8, n * 4, n * 4, 100):
        want.append((at, size))
        at += align16(size)
    parts, end = parts_exe(112, [(size, 16) for _, size in want], 16)
    assert parts == want and end == at == 112 + 48 + 48 + 32 + 32 + 112


def test_offsets_past_32_bits(parts_exe):
    big = (1 << 33) + 5
    parts, end = parts_exe(0, [(big, 1), (big, 16)], 16)
    assert parts == [(0, big), ((1 << 33) + 16, big)] and end == (1 << 34) + 32
