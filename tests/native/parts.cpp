// parts.cpp -- csrc/ta_parts.h on its own, for tests/test_parts_cpu.py (plain host C++, no GPU).
//   parts   stdin: lines "from k" and k pairs "bytes align", then "end_align"
//           -> k lines "at bytes", then "end"
#include "ta_parts.h"

#include <cstdio>

// a layout as the host layer writes them, constant-evaluated: a cursor is usable in a constexpr constructor
struct Example {
    Part flags, rows, tail;
    uint64_t bytes = 0;
    constexpr explicit Example(uint64_t R) {
        PartCursor at;
        flags = at.take(16); rows = at.take(12 * R); tail = at.take(4 * R, 16);
        bytes = at.end(16);
    }
};
static_assert(Example(3).rows.at == 16 && Example(3).rows.bytes == 36 && Example(3).tail.at == 64 && Example(3).tail.bytes == 12 &&
              Example(3).bytes == 80, "flags u32[4] | rows [R][3] u32 | tail u32[R] from a multiple of 16, the buffer padded to one");
static_assert(Example(0).rows.bytes == 0 && Example(0).tail.at == 16 && Example(0).bytes == 16, "empty parts take no room");

int main() {
    unsigned long long from, bytes, align;
    int k;
    while (scanf("%llu %d", &from, &k) == 2) {
        PartCursor at(from);
        for (int i = 0; i < k; ++i) {
            if (scanf("%llu %llu", &bytes, &align) != 2 || !align) return 2;
            const Part p = at.take(bytes, align);
            printf("%llu %llu\n", (unsigned long long)p.at, (unsigned long long)p.bytes);
        }
        if (scanf("%llu", &align) != 1 || !align) return 2;
        printf("%llu\n", (unsigned long long)at.end(align));
    }
    return 0;
}
