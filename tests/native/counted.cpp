// counted.cpp -- the layouts of csrc/ta_counted.h on their own, for tests/test_counted_cpu.py (plain host C++, no HIP, no GPU).
//   stdin: lines "scan n from"           -> "counts.at counts.bytes offsets.at offsets.bytes scratch.at scratch.bytes end total_word per_block"
//                "sort n key_bytes from" -> "keys0 keys1 idx0 idx1 temp temp_bytes end"
//                "views"                 -> "ok", or the line of the check that failed
#define TA_COUNTED_LAYOUT_ONLY
#include "ta_counted.h"

#include <cstdio>
#include <cstring>
#include <vector>

// the temp of the radix sort is sized by kernels_wallsort.hip; here a stand-in that the test restates
uint64_t ta::wall_sort_temp_bytes(uint64_t n) { return 100 + 4 * (n / 7); }

static_assert(ta::SCAN_PER_BLOCK == 2048, "256 threads x 8");
static_assert(ScanBlock(0).scratch_part.bytes == 24 && ScanBlock(0).end == 32 && ta::scan_u32_total(0) == 0, "no counts: one word for the total, 16 bytes of slack");
static_assert(ScanBlock(1).offsets_part.at == 16 && ScanBlock(1).scratch_part.at == 32 && ScanBlock(1).scratch_part.bytes == 32 && ScanBlock(1).end == 64,
              "counts u32[n] | offsets u64[n] | block sums, total, slack: each from a multiple of 16");
static_assert(ScanBlock(2049).offsets_part.at == 8208 && ScanBlock(2049).scratch_part.at == 24608 && ScanBlock(2049).scratch_part.bytes == 40 &&
              ScanBlock(2049).end == 24656 && ta::scan_u32_total(2049) == 2, "two block sums, the total behind them");
static_assert(ScanBlock(1, 112).counts_part.at == 112 && ScanBlock(3, ScanBlock(3).end).counts_part.at == ScanBlock(3).end, "a block behind other parts");

#define CHECK(x) do { if (!(x)) { printf("line %d: %s\n", __LINE__, #x); return false; } } while (0)

template <class K> static bool views() {
    const uint64_t n = 5, from = 112;
    const SortLayout l(n, sizeof(K), from);
    std::vector<char> mem(l.end);
    char* base = mem.data();
    SortView<K> a(l, base), b(l, base);
    const auto inside = [&](const void* p, uint64_t bytes) { return (const char*)p >= base + from && (const char*)p + bytes <= base + l.end; };
    const auto distinct = [&](const SortView<K>& v) {
        const char* p[4] = {(const char*)v.keys(), (const char*)v.spare_keys(), (const char*)v.idx(), (const char*)v.spare_idx()};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
                if (p[i] == p[j]) return false;
        return inside(v.keys(), n * sizeof(K)) && inside(v.spare_keys(), n * sizeof(K)) && inside(v.idx(), n * 4) && inside(v.spare_idx(), n * 4) &&
               inside(v.temp, ta::wall_sort_temp_bytes(n));
    };
    CHECK((char*)a.keys() == base + l.keys[0] && (char*)a.spare_keys() == base + l.keys[1]);
    CHECK((char*)a.idx() == base + l.idx[0] && (char*)a.spare_idx() == base + l.idx[1] && (char*)a.temp == base + l.temp);
    CHECK(distinct(a));
    K* const first = a.keys(); K* const second = a.spare_keys();
    uint32_t* const ifirst = a.idx(); uint32_t* const isecond = a.spare_idx();
    a.sorted_into(first);                          // an even number of passes: the data stays where it was
    CHECK(a.keys() == first && a.spare_keys() == second && a.idx() == ifirst && a.spare_idx() == isecond);
    a.sorted_into(second);                         // the sorted pair is the second: current and spare swap
    CHECK(a.keys() == second && a.spare_keys() == first && a.idx() == isecond && a.spare_idx() == ifirst);
    CHECK(distinct(a));
    a.sorted_into(first);                          // ... and back, as the second sort of a chain does
    CHECK(a.keys() == first && a.idx() == ifirst && distinct(a));
    CHECK(b.keys() == first && b.idx() == ifirst && b.spare_keys() == second && distinct(b));      // a second view starts at pair 0 again
    return true;
}

int main() {
    char what[16];
    unsigned long long n, from;
    int key_bytes;
    while (scanf("%15s", what) == 1) {
        if (!strcmp(what, "scan")) {
            if (scanf("%llu %llu", &n, &from) != 2) return 2;
            const ScanBlock b(n, from);
            printf("%llu %llu %llu %llu %llu %llu %llu %llu %d\n", (unsigned long long)b.counts_part.at, (unsigned long long)b.counts_part.bytes,
                   (unsigned long long)b.offsets_part.at, (unsigned long long)b.offsets_part.bytes, (unsigned long long)b.scratch_part.at,
                   (unsigned long long)b.scratch_part.bytes, (unsigned long long)b.end, (unsigned long long)ta::scan_u32_total(n), ta::SCAN_PER_BLOCK);
        } else if (!strcmp(what, "sort")) {
            if (scanf("%llu %d %llu", &n, &key_bytes, &from) != 3) return 2;
            const SortLayout l(n, key_bytes, from);
            printf("%llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)l.keys[0], (unsigned long long)l.keys[1], (unsigned long long)l.idx[0],
                   (unsigned long long)l.idx[1], (unsigned long long)l.temp, (unsigned long long)ta::wall_sort_temp_bytes(n), (unsigned long long)l.end);
        } else if (!strcmp(what, "views")) {
            if (views<uint64_t>() && views<uint32_t>()) printf("ok\n");
        } else {
            return 2;
        }
    }
    return 0;
}
