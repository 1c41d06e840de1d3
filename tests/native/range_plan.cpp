// range_plan.cpp -- csrc/ta_range_plan.h on its own, for tests/test_range_plan_native.py (plain host C++, no GPU).
//   range_plan plan   stdin lines "n0 n1 n2 first_owned label_itemsize waves planes max_groups voxel_cap_log2"
//                     -> "ncb nrb npb tiles per groups"
//   range_plan vec    stdin lines "n2 label_itemsize k" and k pairs "address itemsize"  -> "0" or "1"
#include "ta_range_plan.h"

#include <cstdio>
#include <cstring>

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (!strcmp(argv[1], "plan")) {
        long long d[3], first, cap_groups;
        int itemsize, log2;
        ta::RangeShape shape;
        while (scanf("%lld %lld %lld %lld %d %d %d %lld %d", &d[0], &d[1], &d[2], &first, &itemsize, &shape.waves, &shape.planes, &cap_groups, &log2) == 9) {
            shape.max_groups = cap_groups;
            shape.voxel_cap_log2 = log2;
            const ta::RangeTiles t = ta::range_tiles(d[0], d[1], d[2], first, itemsize, shape);
            const ta::RangePlan p = ta::plan_ranges(t.tiles, t.tile_voxels, shape);
            printf("%lld %lld %lld %lld %u %u\n", (long long)t.ncb, (long long)t.nrb, (long long)t.npb, (long long)t.tiles, p.tiles_per_group, p.groups);
        }
        return 0;
    }
    if (!strcmp(argv[1], "vec")) {
        long long n2;
        int label_itemsize, k;
        while (scanf("%lld %d %d", &n2, &label_itemsize, &k) == 3) {
            ta::StripBuffer b[2] = {{nullptr, 0}, {nullptr, 0}};
            if (k < 1 || k > 2) return 2;
            for (int i = 0; i < k; ++i) {
                unsigned long long address;
                if (scanf("%llu %d", &address, &b[i].itemsize) != 2) return 2;
                b[i].p = (const void*)(uintptr_t)address;
            }
            printf("%d\n", (int)ta::strips_vectorize(n2, label_itemsize, {b[0], b[1]}));
        }
        return 0;
    }
    return 2;
}
