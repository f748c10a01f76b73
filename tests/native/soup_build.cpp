// soup_build.cpp — the host builders on triangle soups read from files, as a
// stand-alone program: tests/test_hostile_ref.py builds it with AddressSanitizer
// and UBSan, where an out-of-bounds index or an out-of-range float-to-int
// conversion in bvh_build.cpp / bvh8_build.cpp aborts the run.
//
//   soup_build FILE...      each FILE: n x 9 float32 (v0 v1 v2 per triangle)
// Prints per file: name, triangles, BVH2 max depth, BVH8 depth at widths 8 and
// 6 for the SAH-optimal and the greedy collapse.
#include <cstdio>
#include <vector>

#include "bvh_build.h"

int main(int argc, char** argv) {
    for (int i = 1; i < argc; i++) {
        FILE* f = std::fopen(argv[i], "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
        std::vector<float> tv;
        float buf[9 * 256];
        size_t got;
        while ((got = std::fread(buf, sizeof(float), 9 * 256, f)) > 0) tv.insert(tv.end(), buf, buf + got);
        std::fclose(f);
        if (tv.size() % 9) { std::fprintf(stderr, "%s: not whole triangles\n", argv[i]); return 2; }
        const uint64_t n = tv.size() / 9;
        const spt::BvhBuildResult b2 = spt::build_bvh(tv.data(), n);
        if (b2.slot2tri.size() != n) return 1;
        std::printf("%s %llu %u", argv[i], (unsigned long long)n, b2.max_depth);
        for (int width : {8, 6})
            for (bool greedy : {false, true}) {
                const spt::Bvh8BuildResult b8 = spt::build_bvh8(tv.data(), n, greedy, width);
                if (b8.slot2tri.size() != n) return 1;
                std::printf(" %u", b8.depth);
            }
        std::printf("\n");
    }
    return 0;
}
