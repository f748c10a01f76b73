// Writes the host builders' trees to a file for tests/bvh_audit.py
// (tests/test_bvh_audit.py): seeded triangle soups of 1, 9, 200 and 5000
// triangles — as generated, with every z equal (a zero-extent axis), with a
// far outlier vertex, with a +inf, a -inf and a NaN coordinate, and on a 1/8
// grid with coordinates of 1e-30 and 6e-17 among them — built
// with build_bvh8 (width 8 and 6, SAH-optimal and greedy collapse; width 6
// also as 64-B nodes, node6.h) and build_bvh, in the builders' compact layout.
// Host-only, its own main: built with the host C++ compiler together with
// bvh_build.cpp and bvh8_build.cpp.
//
// Per tree: 12 uint32 (magic, format 8 / 6 / 2, words per node, triangles,
// nodes, leaves, depth, largest leaf, soup size, variant, build, 0), the node
// words, slot2tri, the 16-float triangle records (spt_internal.h
// tri_record_fill) and the soup's 9 floats per triangle.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bvh_build.h"
#include "node6.h"

using namespace spt;

namespace {

struct Lcg {
    uint64_t s;
    float next() {  // [0, 1)
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((s >> 40) & 0xffffffu) / 16777216.0f;
    }
};

std::vector<float> soup(uint64_t n, uint64_t seed, int variant) {
    Lcg r{seed};
    std::vector<float> tv(n * 9);
    for (uint64_t t = 0; t < n; t++) {
        float c[3] = {r.next() * 10.0f - 5.0f, r.next() * 4.0f, r.next() * 10.0f - 5.0f};
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++) tv[t * 9 + k * 3 + a] = c[a] + (r.next() - 0.5f) * 0.6f;
    }
    if (variant == 1)
        for (uint64_t i = 0; i < n * 3; i++) tv[i * 3 + 2] = 0.5f;
    if (variant == 2) tv[(n / 2) * 9 + 4] += 1.0e4f;
    if (variant == 4) {  // round coordinates, and tiny ones beside them: differences that round in double
        for (float& x : tv) x = std::round(x * 8.0f) / 8.0f;
        for (uint64_t t = 0; t < n; t += 3) tv[t * 9 + (t % 9)] = (t & 1u) ? 6.0e-17f : -1.0e-30f;
        // triangle 0 spans x = -1e-30 .. 255 * 2^-7: the extent rounds to 255 steps of 2^-7 exactly
        tv[3] = 0.5f;
        tv[6] = 1.9921875f;
    }
    if (variant == 3) {
        tv[(n / 2) * 9 + 0] = INFINITY;
        tv[(n / 3) * 9 + 5] = -INFINITY;
        tv[(n / 5) * 9 + 7] = NAN;
    }
    return tv;
}

bool put(FILE* f, const void* p, size_t bytes) { return bytes == 0 || std::fwrite(p, bytes, 1, f) == 1; }

bool dump(FILE* f, uint32_t fmt, uint32_t stride, const std::vector<uint32_t>& nodes,
          const std::vector<uint32_t>& slot2tri, const std::vector<float>& tv, uint64_t leaves, uint32_t depth,
          uint32_t max_leaf, uint32_t variant, uint32_t build) {
    const uint32_t n = (uint32_t)slot2tri.size();
    std::vector<float> rec((size_t)n * 16, 0.0f);
    for (uint32_t s = 0; s < n; s++) {
        const float* v = &tv[(size_t)slot2tri[s] * 9];
        for (int k = 0; k < 3; k++) {
            float* r = &rec[(size_t)s * 16 + 5 * k];
            r[0] = v[3 * k]; r[1] = v[3 * k + 1]; r[2] = v[3 * k + 2]; r[3] = v[3 * k]; r[4] = v[3 * k + 1];
        }
        std::memcpy(&rec[(size_t)s * 16 + 15], &slot2tri[s], 4);
    }
    const uint32_t head[12] = {0x44485642u, fmt, stride, n, (uint32_t)(nodes.size() / stride), (uint32_t)leaves, depth,
                               max_leaf, n, variant, build, 0u};
    return put(f, head, sizeof(head)) && put(f, nodes.data(), nodes.size() * 4) && put(f, slot2tri.data(), n * 4ull) &&
           put(f, rec.data(), rec.size() * 4) && put(f, tv.data(), tv.size() * 4);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: bvh_dump OUT\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    bool ok = true;
    int trees = 0;
    for (uint64_t n : {1ull, 9ull, 200ull, 5000ull})
        for (int variant = 0; variant < 5; variant++) {
            const std::vector<float> tv = soup(n, 1234 + n, variant);
            for (uint32_t build = 0; build < 4; build++) {  // 0 / 1: width 8 optimal / greedy; 2 / 3: width 6
                const int width = build < 2 ? 8 : 6;
                const Bvh8BuildResult b = build_bvh8(tv.data(), n, (build & 1u) != 0, width);
                ok = ok && dump(f, 8, 20, b.nodes, b.slot2tri, tv, b.leaves, b.depth, 3, variant, build);
                trees++;
                if (width == 6) {
                    bool over = false;
                    const std::vector<uint32_t> n6 = to_node6(b.nodes, &over);
                    if (over) {
                        std::fprintf(stderr, "a width-6 tree has a node with more than six children\n");
                        ok = false;
                    }
                    ok = ok && dump(f, 6, 16, n6, b.slot2tri, tv, b.leaves, b.depth, 3, variant, build + 2);
                    trees++;
                }
            }
            const BvhBuildResult b2 = build_bvh(tv.data(), n);
            std::vector<uint32_t> n2(b2.nodes.size());
            std::memcpy(n2.data(), b2.nodes.data(), n2.size() * 4);
            ok = ok && dump(f, 2, 16, n2, b2.slot2tri, tv, b2.leaves, b2.max_depth, b2.max_leaf, variant, 6);
            trees++;
        }
    ok = std::fclose(f) == 0 && ok;
    std::printf("{\"trees\": %d, \"ok\": %d}\n", trees, ok ? 1 : 0);
    return ok ? 0 : 1;
}
