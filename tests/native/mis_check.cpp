// mis_check.cpp — the MIS weights as a stand-alone host program
// (tests/test_mis_host.py builds it with AddressSanitizer and UBSan): the
// functions the fused kernel calls (spt_math.h), evaluated on rows of float32
// that the Python side writes, one line of result bits (hex) per row.
//
//   mis_check cx FILE       rows nh[3] d[3]: bounce_cx(nh, d, 1 / sqrt(d . d))
//   mis_check cl FILE       rows pdfA r2 cy: mis_light_cl
//   mis_check pair FILE     rows c sb: "mis_shadow_factor mis_bounce_weight"
//   mis_check hit FILE      rows cb s ng[3] pdfA d[3] t: mis_light_hit_weight
//   mis_check escape FILE   rows cb s pdf: mis_escape_weight
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "spt_math.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const char* mode = argv[1];
    const size_t cols = !std::strcmp(mode, "cx") ? 6 : !std::strcmp(mode, "cl") ? 3 : !std::strcmp(mode, "pair") ? 2
                        : !std::strcmp(mode, "hit") ? 10 : !std::strcmp(mode, "escape") ? 3 : 0;
    if (!cols) return 2;
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    std::vector<float> v;
    float buf[1024];
    size_t got;
    while ((got = std::fread(buf, sizeof(float), 1024, f)) > 0) v.insert(v.end(), buf, buf + got);
    std::fclose(f);
    if (v.size() % cols) { std::fprintf(stderr, "%s: not whole rows of %zu\n", argv[2], cols); return 2; }
    for (size_t i = 0; i + cols <= v.size(); i += cols) {
        const float* r = &v[i];
        if (cols == 6) {
            const spt::V3 d = spt::v3(r[3], r[4], r[5]);
            std::printf("%08x\n", spt::f2u(spt::bounce_cx(spt::v3(r[0], r[1], r[2]), d, 1.0f / sqrtf(spt::dot(d, d)))));
        } else if (cols == 2) {
            std::printf("%08x %08x\n", spt::f2u(spt::mis_shadow_factor(r[0], r[1])), spt::f2u(spt::mis_bounce_weight(r[0], r[1])));
        } else if (cols == 10) {
            std::printf("%08x\n", spt::f2u(spt::mis_light_hit_weight(r[0], r[1], spt::v3(r[2], r[3], r[4]), r[5],
                                                                     spt::v3(r[6], r[7], r[8]), r[9])));
        } else if (!std::strcmp(mode, "cl")) {
            std::printf("%08x\n", spt::f2u(spt::mis_light_cl(r[0], r[1], r[2])));
        } else {
            std::printf("%08x\n", spt::f2u(spt::mis_escape_weight(r[0], r[1], r[2])));
        }
    }
    return 0;
}
