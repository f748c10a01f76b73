// light_check.cpp — the host side of light sampling as a stand-alone program
// (tests/test_nee_host.py builds it with AddressSanitizer and UBSan):
//
//   light_check hash            rows "pixel sample depth k" on stdin: one line of
//                               light_uniform's float bits (hex) per row
//   light_check map             rows "xi1bits xi2bits" (hex): "b1bits b2bits" of light_tri_map
//   light_check soup FILE...    each FILE n x 9 float32 (v0 v1 v2 per triangle): the
//                               table of the soup with one emitting material, then with
//                               a non-monotone material order — prints per file
//                               "name triangles lights chosen_flat non_monotone"
//                               (the last two must be 0: a light a number can choose
//                               has an area, so a unit normal and a pdf that is not
//                               NaN or negative — it may underflow to 0 in f32 when
//                               the table's area is astronomic; the cdf never decreases)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "light_table.h"
#include "spt_math.h"

static int check_table(const spt::LightTable& lt, unsigned* zero_pdf, unsigned* non_monotone) {
    const size_t n = lt.ids.size();
    if (lt.cdf.size() != n || lt.pdfA.size() != n || lt.rec.size() != n * spt::kLightFloats) return 1;
    if (n && lt.cdf[n - 1] != 1.0f) return 1;
    float prev = 0.0f;
    for (size_t i = 0; i < n; i++) {
        if (!(lt.cdf[i] >= prev)) (*non_monotone)++;
        // the numbers in [prev, cdf_i) choose light i
        const float* nr = &lt.rec[i * spt::kLightFloats + 9];
        const float n2 = nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2];
        if (lt.cdf[i] > prev && (!(n2 > 0.99f && n2 < 1.01f) || !(lt.pdfA[i] >= 0.0f))) (*zero_pdf)++;
        if (i && lt.ids[i] <= lt.ids[i - 1]) return 1;
        prev = lt.cdf[i];
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    char line[256];
    if (!std::strcmp(argv[1], "hash")) {
        while (std::fgets(line, sizeof(line), stdin)) {
            unsigned long long c[4];
            if (std::sscanf(line, "%llu %llu %llu %llu", &c[0], &c[1], &c[2], &c[3]) != 4) continue;
            std::printf("%08x\n", spt::f2u(spt::light_uniform((uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2], (uint32_t)c[3])));
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "map")) {
        while (std::fgets(line, sizeof(line), stdin)) {
            unsigned a, b;
            if (std::sscanf(line, "%x %x", &a, &b) != 2) continue;
            float b1, b2;
            spt::light_tri_map(spt::u2f(a), spt::u2f(b), b1, b2);
            std::printf("%08x %08x\n", spt::f2u(b1), spt::f2u(b2));
        }
        return 0;
    }
    if (std::strcmp(argv[1], "soup")) return 2;
    for (int i = 2; i < argc; i++) {
        FILE* f = std::fopen(argv[i], "rb");
        if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
        std::vector<float> tv;
        float buf[9 * 256];
        size_t got;
        while ((got = std::fread(buf, sizeof(float), 9 * 256, f)) > 0) tv.insert(tv.end(), buf, buf + got);
        std::fclose(f);
        if (tv.size() % 9) { std::fprintf(stderr, "%s: not whole triangles\n", argv[i]); return 2; }
        const uint64_t n = tv.size() / 9;
        unsigned zero_pdf = 0, non_monotone = 0;
        spt::LightTable lt;
        const float one[3] = {1.0f, 2.0f, 3.0f};
        spt::light_table_build(tv.data(), nullptr, n, one, 1, lt);
        const size_t all = lt.ids.size();
        if (check_table(lt, &zero_pdf, &non_monotone)) return 1;
        if (all != 0 && all != n) return 1;  // every triangle is a member, or the table is empty
        // materials 2, 0, 1, 2, ... (out of range included): 0 and 1 emit, 1 far brighter
        std::vector<int32_t> mat(n);
        for (uint64_t t = 0; t < n; t++) mat[t] = (int32_t)((t + 2) % 4) - (t % 7 == 0 ? 5 : 0);
        const float two[6] = {0.0f, 0.5f, 0.0f, 1e30f, 0.0f, 1e-30f};
        spt::light_table_build(tv.data(), mat.data(), n, two, 2, lt);
        if (check_table(lt, &zero_pdf, &non_monotone)) return 1;
        std::printf("%s %llu %zu %u %u\n", argv[i], (unsigned long long)n, all, zero_pdf, non_monotone);
    }
    return 0;
}
