// sky_check.cpp — the host side of sky sampling as a stand-alone program
// (tests/test_sky_host.py builds it with AddressSanitizer and UBSan):
//
//   sky_check hash          rows "pixel sample depth k" on stdin: one line of
//                           sky_uniform's float bits (hex) per row
//   sky_check unfold        rows "abits bbits" (hex): "xbits ybits zbits" of sky_unfold
//   sky_check pdf FILE      FILE holds float32s: n, the 9 rotation entries, the n * n
//                           density plane, then directions (3 floats each): one line of
//                           sky_density's float bits per direction
//   sky_check build         sky_table_build on n = 1, 2 and 4096 and on hostile
//                           images; prints per case "name n cells bad" — bad counts
//                           broken invariants and must be 0: every cdf ends in 1 and
//                           never decreases, every density is finite and not
//                           negative, and a cell a number can draw has a positive one
//                           unless its probability underflows f32
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "sky_table.h"
#include "spt_math.h"

static unsigned check_table(const spt::SkyTable& t, uint32_t n) {
    if (t.empty()) return 0;
    unsigned bad = 0;
    const size_t nn = (size_t)n * n;
    if (t.n != n || t.marg.size() != n || t.cond.size() != nn || t.pdf.size() != nn) return 1;
    if (t.marg[n - 1] != 1.0f) bad++;
    float prev = 0.0f;
    for (uint32_t j = 0; j < n; j++) {
        if (!(t.marg[j] >= prev)) bad++;
        const bool drawn = t.marg[j] > prev;
        const double pm = (double)t.marg[j] - (double)prev;
        prev = t.marg[j];
        const float* c = &t.cond[(size_t)j * n];
        if (c[n - 1] != 1.0f) bad++;
        float pc = 0.0f;
        for (uint32_t i = 0; i < n; i++) {
            if (!(c[i] >= pc)) bad++;
            const float p = t.pdf[(size_t)j * n + i];
            if (!std::isfinite(p) || p < 0.0f) bad++;
            // a cell both cdfs can reach carries weight, so a density unless it underflows
            if (drawn && c[i] > pc && !(p > 0.0f) && ((double)c[i] - (double)pc) * pm > 1e-30) bad++;
            pc = c[i];
        }
    }
    return bad;
}

static void run_case(const char* name, const std::vector<float>& rgb, uint32_t n) {
    spt::SkyTable t;
    spt::sky_table_build(rgb.data(), n, t);
    std::printf("%s %u %zu %u\n", name, n, t.empty() ? (size_t)0 : t.pdf.size(), check_table(t, n));
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    char line[256];
    if (!std::strcmp(argv[1], "hash")) {
        while (std::fgets(line, sizeof(line), stdin)) {
            unsigned long long c[4];
            if (std::sscanf(line, "%llu %llu %llu %llu", &c[0], &c[1], &c[2], &c[3]) != 4) continue;
            std::printf("%08x\n", spt::f2u(spt::sky_uniform((uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2], (uint32_t)c[3])));
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "unfold")) {
        while (std::fgets(line, sizeof(line), stdin)) {
            unsigned a, b;
            if (std::sscanf(line, "%x %x", &a, &b) != 2) continue;
            const spt::V3 p = spt::sky_unfold(spt::u2f(a), spt::u2f(b));
            std::printf("%08x %08x %08x\n", spt::f2u(p.x), spt::f2u(p.y), spt::f2u(p.z));
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "pdf")) {
        if (argc < 3) return 2;
        FILE* f = std::fopen(argv[2], "rb");
        if (!f) return 2;
        std::vector<float> v;
        float buf[1024];
        size_t got;
        while ((got = std::fread(buf, sizeof(float), 1024, f)) > 0) v.insert(v.end(), buf, buf + got);
        std::fclose(f);
        if (v.size() < 10) return 2;
        const uint32_t n = (uint32_t)v[0];
        const size_t head = 10 + (size_t)n * n;
        if (n == 0 || v.size() < head || (v.size() - head) % 3) return 2;
        for (size_t k = head; k < v.size(); k += 3)
            std::printf("%08x\n", spt::f2u(spt::sky_density(n, &v[1], &v[10], spt::v3(v[k], v[k + 1], v[k + 2]))));
        return 0;
    }
    if (std::strcmp(argv[1], "build")) return 2;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    run_case("one", std::vector<float>{0.5f, 2.0f, 1.0f}, 1);
    run_case("one_zero", std::vector<float>{0.0f, 0.0f, 0.0f}, 1);
    {
        std::vector<float> v(12);
        for (size_t k = 0; k < v.size(); k++) v[k] = (float)(k % 5) * 0.25f;
        run_case("two", v, 2);
    }
    {
        const uint32_t n = 7;
        std::vector<float> v((size_t)n * n * 3);
        uint32_t s = 12345u;
        for (float& x : v) { s = s * 1664525u + 1013904223u; x = (float)(s >> 8) * (1.0f / 16777216.0f); }
        std::vector<float> h = v;
        h[0] = nan; h[4] = inf; h[8] = -inf; h[30] = -3.0f; h[31] = 3e38f; h[40] = 1e-45f;
        run_case("hostile", h, n);
        std::vector<float> allnan(v.size(), nan);
        run_case("all_nan", allnan, n);
        std::vector<float> huge(v.size(), 3e38f);
        run_case("huge", huge, n);
        std::vector<float> tiny(v.size(), 1e-45f);
        run_case("subnormal", tiny, n);
        std::vector<float> neg(v.size());
        for (size_t k = 0; k < v.size(); k++) neg[k] = -v[k];
        run_case("negative", neg, n);
        std::vector<float> lastrows = v;  // the last rows and columns carry no weight
        for (uint32_t j = 0; j < n; j++)
            for (uint32_t i = 0; i < n; i++)
                if (j >= 3 || i >= 3)
                    for (int c = 0; c < 3; c++) lastrows[((size_t)j * n + i) * 3 + c] = 0.0f;
        run_case("zero_tail", lastrows, n);
    }
    {
        const uint32_t n = 4096;
        std::vector<float> v((size_t)n * n * 3);
        uint32_t s = 99u;
        for (size_t k = 0; k < v.size(); k++) {
            s = s * 1664525u + 1013904223u;
            v[k] = (s >> 28) == 0 ? 1000.0f : (float)(s >> 8) * (1.0f / 16777216.0f);
        }
        run_case("large", v, n);
    }
    spt::SkyTable t;
    spt::sky_table_build(nullptr, 4, t);
    if (!t.empty()) return 1;
    const float one[3] = {1, 1, 1};
    spt::sky_table_build(one, 0, t);
    if (!t.empty()) return 1;
    spt::sky_table_build(one, 4097, t);
    if (!t.empty()) return 1;
    return 0;
}
