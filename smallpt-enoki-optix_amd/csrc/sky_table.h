// sky_table.h — the sampling table of a scene's sky image
// (spt_scene_set_sky_sampling), built on the host in f64 and
// rounded once.  Plain C++, no HIP: capi.cpp builds the scene's table with it,
// spt_sky_table_build exposes it, and tests/native/sky_check.cpp runs it under
// the sanitizers.
//
// For the n x n texels T(i, j) (column i, row j) as the scene stores them:
//   Y(i, j)    = max(|r|, |g|, |b|)                         (fmax: a NaN channel is skipped)
//   Ybar(i, j) = sum_{dy = -1..1} sum_{dx = -1..1} (k(dx) k(dy)) Y(wrap(i + dx, j + dy)),
//                k = {1/8, 3/4, 1/8}, added in that order from 0; wrap is the
//                octahedral edge rule (envmap_wrap: the column first, then the
//                row).  It is the mean of the bilinear interpolant of Y over the
//                texel's own cell, so it is positive wherever a lookup inside
//                the cell can be non-zero.
//   w(i, j)    = Ybar / l^3, l = sqrt((x x + y y) + z z) of the texel centre's
//                octahedron point p_c = (x, y, z) — the solid angle of the cell
//                per unit of its area; not finite or not positive: 0
//   row_j      = sum_i w(i, j), total = sum_j row_j         (both sequential)
//   marg_j     = f32(sum_{j' <= j} row_j' / total)          the last forced to 1
//   cond(i, j) = f32(sum_{i' <= i} w(i', j) / row_j)        the last of each row forced
//                to 1; a row of weight 0: zeros, then 1 (flat in marg, never drawn)
//   pdf(i, j)  = f32((w(i, j) / total) (n n / 4))           the density over the [-1, 1]^2
//                square the sampler is weighed with
// total = 0 or not finite: the table is empty.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

namespace spt {

constexpr uint32_t kSkyMaxN = 4096;  // kEnvMapMaxN

struct SkyTable {
    uint32_t n = 0;
    std::vector<float> marg;  // n
    std::vector<float> cond;  // n * n, row j at j * n
    std::vector<float> pdf;   // n * n
    bool empty() const { return marg.empty(); }
    void clear() { n = 0; marg.clear(); cond.clear(); pdf.clear(); }
};

// envmap_wrap (spt_internal.h), restated without HIP
inline void sky_wrap(int32_t n, int32_t& i, int32_t& j) {
    if (i < 0) { i = 0; j = n - 1 - j; }
    else if (i >= n) { i = n - 1; j = n - 1 - j; }
    if (j < 0) { j = 0; i = n - 1 - i; }
    else if (j >= n) { j = n - 1; i = n - 1 - i; }
}

// rgb: n * n * 3 floats, row-major (row j, column i), 1 <= n <= kSkyMaxN.
inline void sky_table_build(const float* rgb, uint32_t n, SkyTable& out) {
    out.clear();
    if (!rgb || n == 0 || n > kSkyMaxN) return;
    const int32_t ni = (int32_t)n;
    const size_t nn = (size_t)n * n;
    std::vector<float> Y(nn);
    for (size_t k = 0; k < nn; k++)
        Y[k] = std::fmax(std::fmax(std::fabs(rgb[3 * k]), std::fabs(rgb[3 * k + 1])), std::fabs(rgb[3 * k + 2]));
    static const double kk[3] = {0.125, 0.75, 0.125};
    std::vector<double> w(nn), row(n);
    double total = 0.0;
    for (int32_t j = 0; j < ni; j++) {
        double rs = 0.0;
        for (int32_t i = 0; i < ni; i++) {
            double yb = 0.0;
            for (int32_t dy = -1; dy <= 1; dy++)
                for (int32_t dx = -1; dx <= 1; dx++) {
                    int32_t si = i + dx, sj = j + dy;
                    sky_wrap(ni, si, sj);
                    yb += (kk[dx + 1] * kk[dy + 1]) * (double)Y[(size_t)sj * n + (size_t)si];
                }
            const double a = ((double)i + 0.5) / (double)n * 2.0 - 1.0, b = ((double)j + 0.5) / (double)n * 2.0 - 1.0;
            const double z = 1.0 - std::fabs(a) - std::fabs(b);
            const double x = z < 0.0 ? (1.0 - std::fabs(b)) * (a < 0.0 ? -1.0 : 1.0) : a;
            const double y = z < 0.0 ? (1.0 - std::fabs(a)) * (b < 0.0 ? -1.0 : 1.0) : b;
            const double l = std::sqrt((x * x + y * y) + z * z);
            double wi = yb / ((l * l) * l);
            if (!std::isfinite(wi) || !(wi > 0.0)) wi = 0.0;
            w[(size_t)j * n + (size_t)i] = wi;
            rs += wi;
        }
        row[j] = rs;
        total += rs;
    }
    if (!(total > 0.0) || !std::isfinite(total)) return;
    out.n = n;
    out.marg.resize(n);
    out.cond.resize(nn);
    out.pdf.resize(nn);
    const double cell = ((double)n * (double)n) / 4.0;
    double run = 0.0;
    for (uint32_t j = 0; j < n; j++) {
        run += row[j];
        out.marg[j] = (float)(run / total);
        double rr = 0.0;
        for (uint32_t i = 0; i < n; i++) {
            const size_t k = (size_t)j * n + i;
            rr += w[k];
            out.cond[k] = row[j] > 0.0 ? (float)(rr / row[j]) : 0.0f;
            out.pdf[k] = (float)((w[k] / total) * cell);
        }
        out.cond[(size_t)j * n + (n - 1)] = 1.0f;
    }
    out.marg[n - 1] = 1.0f;
}

}  // namespace spt
