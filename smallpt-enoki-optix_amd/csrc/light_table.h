// light_table.h — the light table of a scene with light sampling on
// (spt_scene_set_light_sampling), built on the host in f64.
// Plain C++, no HIP: capi.cpp builds the scene's table with it,
// spt_light_table_build exposes it, and tests/native/light_check.cpp runs it
// under the sanitizers on hostile triangle soups.
//
// Members: the triangles whose material has non-zero emission (mat < nemit,
// some channel != 0), in original triangle id order, so the table does not
// depend on the builder, the tree width or the slot order.
//   area_i = 1/2 |(v1 - v0) x (v2 - v0)|      from the f32 vertices, in f64
//   w_i    = area_i max(Le_r, Le_g, Le_b)     a non-finite or zero (or negative)
//                                             weight becomes 0: the triangle
//                                             stays in the table, never chosen
//   cdf_i  = f32(sum_{j <= i} w_j / sum w)    summed sequentially; the last is 1
//   pdfA_i = f32(w_i / (sum w area_i))        0 where w_i = 0
// sum w = 0, or no member: the table is empty.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

namespace spt {

// One light on the device: 64 B, four quads.
//   q0 = (v0, v1.x)  q1 = (v1.yz, v2.xy)  q2 = (v2.z, n)  q3 = (Le, pdfA)
// n: the unit geometric normal (v1 - v0) x (v2 - v0) / |.|, rounded from f64
// (0 for a triangle without one).
constexpr uint32_t kLightFloats = 16;
constexpr uint32_t kMaxLights = 1u << 24;  // the binary search and the table's size in 32 bits

struct LightTable {
    std::vector<uint32_t> ids;   // original triangle ids, ascending
    std::vector<float> cdf, pdfA;
    std::vector<float> rec;      // kLightFloats per light
    bool empty() const { return ids.empty(); }
    void clear() { ids.clear(); cdf.clear(); pdfA.clear(); rec.clear(); }
};

// tv: 9 floats per triangle (v0 v1 v2); mat: a material id per triangle, or
// null (material 0); emission: 3 floats per material, or null.
inline void light_table_build(const float* tv, const int32_t* mat, uint64_t ntri, const float* emission,
                              uint32_t nemit, LightTable& out) {
    out.clear();
    if (!emission || nemit == 0 || ntri == 0) return;
    std::vector<double> w, area;
    for (uint64_t t = 0; t < ntri; t++) {
        const int64_t m = mat ? mat[t] : 0;
        if (m < 0 || m >= (int64_t)nemit) continue;
        const float* e = emission + (size_t)m * 3;
        if (e[0] == 0.0f && e[1] == 0.0f && e[2] == 0.0f) continue;
        const float* v = tv + (size_t)t * 9;
        const double ax = (double)v[3] - v[0], ay = (double)v[4] - v[1], az = (double)v[5] - v[2];
        const double bx = (double)v[6] - v[0], by = (double)v[7] - v[1], bz = (double)v[8] - v[2];
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        const double len = std::sqrt(cx * cx + cy * cy + cz * cz);
        const double a = 0.5 * len;
        double wi = a * (double)std::fmax(e[0], std::fmax(e[1], e[2]));
        if (!std::isfinite(wi) || !(wi > 0.0)) wi = 0.0;
        out.ids.push_back((uint32_t)t);
        w.push_back(wi);
        area.push_back(a);
        const bool unit = std::isfinite(len) && len > 0.0;
        const float n[3] = {unit ? (float)(cx / len) : 0.0f, unit ? (float)(cy / len) : 0.0f,
                            unit ? (float)(cz / len) : 0.0f};
        const float r[kLightFloats] = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], n[0], n[1], n[2],
                                       e[0], e[1], e[2], 0.0f};
        out.rec.insert(out.rec.end(), r, r + kLightFloats);
    }
    double total = 0.0;
    for (double x : w) total += x;
    if (!(total > 0.0) || !std::isfinite(total)) {
        out.clear();
        return;
    }
    const size_t n = out.ids.size();
    out.cdf.resize(n);
    out.pdfA.resize(n);
    double run = 0.0;
    for (size_t i = 0; i < n; i++) {
        run += w[i];
        out.cdf[i] = (float)(run / total);
        out.pdfA[i] = w[i] > 0.0 ? (float)(w[i] / (total * area[i])) : 0.0f;
        out.rec[i * kLightFloats + 15] = out.pdfA[i];
    }
    out.cdf[n - 1] = 1.0f;
}

}  // namespace spt
