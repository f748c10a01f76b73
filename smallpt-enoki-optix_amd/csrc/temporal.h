// temporal.h — spt_temporal_accumulate's per-pixel arithmetic: the temporal
// accumulation of Schied et al. 2017 ("Spatiotemporal Variance-Guided
// Filtering"), whose spatial half is spt_denoise_var (denoise.hip).  The last
// frame's running mean, second moment and history length are reprojected
// through the current first-hit depth into the previous view, gathered with
// the bilinear taps whose surface agrees, and blended with the current frame's
// samples.  Compiled by hipcc for gfx950 (temporal.hip) and by the host
// compiler (tests/native/temporal_check.cpp): one text, the steps of
// include/spt.h in their order, every operation f32 and rounded once
// (-ffp-contract=off, correctly rounded divide and sqrt, nothing transcendental).
#pragma once
#include <math.h>

#include "spt_math.h"

namespace spt_temporal {

using spt::Camera;
using spt::V3;

// Planes are width x height floats, SoA; the 3-plane images are channel-major.
struct TemporalArgs {
    Camera cam, prev_cam;
    uint32_t width, height;
    float samples, max_history, sigma_depth, normal_min;
    uint32_t has_prev;    // 0: first frame, no plane of prev_* is read
    uint32_t depth_test;  // sigma_depth > 0
    uint32_t normal_test; // normal_min > -1 and both sides carry their three normal planes
    const float *sum, *sum_sq;                                           // 3 planes each
    const float *depth, *coverage, *normal_x, *normal_y, *normal_z;      // the current frame's guides
    const float *prev_color, *prev_moment2, *prev_length;                // 3, 3, 1 planes
    const float *prev_depth, *prev_coverage, *prev_normal_x, *prev_normal_y, *prev_normal_z;
    float *out_color, *out_moment2, *out_length;                         // 3, 3, 1 planes
    float *film, *variance;                                              // 3 planes each, may be null
};

struct TemporalPixel {
    float color[3], moment2[3], length, variance[3];
    uint32_t taps;    // valid taps gathered (0: no history)
    uint32_t snapped; // bit 0: x snapped to a pixel centre, bit 1: y
};

// Step 5: a coordinate within 1/64 of a pixel centre is that centre, so a
// camera that did not move reads exactly its own pixel.
SPT_HD float snap(float s, uint32_t& hit) {
    const float r = rintf(s);
    hit = fabsf(s - r) <= 0.015625f ? 1u : 0u;
    return hit ? r : s;
}

// Pixel (x, y) of the new history; writes nothing.
SPT_HD TemporalPixel temporal_pixel(const TemporalArgs& a, uint32_t x, uint32_t y) {
    const size_t P = (size_t)a.width * a.height;
    const size_t i = (size_t)y * a.width + x;
    TemporalPixel r;
    r.taps = 0;
    r.snapped = 0;
    float sw = 0.0f, hl = 0.0f, hc[3] = {0.0f, 0.0f, 0.0f}, hm[3] = {0.0f, 0.0f, 0.0f};
    if (a.has_prev) {
        // 1-3: the pixel's class, centre ray and world point
        const float cov = a.coverage[i];
        const bool surface = cov > 0.0f;
        const V3 d = spt::camera_sample_dir(a.cam, x, y, a.cam.origin, 0.5f, 0.5f);
        V3 v = d;
        float zexp = 0.0f;
        if (surface) {
            const float z = a.depth[i] / cov;
            const V3 X = {a.cam.origin.x + z * d.x, a.cam.origin.y + z * d.y, a.cam.origin.z + z * d.z};
            v = X - a.prev_cam.origin;
            zexp = sqrtf(spt::dot(v, v));
        }
        // 4: into the previous view
        const V3 l = spt::to_local(a.prev_cam.frame, v);
        const float fx = (l.x * a.prev_cam.dist_lens_to_film) / l.z;
        const float fy = (l.y * a.prev_cam.dist_lens_to_film) / l.z;
        const float ndx = 0.5f - fx / (a.prev_cam.ratio * a.prev_cam.film_y);
        const float ndy = 0.5f - fy / a.prev_cam.film_y;
        const float fw = (float)a.width, fh = (float)a.height;
        float sx = ndx * fw - 0.5f, sy = ndy * fh - 0.5f;
        const bool inside = l.z > 0.0f && fabsf(sx) < INFINITY && fabsf(sy) < INFINITY && sx > -1.0f && sx < fw &&
                            sy > -1.0f && sy < fh;
        if (inside) {
            // 5-6: snap, bilinear taps
            uint32_t hx, hy;
            sx = snap(sx, hx);
            sy = snap(sy, hy);
            r.snapped = hx | (hy << 1);
            const float x0f = floorf(sx), y0f = floorf(sy);
            const float tx = sx - x0f, ty = sy - y0f;
            const int32_t x0 = (int32_t)x0f, y0 = (int32_t)y0f;  // in [-1, width] x [-1, height]
            const float w4[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
            float nx = 0.0f, ny = 0.0f, nz = 0.0f;
            if (surface && a.normal_test) {
                nx = a.normal_x[i] / cov;
                ny = a.normal_y[i] / cov;
                nz = a.normal_z[i] / cov;
            }
            for (int k = 0; k < 4; k++) {
                const int32_t qx = x0 + (k & 1), qy = y0 + (k >> 1);
                const float w = w4[k];
                if (w == 0.0f || qx < 0 || qy < 0 || qx >= (int32_t)a.width || qy >= (int32_t)a.height) continue;
                const size_t j = (size_t)qy * a.width + (size_t)qx;
                // 7: the tap's history exists and saw the same surface (or the sky)
                const float len = a.prev_length[j];
                if (!(len > 0.0f)) continue;
                const float cq = a.prev_coverage[j];
                if (surface) {
                    if (!(cq > 0.0f)) continue;
                    if (a.depth_test) {
                        const float zq = a.prev_depth[j] / cq;
                        if (!(fabsf(zq - zexp) <= a.sigma_depth * zexp)) continue;
                    }
                    if (a.normal_test) {
                        const V3 nq = {a.prev_normal_x[j] / cq, a.prev_normal_y[j] / cq, a.prev_normal_z[j] / cq};
                        if (!(spt::dot(spt::v3(nx, ny, nz), nq) >= a.normal_min)) continue;
                    }
                } else if (!(cq <= 0.0f)) {
                    continue;
                }
                // 8: gather
                sw = sw + w;
                hl = hl + w * len;
                for (int c = 0; c < 3; c++) {
                    hc[c] = hc[c] + w * a.prev_color[c * P + j];
                    hm[c] = hm[c] + w * a.prev_moment2[c * P + j];
                }
                r.taps++;
            }
        }
    }
    // 8-10: the history's means, its length capped, and the blend
    float Nh = 0.0f;
    if (sw > 0.0f) {
        hl = hl / sw;
        for (int c = 0; c < 3; c++) {
            hc[c] = hc[c] / sw;
            hm[c] = hm[c] / sw;
        }
        Nh = fminf(hl, a.max_history);
    }
    const float n = a.samples;
    const bool blend = Nh > 0.0f;
    const float N = blend ? Nh + n : n;
    const float alpha = n / N;
    for (int c = 0; c < 3; c++) {
        const float m = a.sum[c * P + i] / n, q = a.sum_sq[c * P + i] / n;
        r.color[c] = blend ? hc[c] + alpha * (m - hc[c]) : m;
        r.moment2[c] = blend ? hm[c] + alpha * (q - hm[c]) : q;
        // 11: spt_render_accum's variance of the mean with N for n
        r.variance[c] = N < 2.0f ? 0.0f : fmaxf(r.moment2[c] - r.color[c] * r.color[c], 0.0f) / (N - 1.0f);
    }
    r.length = N;
    return r;
}

// Stores the pixel into the planes of `a` that are not null.
SPT_HD void temporal_store(const TemporalArgs& a, uint32_t x, uint32_t y, const TemporalPixel& r) {
    const size_t P = (size_t)a.width * a.height;
    const size_t i = (size_t)y * a.width + x;
    for (int c = 0; c < 3; c++) {
        a.out_color[c * P + i] = r.color[c];
        a.out_moment2[c * P + i] = r.moment2[c];
        if (a.film) a.film[c * P + i] = r.color[c];
        if (a.variance) a.variance[c * P + i] = r.variance[c];
    }
    a.out_length[i] = r.length;
}

}  // namespace spt_temporal
