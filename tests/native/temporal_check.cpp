// The per-pixel arithmetic of spt_temporal_accumulate (csrc/temporal.h), compiled
// for the host and held against a float64 restatement of include/spt.h's steps
// on a grid of pixels and depths.  Host-only, its own main; built with the host
// C++ compiler, optionally under the sanitizers (every tap index is then checked
// against the planes' bounds).
//
// Scenes: every pixel of a W x H image sees a surface at one depth z (coverage
// 3/4, depth premultiplied), for z = 0.05 .. 500; the previous frame's colour
// and second moment are ramps in pixel coordinates (so the bilinear gather is a
// smooth function of the reprojected position), its length is 9 with every 7th
// pixel 0, and its depth plane is the distance the current point has from the
// previous camera, in f64, rounded: the depth test passes except where
// rounding decides.  Cameras: the same view twice (every pixel must snap onto
// itself and take exactly its own history), a translated and turned view, and a
// view turned by more than 90 degrees (no history anywhere).
//
// One line per case:  name WxH z pixels P exact E flips F maxerr M
//   exact   pixels whose colour, moment and length equal the f64 result rounded
//   flips   pixels where f32 and f64 disagree on a decision (snap, tap validity)
//   maxerr  largest |f32 - f64| of the colour over the pixels without a flip
// and "temporal_check ok" when every case holds its bound.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "camera_make.h"
#include "temporal.h"

using namespace spt;
using namespace spt_temporal;

namespace {

struct D3 { double x, y, z; };
D3 d3(V3 v) { return {v.x, v.y, v.z}; }
double ddot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D3 dlocal(const Frame& f, D3 w) { return {ddot(d3(f.bx), w), ddot(d3(f.by), w), ddot(d3(f.bz), w)}; }
D3 dworld(const Frame& f, D3 l) {
    return {f.bx.x * l.x + f.by.x * l.y + f.bz.x * l.z, f.bx.y * l.x + f.by.y * l.y + f.bz.y * l.z,
            f.bx.z * l.x + f.by.z * l.y + f.bz.z * l.z};
}

// the pinhole centre ray of pixel (x, y) in f64, from the camera's f32 constants
D3 centre_dir(const Camera& c, uint32_t x, uint32_t y) {
    const double fx = (0.5 - (x + 0.5) / (double)c.fw) * ((double)c.ratio * (double)c.film_y);
    const double fy = (0.5 - (y + 0.5) / (double)c.fh) * (double)c.film_y;
    D3 f = {c.focal_dist * fx / c.dist_lens_to_film, c.focal_dist * fy / c.dist_lens_to_film, c.focal_z};
    const double inv = 1.0 / std::sqrt(ddot(f, f));
    return dworld(c.frame, {f.x * inv, f.y * inv, f.z * inv});
}

struct Ref {
    double color[3], moment2[3], length;
    uint32_t taps, snapped;
};

// include/spt.h's steps 1-10 in f64 (surface pixels with the depth test; no normals)
Ref reference(const TemporalArgs& a, uint32_t x, uint32_t y) {
    const size_t P = (size_t)a.width * a.height, i = (size_t)y * a.width + x;
    Ref r{};
    double sw = 0, hl = 0, hc[3] = {0, 0, 0}, hm[3] = {0, 0, 0};
    if (a.has_prev) {
        const double cov = a.coverage[i];
        const D3 d = centre_dir(a.cam, x, y);
        const double z = a.depth[i] / cov;
        const D3 X = {a.cam.origin.x + z * d.x, a.cam.origin.y + z * d.y, a.cam.origin.z + z * d.z};
        const D3 v = {X.x - a.prev_cam.origin.x, X.y - a.prev_cam.origin.y, X.z - a.prev_cam.origin.z};
        const double zexp = std::sqrt(ddot(v, v));
        const D3 l = dlocal(a.prev_cam.frame, v);
        const double fx = l.x * a.prev_cam.dist_lens_to_film / l.z, fy = l.y * a.prev_cam.dist_lens_to_film / l.z;
        double sx = (0.5 - fx / ((double)a.prev_cam.ratio * a.prev_cam.film_y)) * a.width - 0.5;
        double sy = (0.5 - fy / (double)a.prev_cam.film_y) * a.height - 0.5;
        if (l.z > 0 && std::isfinite(sx) && std::isfinite(sy) && sx > -1 && sx < a.width && sy > -1 && sy < a.height) {
            const double rx = std::nearbyint(sx), ry = std::nearbyint(sy);
            if (std::fabs(sx - rx) <= 1.0 / 64) { sx = rx; r.snapped |= 1u; }
            if (std::fabs(sy - ry) <= 1.0 / 64) { sy = ry; r.snapped |= 2u; }
            const double x0 = std::floor(sx), y0 = std::floor(sy), tx = sx - x0, ty = sy - y0;
            const double w4[4] = {(1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty};
            for (int k = 0; k < 4; k++) {
                const long qx = (long)x0 + (k & 1), qy = (long)y0 + (k >> 1);
                if (w4[k] == 0 || qx < 0 || qy < 0 || qx >= (long)a.width || qy >= (long)a.height) continue;
                const size_t j = (size_t)qy * a.width + (size_t)qx;
                if (!(a.prev_length[j] > 0) || !(a.prev_coverage[j] > 0)) continue;
                const double zq = (double)a.prev_depth[j] / a.prev_coverage[j];
                if (a.depth_test && !(std::fabs(zq - zexp) <= (double)a.sigma_depth * zexp)) continue;
                sw += w4[k];
                hl += w4[k] * a.prev_length[j];
                for (int c = 0; c < 3; c++) {
                    hc[c] += w4[k] * a.prev_color[c * P + j];
                    hm[c] += w4[k] * a.prev_moment2[c * P + j];
                }
                r.taps++;
            }
        }
    }
    const double n = a.samples;
    double Nh = 0;
    if (sw > 0) Nh = std::fmin(hl / sw, (double)a.max_history);
    const double N = Nh > 0 ? Nh + n : n;
    for (int c = 0; c < 3; c++) {
        const double m = a.sum[c * P + i] / n, q = a.sum_sq[c * P + i] / n;
        r.color[c] = Nh > 0 ? hc[c] / sw + n / N * (m - hc[c] / sw) : m;
        r.moment2[c] = Nh > 0 ? hm[c] / sw + n / N * (q - hm[c] / sw) : q;
    }
    r.length = N;
    return r;
}

spt_camera view(float fx, float fy, float fz, float ax, float ay, float az, float lens) {
    spt_camera c{};
    c.look_from[0] = fx; c.look_from[1] = fy; c.look_from[2] = fz;
    c.look_at[0] = ax; c.look_at[1] = ay; c.look_at[2] = az;
    c.up[1] = 1.0f;
    c.lens_radius = lens;
    c.focal_dist = 1.0f;
    c.fov_y = 0.6981317f;
    c.film_size_y = 0.035f;
    return c;
}

struct Case {
    const char* name;
    spt_camera cur, prev;
    int kind;  // 0: the same view, 1: moved, 2: turned away
};

bool run(const Case& cs, uint32_t W, uint32_t H, float z) {
    const size_t P = (size_t)W * H;
    TemporalArgs a{};
    a.cam = make_camera(cs.cur, W, H);
    a.prev_cam = make_camera(cs.prev, W, H);
    a.width = W; a.height = H;
    a.samples = 4.0f; a.max_history = 64.0f; a.sigma_depth = 0.1f; a.normal_min = 0.9f;
    a.has_prev = 1; a.depth_test = 1; a.normal_test = 0;
    std::vector<float> sum(3 * P), sum_sq(3 * P), depth(P), cov(P, 0.75f), pcol(3 * P), pmom(3 * P), plen(P), pdep(P),
        pcov(P, 0.5f), ocol(3 * P), omom(3 * P), olen(P), film(3 * P), var(3 * P);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            depth[i] = z * 0.75f;
            plen[i] = i % 7 == 3 ? 0.0f : 9.0f;
            for (int c = 0; c < 3; c++) {
                sum[c * P + i] = 4.0f * (0.25f + 0.125f * c);
                sum_sq[c * P + i] = 4.0f * (0.5f + 0.125f * c);
                pcol[c * P + i] = 0.5f + 0.001f * x + 0.002f * y + 0.1f * c;
                pmom[c * P + i] = 1.5f + 0.002f * x + 0.001f * y;
            }
        }
    a.sum = sum.data(); a.sum_sq = sum_sq.data();
    a.depth = depth.data(); a.coverage = cov.data();
    a.prev_color = pcol.data(); a.prev_moment2 = pmom.data(); a.prev_length = plen.data();
    a.prev_depth = pdep.data(); a.prev_coverage = pcov.data();
    a.out_color = ocol.data(); a.out_moment2 = omom.data(); a.out_length = olen.data();
    a.film = film.data(); a.variance = var.data();
    // the previous frame's depth: what the previous camera measures to the point each previous pixel sees,
    // which for this one-depth scene is z along the previous pixel's own ray when the views agree, and
    // close enough to pass the 10 % test otherwise; stored premultiplied by its coverage
    for (size_t i = 0; i < P; i++) pdep[i] = z * 0.5f;
    if (cs.kind == 1) {
        // moved view: each previous pixel sees the current shell of points at about |X - C'.origin|; take
        // the exact value for the pixel the current pixel lands on (nearest), elsewhere z
        for (uint32_t y = 0; y < H; y++)
            for (uint32_t x = 0; x < W; x++) {
                const D3 d = centre_dir(a.cam, x, y);
                const D3 X = {a.cam.origin.x + z * d.x, a.cam.origin.y + z * d.y, a.cam.origin.z + z * d.z};
                const D3 v = {X.x - a.prev_cam.origin.x, X.y - a.prev_cam.origin.y, X.z - a.prev_cam.origin.z};
                const D3 l = dlocal(a.prev_cam.frame, v);
                if (!(l.z > 0)) continue;
                const double sx = (0.5 - l.x * a.prev_cam.dist_lens_to_film / l.z / ((double)a.prev_cam.ratio * a.prev_cam.film_y)) * W - 0.5;
                const double sy = (0.5 - l.y * a.prev_cam.dist_lens_to_film / l.z / (double)a.prev_cam.film_y) * H - 0.5;
                const long qx = std::lround(sx), qy = std::lround(sy);
                if (qx < 0 || qy < 0 || qx >= (long)W || qy >= (long)H) continue;
                pdep[(size_t)qy * W + qx] = (float)(std::sqrt(ddot(v, v)) * 0.5);
            }
    }
    size_t exact = 0, flips = 0, history = 0;
    double maxerr = 0;
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const TemporalPixel r = temporal_pixel(a, x, y);
            temporal_store(a, x, y, r);
            const Ref f = reference(a, x, y);
            history += r.taps > 0;
            if (r.taps != f.taps || r.snapped != f.snapped) { flips++; continue; }
            bool same = r.length == (float)f.length;
            for (int c = 0; c < 3; c++) {
                same = same && r.color[c] == (float)f.color[c] && r.moment2[c] == (float)f.moment2[c];
                maxerr = std::fmax(maxerr, std::fabs((double)r.color[c] - f.color[c]));
                maxerr = std::fmax(maxerr, std::fabs((double)r.moment2[c] - f.moment2[c]));
            }
            exact += same;
            if (cs.kind == 0 && (r.snapped != 3u || r.taps != (plen[(size_t)y * W + x] > 0.0f ? 1u : 0u))) {
                std::printf("FAIL %s %ux%u z %g: pixel (%u, %u) does not read exactly itself\n", cs.name, W, H, z, x, y);
                return false;
            }
        }
    std::printf("%s %ux%u z %g pixels %zu history %zu exact %zu flips %zu maxerr %.3g\n", cs.name, W, H, (double)z, P,
                history, exact, flips, maxerr);
    // f32 against f64: the ramps' slopes (2e-3 per pixel) times the reprojection's position error (below
    // 2e-3 pixel, include/spt.h step 5) plus a few roundings of values below 4
    bool ok = maxerr <= 1e-5 && flips * 50 <= P;
    if (cs.kind == 0) ok = ok && flips == 0 && history == P - (P + 3) / 7;
    if (cs.kind == 2) ok = ok && history == 0;
    if (cs.kind == 1 && z >= 1.0f && W >= 64) ok = ok && history * 2 > P;  // the move is a few pixels of a wide image
    if (!ok) std::printf("FAIL %s %ux%u z %g\n", cs.name, W, H, (double)z);
    return ok;
}

}  // namespace

int main() {
    const Case cases[] = {
        {"same", view(0.0f, 3.03f, 5.0f, 0.0f, 0.03f, 0.0f, 0.0f), view(0.0f, 3.03f, 5.0f, 0.0f, 0.03f, 0.0f, 0.0f), 0},
        {"same_lens", view(0.3f, 1.0f, 4.0f, 0.1f, 0.5f, 0.0f, 0.05f), view(0.3f, 1.0f, 4.0f, 0.1f, 0.5f, 0.0f, 0.0f), 0},
        {"moved", view(0.4f, 3.1f, 4.9f, 0.1f, 0.03f, 0.0f, 0.0f), view(0.0f, 3.03f, 5.0f, 0.0f, 0.03f, 0.0f, 0.0f), 1},
        {"away", view(0.0f, 3.03f, 5.0f, 0.0f, 0.03f, 10.0f, 0.0f), view(0.0f, 3.03f, 5.0f, 0.0f, 0.03f, 0.0f, 0.0f), 2},
    };
    const uint32_t sizes[][2] = {{70, 50}, {64, 48}, {1, 1}, {3, 70}, {480, 270}};
    const float depths[] = {0.05f, 0.7f, 5.0f, 37.0f, 500.0f};
    bool ok = true;
    for (const Case& cs : cases)
        for (const auto& s : sizes)
            for (float z : depths) ok = run(cs, s[0], s[1], z) && ok;
    std::printf(ok ? "temporal_check ok\n" : "temporal_check FAILED\n");
    return ok ? 0 : 1;
}
