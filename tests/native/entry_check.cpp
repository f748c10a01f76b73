// The contract of camera_entry.h, checked on the host: on trees of 64-B nodes
// from build_bvh8(.., 6) + to_node6 (node6.h) — the 200- and 5000-triangle
// soups of bvh_dump.cpp as generated, with every z equal and with a far
// outlier, and a tessellated ground quad with a box on it — and under seeded
// pinhole cameras at 16 x 16, 64 x 64 and 24 x 17 (sizes that are no power of
// two take camera_sample_dir's divide), every pixel's chain is walked as
// camera_entry_kernel walks it.  For 64 seeded xi per pixel and the four
// corners of [0, 1 - 2^-23]^2 the camera ray is computed in f32 with the camera
// functions of spt_math.h, and at every chain node the children a plain-C++
// restatement of Tracer8T::visit_words6 accepts (1.0f / d for the reciprocal;
// tbox = cull_tmin(kRayTmin), ht = kRayTmax) must be a subset of {the chain's
// child}.  One line per (tree, camera, size): pixels, pixels with an entry
// below the root, chain nodes checked, ray visits, violations, deepest chain.
// Host-only, its own main: built with the host C++ compiler together with
// bvh_build.cpp and bvh8_build.cpp, under the sanitizers.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bvh_build.h"
#include "camera_entry.h"
#include "node6.h"
#include "spt_math.h"

using namespace spt;

namespace {

struct Lcg {
    uint64_t s;
    float next() {  // [0, 1)
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((s >> 40) & 0xffffffu) / 16777216.0f;
    }
};

// bvh_dump.cpp's soup: variant 0 as generated, 1 every z equal, 2 a far outlier vertex
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
    return tv;
}

void quad(std::vector<float>& tv, const float* o, const float* u, const float* v, int nu, int nv) {
    for (int i = 0; i < nu; i++)
        for (int j = 0; j < nv; j++) {
            float p[4][3];
            for (int k = 0; k < 4; k++)
                for (int a = 0; a < 3; a++)
                    p[k][a] = o[a] + u[a] * (float)(i + (k == 1 || k == 2)) / (float)nu + v[a] * (float)(j + (k >= 2)) / (float)nv;
            const int idx[6] = {0, 1, 2, 0, 2, 3};
            for (int k : idx)
                for (int a = 0; a < 3; a++) tv.push_back(p[k][a]);
        }
}

// a 24 x 24 ground of 32 x 32 quads with a unit box (8 x 8 quads a face) on it
std::vector<float> ground_and_box() {
    std::vector<float> tv;
    const float go[3] = {-12, 0, -12}, gu[3] = {24, 0, 0}, gv[3] = {0, 0, 24};
    quad(tv, go, gu, gv, 32, 32);
    const float lo[3] = {-0.5f, 0.0f, -0.5f};
    for (int axis = 0; axis < 3; axis++)
        for (int side = 0; side < 2; side++) {
            float o[3] = {lo[0], lo[1], lo[2]}, u[3] = {0, 0, 0}, v[3] = {0, 0, 0};
            o[axis] += (float)side;
            u[(axis + 1) % 3] = 1.0f;
            v[(axis + 2) % 3] = 1.0f;
            quad(tv, o, u, v, 8, 8);
        }
    return tv;
}

// render.cpp make_camera
Camera make_camera(const float* from_, const float* at_, const float* up_, float fov_y, float focal_dist, uint32_t w,
                   uint32_t h) {
    Camera cam;
    const V3 from = v3(from_[0], from_[1], from_[2]), at = v3(at_[0], at_[1], at_[2]), up = v3(up_[0], up_[1], up_[2]);
    cam.origin = from;
    const V3 z = normalize(at - from);
    const V3 x = normalize(cross(up, z));
    const V3 y = normalize(cross(z, x));
    cam.frame.bx = x; cam.frame.by = y; cam.frame.bz = z;
    cam.lens_radius = 0.0f;
    cam.focal_dist = focal_dist;
    cam.film_y = 0.035f;
    cam.dist_lens_to_film = (cam.film_y * 0.5f) / std::tan(fov_y * 0.5f);
    cam.ratio = (float)w / (float)h;
    cam.fw = (float)w;
    cam.fh = (float)h;
    cam.inv_fw = (w & (w - 1u)) == 0u ? 1.0f / cam.fw : 0.0f;
    cam.inv_fh = (h & (h - 1u)) == 0u ? 1.0f / cam.fh : 0.0f;
    volatile float fz = cam.dist_lens_to_film;
    volatile float num = cam.focal_dist * fz;
    cam.focal_z = num / fz;
    return cam;
}

// kernels.hip camera_ray with the draws given: the lens draw, then the film draw
void camera_ray(const Camera& cam, uint32_t x, uint32_t y, const float* xi, V3& o, V3& d) {
    o = camera_sample_pos(cam, xi[0], xi[1]);
    d = camera_sample_dir(cam, x, y, o, xi[2], xi[3]);
}

// Tracer8T::init_slabs + visit_words6 restated: the children (bit c) whose meta
// byte contributes hit bits and whose slab test the ray passes at the root's
// tbox and ht.
uint32_t ray_visit6(const uint32_t* w, V3 o, V3 d) {
    const float dd[3] = {d.x, d.y, d.z}, oo[3] = {o.x, o.y, o.z};
    const uint32_t eb[3] = {(w[5] >> 16) & 0xffu, w[5] >> 24, w[6] >> 24};
    const float tbox = cull_tmin(kRayTmin), ht = kRayTmax;
    float ax[3], be[3], bx[3], ix[3];
    for (int a = 0; a < 3; a++) {
        const float dc = fabsf(dd[a]) < kSlabMinDir ? copysignf(kSlabMinDir, dd[a]) : dd[a];
        ix[a] = 1.0f / dc;
        ax[a] = u2f(eb[a] << 23) * ix[a];
        const float b = (u2f(w[a]) - oo[a]) * ix[a];
        const float m = fmaf(fabsf(ax[a]), 255.0f * kSlabMarginRel, fabsf(b) * kSlabMarginRel);
        be[a] = b - m;
        bx[a] = b + m;
    }
    uint32_t mask = 0;
    for (uint32_t c = 0; c < 6; c++) {
        if ((entry_meta6(w, c) >> 5) == 0u) continue;
        float te[3], tx[3];
        for (uint32_t a = 0; a < 3; a++) {
            uint32_t qlo, qhi;
            entry_planes6(w, c, a, qlo, qhi);
            const bool pos = ix[a] >= 0.0f;
            te[a] = fmaf((float)(pos ? qlo : qhi), ax[a], be[a]);
            tx[a] = fmaf((float)(pos ? qhi : qlo), ax[a], bx[a]);
        }
        const float tn = fmaxf(fmaxf(te[0], te[1]), fmaxf(te[2], tbox));
        const float tf = fminf(fminf(tx[0], tx[1]), fminf(tx[2], ht));
        if (tn <= tf) mask |= 1u << c;
    }
    return mask;
}

struct Tally {
    unsigned long long pixels = 0, below = 0, nodes = 0, visits = 0, bad = 0, deepest = 0;
};

void check(const std::vector<uint32_t>& n6, const Camera& cam, uint32_t W, uint32_t H, uint64_t seed, Tally& t) {
    const size_t nn = n6.size() / 16;
    constexpr int kRays = 68;
    std::vector<V3> ro(kRays), rd(kRays);
    for (uint32_t py = 0; py < H; py++)
        for (uint32_t px = 0; px < W; px++) {
            t.pixels++;
            EntryBeam b;
            if (!entry_beam(cam, px, py, b)) continue;
            Pcg32 rng;
            rng.seed(seed, (uint64_t)py * W + px);
            const float top = 1.0f - 1.0f / 8388608.0f;
            for (int r = 0; r < kRays; r++) {
                float xi[4];
                for (float& v : xi) v = rng.next_float();
                if (r >= 64) {  // the corners of the film draw
                    xi[2] = (r & 1) ? top : 0.0f;
                    xi[3] = (r & 2) ? top : 0.0f;
                }
                camera_ray(cam, px, py, xi, ro[r], rd[r]);
            }
            size_t node = 0;
            unsigned long long depth = 0;
            for (uint32_t step = 0; step < kEntryMaxDepth; step++) {
                const uint32_t* w = &n6[node * 16];
                uint32_t word, rank;
                if (!entry_descend6(w, b, word, rank)) break;
                const size_t child = (size_t)(word & 0x00ffffffu) + rank;  // the compact layout
                if (child == 0 || child >= nn) {
                    t.bad++;  // the chain left the tree
                    break;
                }
                // the chain's child: the one whose meta byte names the word's slot
                uint32_t cc = 6;
                for (uint32_t c = 0; c < 6; c++) {
                    const uint32_t m = entry_meta6(w, c);
                    if ((m >> 5) != 0u && (m & 0x18u) == 0x18u && (m & 7u) == (word >> 24)) cc = c;
                }
                if (cc == 6) {
                    t.bad++;
                    break;
                }
                t.nodes++;
                for (int r = 0; r < kRays; r++) {
                    t.visits++;
                    if (ray_visit6(w, ro[r], rd[r]) & ~(1u << cc)) t.bad++;
                }
                node = child;
                depth++;
            }
            if (depth) t.below++;
            if (depth > t.deepest) t.deepest = depth;
        }
}

}  // namespace

int main() {
    struct Scene {
        std::string name;
        std::vector<float> tv;
    };
    std::vector<Scene> scenes;
    const char* vname[3] = {"plain", "flat_z", "outlier"};
    for (uint64_t n : {200ull, 5000ull})
        for (int variant = 0; variant < 3; variant++) {
            char nm[32];
            std::snprintf(nm, sizeof(nm), "soup%llu_%s", (unsigned long long)n, vname[variant]);
            scenes.push_back(Scene{nm, soup(n, 1234 + n, variant)});
        }
    scenes.push_back(Scene{"ground_box", ground_and_box()});
    const uint32_t sizes[3][2] = {{16, 16}, {64, 64}, {24, 17}};
    bool ok = true;
    for (const Scene& s : scenes) {
        const Bvh8BuildResult b = build_bvh8(s.tv.data(), s.tv.size() / 9, false, 6);
        bool over = false;
        const std::vector<uint32_t> n6 = to_node6(b.nodes, &over);
        if (over) {
            std::fprintf(stderr, "%s: a width-6 tree has a node with more than six children\n", s.name.c_str());
            return 1;
        }
        Lcg r{77};
        for (int cam_i = 0; cam_i < 4; cam_i++) {
            // camera 0 looks down at the ground from near the box; the rest are seeded around the scene
            float from[3] = {3.0f, 2.5f, 5.0f}, at[3] = {0.0f, 0.5f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f};
            float fov = 0.6911f, focal = 5.0f;
            if (cam_i > 0) {
                for (int a = 0; a < 3; a++) from[a] = (r.next() - 0.5f) * 24.0f;
                from[1] = r.next() * 8.0f + 0.1f;
                for (int a = 0; a < 3; a++) at[a] = (r.next() - 0.5f) * 4.0f;
                fov = 0.3f + r.next() * 1.2f;
                focal = 0.5f + r.next() * 20.0f;
                if (cam_i == 3) { up[0] = 0.3f; up[2] = -0.2f; }
            }
            for (const auto& sz : sizes) {
                const Camera cam = make_camera(from, at, up, fov, focal, sz[0], sz[1]);
                Tally t;
                check(n6, cam, sz[0], sz[1], 99 + cam_i, t);
                std::printf("%s cam%d %ux%u pixels %llu below %llu nodes %llu visits %llu bad %llu deepest %llu\n", s.name.c_str(),
                            cam_i, sz[0], sz[1], t.pixels, t.below, t.nodes, t.visits, t.bad, t.deepest);
                ok = ok && t.bad == 0;
            }
        }
    }
    // a thin lens, and frames and origins that are not finite, have no beam
    {
        const float from[3] = {3, 2.5f, 5}, at[3] = {0, 0.5f, 0}, up[3] = {0, 1, 0};
        Camera c = make_camera(from, at, up, 0.69f, 5.0f, 16, 16);
        EntryBeam b;
        int none = 0;
        Camera t = c; t.lens_radius = 0.01f; none += !entry_beam(t, 3, 4, b);
        t = c; t.frame.by.x = NAN; none += !entry_beam(t, 3, 4, b);
        t = c; t.origin.z = INFINITY; none += !entry_beam(t, 3, 4, b);
        t = c; t.focal_z = 0.0f; none += !entry_beam(t, 3, 4, b);
        t = c; t.dist_lens_to_film = NAN; none += !entry_beam(t, 3, 4, b);
        const int some = entry_beam(c, 3, 4, b) ? 1 : 0;
        std::printf("no_beam %d of 5, beam %d\n", none, some);
        ok = ok && none == 5 && some == 1;
    }
    return ok ? 0 : 1;
}
