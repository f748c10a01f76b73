// camera_entry.h — the BVH entry node of a pixel's camera rays (DESIGN.md §4,
// "Camera entry").  Every ray a pinhole camera makes for pixel (px, py) lies in
// that pixel's pyramid, its beam.  Where the beam can touch only one child of
// a node, and that child is an inner node, every ray of the pixel goes through
// that child and no other: the visits down that chain decide nothing, and the
// camera cast starts the pixel's rays at the chain's end (Tracer8T::init_slabs'
// entry word) instead of at the root.  64-B six-wide nodes only (bvh_build.h).
//
// __host__ __device__, f64: camera_entry_kernel (kernels.hip) runs it one lane
// per tile pixel, tests/native/entry_check.cpp on the host.
//
// The contract.  At every node on the chain, for every camera ray the cast can
// make for the pixel — any xi in [0,1)^2, as camera_ray computes it in f32 —
// the children the ray's own visit accepts (Tracer8T::visit_words6 with tbox =
// box_tmin(kRayTmin), ht = kRayTmax) are a subset of {the chain's child}.
// Starting at the chain's end is then culling the chain's siblings, which no
// such ray would have entered: same triangles tested, same hit.
//
// The beam (entry_beam).  A pinhole ray starts at the camera origin exactly
// (camera_sample_pos: the lens offset is 0 * r) and its direction is
// d = M normalize(F(xi)), F affine in xi over the pixel's rectangle of the
// focal plane z = Fz, M the camera frame.  For F = sum l_i F_i (corners F_i,
// l convex), d = S sum m_i d_i with m convex and S = sum l_i |F_i| / |F|, the
// Jensen gap of |.|, whose Hessian on the plane is at most 1 / |Fz|:
//   1 <= S <= 1 + D^2 / (2 Fz^2),   D the rectangle's diagonal,
// so each component of d lies within D^2 / (2 Fz^2) of the corners' interval
// (the curvature of d / |d| over one pixel, second order in its angle).  The
// f32 rounding of camera_sample_dir adds: (px + xi) / fw and the subtraction
// from 0.5 at most 3.5 * 2^-24 absolute, the three products and the divide to
// F.x at most 3 * 2^-24 relative — under 8 * 2^-24 K with K the focal plane's
// width (height for F.y); normalize at most 4 * 2^-24 per component of a unit
// vector; both through M (row sums <= sqrt 3) and to_world's own five
// roundings of terms <= 1, 6 * 2^-24:
//   slack = D^2 / (2 Fz^2) + 2^-24 (16 + 14 |K| / |Fz|),  |K| = |(Kx, Ky)|.
// The corners are evaluated in f64 from the camera's f32 constants in the
// device's operation order.  A camera whose intermediate values could leave
// f32's normal range has no beam (word 0 everywhere), nor has a thin lens or a
// frame that is not finite.  (xi = (1/2, 1/2) in the lens draw makes the
// reference's disk mapping 0 / 0 and the origin NaN: that ray, one in 2^46,
// fails every triangle test wherever it starts.)
//
// An axis whose interval contains 0 or reaches inside +-kSlabMinDir (where
// init_slabs clamps) constrains nothing.  Otherwise the sign is fixed and the
// ray's reciprocal (v_rcp_f32, 1 ulp) lies in [1 / hi, 1 / lo] widened by
// 2^-22 relative.
//
// The visit (entry_visit6).  The ray's slab value t = q (2^e ix) + (p - o) ix
// -+ m, m = kSlabMarginRel (255 |2^e ix| + |(p - o) ix|), carries five f32
// roundings of quantities bounded by 255 |2^e ix| + 3 |(p - o) ix|, together
// under 0.2 m: it sits within m of the exact value at the ray's ix and then
// moves by m itself, so the beam uses 2 m (plus 1e-30 absolute for results in
// the subnormal range).  For a fixed sign of ix that bound is linear in ix:
// its extremes over the interval are at the end points.  A child is accepted
// when the largest least entry over the constrained axes is at most the
// smallest greatest exit and that exit is >= 0 (the ray's tbox is positive;
// its tmax is ignored).  An axis whose f32 products could overflow (the ray's
// visit then drops it: fmaxf / fminf skip the NaN) constrains nothing.
#pragma once
#include <stdint.h>

#include "spt_math.h"

namespace spt {

constexpr float kSlabMarginRel = 1e-6f;  // kernels.hip kMarginRel
constexpr float kSlabMinDir = 1e-20f;    // kernels.hip kMinDir
constexpr uint32_t kEntryMaxDepth = 64;  // the descent's bound (a sound tree is far shallower)

struct EntryBeam {
    double o[3];          // the rays' origin
    double i0[3], i1[3];  // the reciprocal direction's interval, i0 <= i1 of one sign
    bool con[3];          // the axis constrains (else i0, i1 are not set)
};

SPT_HD bool entry_finite(double x) { return x - x == 0.0; }

// The unit direction of pixel (px, py) at xi = (cx, cy), cx, cy in {0, 1}, and
// the focal point F it came from (camera_sample_dir with a zero lens offset).
SPT_HD void entry_corner(const Camera& c, uint32_t px, uint32_t py, uint32_t cx, uint32_t cy, double* d, double* F) {
    const double ndc_x = ((double)(float)px + (double)cx) / (double)c.fw;
    const double ndc_y = ((double)(float)py + (double)cy) / (double)c.fh;
    const float kx = c.ratio * c.film_y;  // the device's f32 constant
    const double fx = (0.5 - ndc_x) * (double)kx;
    const double fy = (0.5 - ndc_y) * (double)c.film_y;
    const double fz = (double)c.dist_lens_to_film;
    F[0] = ((double)c.focal_dist * fx) / fz;
    F[1] = ((double)c.focal_dist * fy) / fz;
    F[2] = (double)c.focal_z;
    const double inv = 1.0 / sqrt((F[0] * F[0] + F[1] * F[1]) + F[2] * F[2]);
    const double ux = F[0] * inv, uy = F[1] * inv, uz = F[2] * inv;
    d[0] = ((double)c.frame.bx.x * ux + (double)c.frame.by.x * uy) + (double)c.frame.bz.x * uz;
    d[1] = ((double)c.frame.bx.y * ux + (double)c.frame.by.y * uy) + (double)c.frame.bz.y * uz;
    d[2] = ((double)c.frame.bx.z * ux + (double)c.frame.by.z * uy) + (double)c.frame.bz.z * uz;
}

// The beam of pixel (px, py) — py the image row, as camera_ray takes it.
// False: no beam (the pixel's entry stays the root).
SPT_HD bool entry_beam(const Camera& c, uint32_t px, uint32_t py, EntryBeam& b) {
    if (c.lens_radius != 0.0f) return false;
    const float fr[9] = {c.frame.bx.x, c.frame.bx.y, c.frame.bx.z, c.frame.by.x, c.frame.by.y,
                         c.frame.by.z, c.frame.bz.x, c.frame.bz.y, c.frame.bz.z};
    for (int k = 0; k < 9; k++)
        if (!(fabs((double)fr[k]) <= 1.0000005)) return false;  // unit columns (make_camera), finite
    b.o[0] = (double)c.origin.x; b.o[1] = (double)c.origin.y; b.o[2] = (double)c.origin.z;
    if (!entry_finite(b.o[0]) || !entry_finite(b.o[1]) || !entry_finite(b.o[2])) return false;
    if (!(c.fw >= 1.0f && c.fh >= 1.0f)) return false;
    const double big = 1e18, tiny = 1e-18;
    const double fz = (double)c.dist_lens_to_film, Fz = (double)c.focal_z;
    const double Kx = ((double)c.focal_dist * (double)(c.ratio * c.film_y)) / fz;
    const double Ky = ((double)c.focal_dist * (double)c.film_y) / fz;
    // every f32 intermediate of camera_sample_dir stays in the normal range
    if (!(fabs(fz) >= tiny && fabs(fz) <= big && fabs(Fz) >= tiny && fabs(Fz) <= big)) return false;
    if (!(fabs((double)c.focal_dist) <= big && fabs((double)c.film_y) <= big && fabs((double)c.ratio) <= big)) return false;
    if (!(fabs(Kx) <= big && fabs(Ky) <= big && fabs((double)c.focal_dist * (double)(c.ratio * c.film_y)) <= big &&
          fabs((double)c.focal_dist * (double)c.film_y) <= big))
        return false;
    double lo[3], hi[3], F00[3], F11[3], F[3], d[3];
    for (uint32_t k = 0; k < 4; k++) {
        entry_corner(c, px, py, k & 1u, k >> 1, d, k == 0 ? F00 : (k == 3 ? F11 : F));
        for (int a = 0; a < 3; a++) {
            if (!entry_finite(d[a])) return false;
            lo[a] = k == 0 || d[a] < lo[a] ? d[a] : lo[a];
            hi[a] = k == 0 || d[a] > hi[a] ? d[a] : hi[a];
        }
    }
    const double D2 = (F11[0] - F00[0]) * (F11[0] - F00[0]) + (F11[1] - F00[1]) * (F11[1] - F00[1]);
    const double u = 1.0 / 16777216.0;  // 2^-24
    const double slack = D2 / (2.0 * Fz * Fz) + u * (16.0 + 14.0 * sqrt(Kx * Kx + Ky * Ky) / fabs(Fz));
    if (!entry_finite(slack)) return false;
    const double r = 1.0 / 4194304.0;  // 2^-22: the hardware reciprocal's ulp, and this function's own f64 roundings
    for (int a = 0; a < 3; a++) {
        const double l = lo[a] - slack, h = hi[a] + slack;
        b.con[a] = false;
        b.i0[a] = b.i1[a] = 0.0;
        if (l >= (double)kSlabMinDir) {         // 0 < l <= d <= h: 1 / h <= ix <= 1 / l
            b.con[a] = true;
            b.i0[a] = (1.0 / h) * (1.0 - r);
            b.i1[a] = (1.0 / l) * (1.0 + r);
        } else if (h <= -(double)kSlabMinDir) {  // l <= d <= h < 0: 1 / h <= ix <= 1 / l, both negative
            b.con[a] = true;
            b.i0[a] = (1.0 / h) * (1.0 + r);
            b.i1[a] = (1.0 / l) * (1.0 - r);
        }
    }
    return true;
}

// Child c's meta byte and quantised planes of axis a in the 64-B node w[16].
SPT_HD uint32_t entry_meta6(const uint32_t* w, uint32_t c) { return ((c < 4 ? w[4] : w[5]) >> ((c & 3u) * 8u)) & 0xffu; }
SPT_HD void entry_planes6(const uint32_t* w, uint32_t c, uint32_t a, uint32_t& qlo, uint32_t& qhi) {
    if (c < 4) {
        qlo = (w[7 + 2 * a] >> (c * 8u)) & 0xffu;
        qhi = (w[8 + 2 * a] >> (c * 8u)) & 0xffu;
    } else {
        qlo = (w[13 + a] >> ((c - 4u) * 8u)) & 0xffu;
        qhi = (w[13 + a] >> ((c - 4u) * 8u + 16u)) & 0xffu;
    }
}

// The children of node w[16] some ray of the beam may be accepted into, as
// the ray's visit reads them: bit c for child c (only children whose meta
// byte contributes hit bits; an empty slot never does).
SPT_HD uint32_t entry_visit6(const uint32_t* w, const EntryBeam& b) {
    const uint32_t eb[3] = {(w[5] >> 16) & 0xffu, w[5] >> 24, w[6] >> 24};
    double A[3], B[3], M[3];
    bool con[3];
    for (int a = 0; a < 3; a++) {
        A[a] = (double)u2f(eb[a] << 23);  // as the visit makes it: 2^(e - 127), 0 for e = 0, inf for e = 255
        B[a] = (double)u2f(w[a]) - b.o[a];
        M[a] = 2.0 * (double)kSlabMarginRel * (255.0 * A[a] + fabs(B[a]));
        con[a] = b.con[a];
        if (con[a]) {
            const double im = fabs(b.i0[a]) > fabs(b.i1[a]) ? fabs(b.i0[a]) : fabs(b.i1[a]);
            // (also false for a NaN or an infinity in the node)
            if (!((255.0 * A[a] + fabs(B[a])) * im <= 1e30)) con[a] = false;
        }
    }
    uint32_t mask = 0;
    for (uint32_t c = 0; c < 6; c++) {
        if ((entry_meta6(w, c) >> 5) == 0u) continue;
        double tn = -INFINITY, tf = INFINITY;
        for (uint32_t a = 0; a < 3; a++) {
            if (!con[a]) continue;
            uint32_t qlo, qhi;
            entry_planes6(w, c, a, qlo, qhi);
            const bool pos = b.i0[a] > 0.0;
            // the entry plane is the lo plane for a positive direction; m = M |ix| / 2
            const double ce = (pos ? (double)qlo : (double)qhi) * A[a] + B[a] + (pos ? -M[a] : M[a]);
            const double cx = (pos ? (double)qhi : (double)qlo) * A[a] + B[a] + (pos ? M[a] : -M[a]);
            const double e0 = ce * b.i0[a], e1 = ce * b.i1[a], x0 = cx * b.i0[a], x1 = cx * b.i1[a];
            const double e = (e0 < e1 ? e0 : e1) - 1e-30, x = (x0 > x1 ? x0 : x1) + 1e-30;
            tn = e > tn ? e : tn;
            tf = x < tf ? x : tf;
        }
        if (tn <= tf && tf >= 0.0) mask |= 1u << c;
    }
    return mask;
}

// One step of the descent at node w[16]: true when the beam is accepted into
// exactly one child and that child is an inner node — `word` is then its entry
// word, the node's child-group word in bits 0..23 and the child's slot in bits
// 24..26 (on the device the child sits at (group << group_shift) + slot), and
// `rank` the inner children before it (a compact tree's child: group + rank).
SPT_HD bool entry_descend6(const uint32_t* w, const EntryBeam& b, uint32_t& word, uint32_t& rank) {
    const uint32_t mask = entry_visit6(w, b);
    if (mask == 0u || (mask & (mask - 1u)) != 0u) return false;
    uint32_t c = 0;
    while (!((mask >> c) & 1u)) c++;
    const uint32_t m = entry_meta6(w, c);
    if ((m & 0x18u) != 0x18u) return false;  // a leaf
    rank = 0;
    for (uint32_t i = 0; i < c; i++) {
        const uint32_t mi = entry_meta6(w, i);
        if ((mi >> 5) != 0u && (mi & 0x18u) == 0x18u) rank++;
    }
    word = (w[6] & 0x00ffffffu) | ((m & 7u) << 24);
    return true;
}

}  // namespace spt
