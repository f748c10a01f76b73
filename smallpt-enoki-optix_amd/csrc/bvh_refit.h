// bvh_refit.h — the per-node arithmetic of an in-place BVH refit
// (spt_scene_update_geometry): for each of the three device node formats
// (bvh_build.h: the 80-B eight-wide node, the 64-B six-wide node, the BVH2
// node) "which children does this node have and where" and "given the exact
// f32 boxes of the children, rewrite the node's box words and return the
// node's own exact box".  Shared by the device kernels (refit.hip) and by a
// serial host restatement (tests/native/refit_check.cpp), so it includes no
// HIP header and compiles with a plain host C++ compiler.
//
// The wide formats re-quantise with the arithmetic of bvh8_build.cpp emit()
// and gpu_build.hip collapse_emit_kernel: f32 fminf / fmaxf unions, the
// frame (origin = the node's f32 lo, per-axis exponent ceil(log2(ext / 255))
// with the ldexp fix-up, infinite or NaN extent -> 127) and the quantisation
// in double, floor / ceil held to the exact planes lo + q * step and clamped to
// [0, 255], empty slots inverted (255 / 0).
// Topology words (meta bytes, tri_base, the child-group word, the imask, the
// octant slot assignment) are never rewritten.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef SPT_HD
#ifdef __HIPCC__
#define SPT_HD __host__ __device__ __forceinline__  // as spt_math.h
#else
#define SPT_HD inline
#define SPT_REFIT_OWN_HD 1
#endif
#endif

namespace spt {

constexpr int kRefitFmt8 = 8, kRefitFmt6 = 6, kRefitFmt2 = 2;
// group_shift value for the builders' compact layout (host restatement only):
// the r-th inner child of a node, in slot order, is node (group word + r)
constexpr uint32_t kRefitCompact = 0xffffffffu;

struct RefitBox {
    float lo[3], hi[3];
};

// A child of a node.  inner: node slot `index`; else a leaf of `count`
// triangle slots from `index` (count 0: an empty slot).
struct RefitKid {
    uint32_t inner, index, count;
};

SPT_HD uint32_t refit_f2u(float f) { return __builtin_bit_cast(uint32_t, f); }
SPT_HD float refit_u2f(uint32_t u) { return __builtin_bit_cast(float, u); }

SPT_HD RefitBox refit_box_empty() {
    RefitBox b;
    for (int a = 0; a < 3; a++) { b.lo[a] = INFINITY; b.hi[a] = -INFINITY; }
    return b;
}
SPT_HD void refit_box_grow(RefitBox& b, const RefitBox& c) {
    for (int a = 0; a < 3; a++) { b.lo[a] = fminf(b.lo[a], c.lo[a]); b.hi[a] = fmaxf(b.hi[a], c.hi[a]); }
}
// The box of one triangle record (spt_internal.h tri_record_fill: vertex k at
// floats 5 k .. 5 k + 2).  A coordinate that is NaN in all three vertices is
// parked at 0 as bvh_build.cpp does (such a triangle is never hit).
SPT_HD RefitBox refit_tri_box(const float* rec) {
    RefitBox b;
    for (int a = 0; a < 3; a++) {
        b.lo[a] = fminf(fminf(rec[a], rec[5 + a]), rec[10 + a]);
        b.hi[a] = fmaxf(fmaxf(rec[a], rec[5 + a]), rec[10 + a]);
        if (!(b.lo[a] <= b.hi[a])) { b.lo[a] = 0.0f; b.hi[a] = 0.0f; }
    }
    return b;
}
// Half the surface area in double (boxes near FLT_MAX overflow a float).
SPT_HD double refit_half_area(const RefitBox& b) {
    const double dx = (double)b.hi[0] - (double)b.lo[0], dy = (double)b.hi[1] - (double)b.lo[1],
                 dz = (double)b.hi[2] - (double)b.lo[2];
    return dx * dy + dy * dz + dz * dx;
}

// ---- decode: the children of a node

SPT_HD RefitKid refit_meta_kid(uint32_t m, uint32_t group, uint32_t group_shift, uint32_t tri_base, uint32_t& rank) {
    RefitKid k;
    k.inner = 0; k.index = 0; k.count = 0;
    if (!m) return k;
    if ((m & 0x18u) == 0x18u) {  // inner: 0b001_(24 + s)
        k.inner = 1;
        k.index = group_shift == kRefitCompact ? group + rank : (group << group_shift) + ((m & 31u) - 24u);
        rank++;
    } else {  // leaf: unary(count) << 5 | offset
        k.index = tri_base + (m & 31u);
        k.count = (uint32_t)__builtin_popcount(m >> 5);
    }
    return k;
}
// 80-B node (w: at least 20 words), one entry per octant slot.
SPT_HD void refit_kids8(const uint32_t* w, uint32_t group_shift, RefitKid kid[8]) {
    uint32_t rank = 0;
    for (uint32_t s = 0; s < 8; s++)
        kid[s] = refit_meta_kid((w[6 + (s >> 2)] >> ((s & 3u) * 8u)) & 0xffu, w[4], group_shift, w[5], rank);
}
// 64-B node (16 words), one entry per child 0..5.
SPT_HD void refit_kids6(const uint32_t* w, uint32_t group_shift, RefitKid kid[6]) {
    uint32_t rank = 0;
    for (uint32_t c = 0; c < 6; c++) {
        const uint32_t m = c < 4 ? (w[4] >> (c * 8u)) & 0xffu : (w[5] >> ((c - 4u) * 8u)) & 0xffu;
        kid[c] = refit_meta_kid(m, w[6] & 0x00ffffffu, group_shift, w[3], rank);
    }
}
// BVH2 node (16 words): child code >= 0 inner node index, < 0 leaf ~(first << 3 | count - 1).
SPT_HD void refit_kids2(const uint32_t* w, RefitKid kid[2]) {
    for (int c = 0; c < 2; c++) {
        const int32_t code = (int32_t)w[12 + c];
        if (code >= 0) {
            kid[c].inner = 1; kid[c].index = (uint32_t)code; kid[c].count = 0;
        } else {
            const uint32_t l = ~(uint32_t)code;
            kid[c].inner = 0; kid[c].index = l >> 3; kid[c].count = (l & 7u) + 1u;
        }
    }
}

// ---- quantisation frame (bvh8_build.cpp emit())

// The sign of (lo + m) - x in exact arithmetic (the sum's rounding error
// recovered with Knuth's two-sum; s is the double nearest the exact sum, so
// it decides unless it equals x).  The quantised planes lo + q * step are
// compared with it: a difference such as kid.lo - lo rounds in double when a
// coordinate lies far below lo's ulp, or lo far below the step.  0 with NaN.
SPT_HD int refit_plane_cmp(double lo, double m, double x) {
    const double s = lo + m, b = s - lo, err = (lo - (s - b)) + (m - b);
    return s > x ? 1 : (s < x ? -1 : (s == x ? (err > 0.0 ? 1 : (err < 0.0 ? -1 : 0)) : 0));
}

SPT_HD int refit_ebias(float lo, float hi) {
    const double ext = (double)hi - (double)lo;
    int e = -100;
    if (!(ext <= 1e300)) {
        e = 127;  // infinite (or NaN) extent: the widest step; such triangles are never hit
    } else if (ext > 0.0) {
        e = (int)ceil(log2(ext / 255.0));
        while (ldexp(255.0, e) < ext) e++;
        while (e < 127 && refit_plane_cmp(lo, ldexp(255.0, e), hi) < 0) e++;  // ext is rounded: the exact plane
        e = e < -100 ? -100 : (e > 127 ? 127 : e);
    }
    return e + 127;
}
SPT_HD void refit_quant(const RefitBox& kid, const RefitBox& node, const int ebias[3], uint32_t ql[3],
                        uint32_t qh[3]) {
    for (int a = 0; a < 3; a++) {
        const double step = ldexp(1.0, ebias[a] - 127);
        double l = floor(((double)kid.lo[a] - (double)node.lo[a]) / step);
        double h = ceil(((double)kid.hi[a] - (double)node.lo[a]) / step);
        if (refit_plane_cmp(node.lo[a], l * step, kid.lo[a]) > 0) l -= 1.0;  // held to the exact planes
        if (refit_plane_cmp(node.lo[a], h * step, kid.hi[a]) < 0) h += 1.0;
        if (!(l >= 0.0)) l = 0.0;  // NaN-safe
        if (!(h <= 255.0)) h = 255.0;
        if (l > 255.0) l = 255.0;
        if (h < 0.0) h = 0.0;
        ql[a] = (uint32_t)(uint8_t)l;
        qh[a] = (uint32_t)(uint8_t)h;
    }
}

// ---- write: the node's box words from its children's exact boxes

// 80-B node: w0-2 origin, the exponent bytes of w3 (imask kept), w8-19.
SPT_HD RefitBox refit_write8(uint32_t* w, const RefitKid kid[8], const RefitBox kb[8]) {
    RefitBox nb = refit_box_empty();
    for (int s = 0; s < 8; s++)
        if (kid[s].inner || kid[s].count) refit_box_grow(nb, kb[s]);
    int eb[3];
    for (int a = 0; a < 3; a++) {
        eb[a] = refit_ebias(nb.lo[a], nb.hi[a]);
        w[a] = refit_f2u(nb.lo[a]);
    }
    w[3] = (w[3] & 0xff000000u) | (uint32_t)eb[0] | ((uint32_t)eb[1] << 8) | ((uint32_t)eb[2] << 16);
    for (int k = 8; k < 20; k++) w[k] = 0u;
    for (int s = 0; s < 8; s++) {
        uint32_t ql[3] = {255u, 255u, 255u}, qh[3] = {0u, 0u, 0u};  // empty: inverted
        if (kid[s].inner || kid[s].count) refit_quant(kb[s], nb, eb, ql, qh);
        const uint32_t sh = (uint32_t)(s & 3) * 8u;
        for (int a = 0; a < 3; a++) {
            w[8 + 2 * a + (s >> 2)] |= ql[a] << sh;
            w[14 + 2 * a + (s >> 2)] |= qh[a] << sh;
        }
    }
    return nb;
}

// 64-B node: w0-2 origin, the exponent bytes in w5 / w6 (meta and the group
// word kept), w7-12 the planes of children 0..3, w13-15 children 4 and 5.
SPT_HD RefitBox refit_write6(uint32_t* w, const RefitKid kid[6], const RefitBox kb[6]) {
    RefitBox nb = refit_box_empty();
    for (int c = 0; c < 6; c++)
        if (kid[c].inner || kid[c].count) refit_box_grow(nb, kb[c]);
    int eb[3];
    for (int a = 0; a < 3; a++) {
        eb[a] = refit_ebias(nb.lo[a], nb.hi[a]);
        w[a] = refit_f2u(nb.lo[a]);
    }
    w[5] = (w[5] & 0x0000ffffu) | ((uint32_t)eb[0] << 16) | ((uint32_t)eb[1] << 24);
    w[6] = (w[6] & 0x00ffffffu) | ((uint32_t)eb[2] << 24);
    for (int k = 7; k < 16; k++) w[k] = 0u;
    for (int c = 0; c < 6; c++) {
        uint32_t ql[3] = {255u, 255u, 255u}, qh[3] = {0u, 0u, 0u};  // empty: inverted
        if (kid[c].inner || kid[c].count) refit_quant(kb[c], nb, eb, ql, qh);
        for (int a = 0; a < 3; a++) {
            if (c < 4) {
                w[7 + 2 * a] |= ql[a] << (c * 8);
                w[8 + 2 * a] |= qh[a] << (c * 8);
            } else {
                w[13 + a] |= (ql[a] << ((c - 4) * 8)) | (qh[a] << (16 + (c - 4) * 8));
            }
        }
    }
    return nb;
}

// BVH2 node: the two exact child boxes (floats 0-11).  A scene of one leaf has
// a root whose two codes are that leaf, the second behind a far-away point
// box (bvh_build.cpp): that box stays.
SPT_HD RefitBox refit_write2(uint32_t* w, const RefitKid kid[2], const RefitBox kb[2]) {
    const bool dup = w[12] == w[13] && !kid[0].inner;
    RefitBox nb = kb[0];
    w[0] = refit_f2u(kb[0].lo[0]); w[1] = refit_f2u(kb[0].hi[0]); w[2] = refit_f2u(kb[0].lo[1]); w[3] = refit_f2u(kb[0].hi[1]);
    w[8] = refit_f2u(kb[0].lo[2]); w[9] = refit_f2u(kb[0].hi[2]);
    if (dup) return nb;
    w[4] = refit_f2u(kb[1].lo[0]); w[5] = refit_f2u(kb[1].hi[0]); w[6] = refit_f2u(kb[1].lo[1]); w[7] = refit_f2u(kb[1].hi[1]);
    w[10] = refit_f2u(kb[1].lo[2]); w[11] = refit_f2u(kb[1].hi[2]);
    refit_box_grow(nb, kb[1]);
    return nb;
}

// Words per node slot of a format on the device.
SPT_HD uint32_t refit_node_words(int fmt) { return fmt == kRefitFmt8 ? 32u : 16u; }

// One node: decode, fetch the children's exact boxes through `src`
// (src.leaf(first_slot, count): the f32 union of those triangles' boxes;
// src.inner(node_slot): the box that node's own refit returned), rewrite the
// box words in w and return the node's exact box.  kid: the decoded children.
template <class Src>
SPT_HD RefitBox refit_node(int fmt, uint32_t* w, uint32_t group_shift, const Src& src, RefitKid kid[8]) {
    RefitBox kb[8];
    const int n = fmt == kRefitFmt8 ? 8 : (fmt == kRefitFmt6 ? 6 : 2);
    if (fmt == kRefitFmt8) refit_kids8(w, group_shift, kid);
    else if (fmt == kRefitFmt6) refit_kids6(w, group_shift, kid);
    else refit_kids2(w, kid);
    for (int c = 0; c < n; c++) {
        if (kid[c].inner) kb[c] = src.inner(kid[c].index);
        else if (kid[c].count) kb[c] = src.leaf(kid[c].index, kid[c].count);
        else kb[c] = refit_box_empty();
    }
    if (fmt == kRefitFmt8) return refit_write8(w, kid, kb);
    if (fmt == kRefitFmt6) return refit_write6(w, kid, kb);
    return refit_write2(w, kid, kb);
}

}  // namespace spt

#ifdef SPT_REFIT_OWN_HD
#undef SPT_HD
#undef SPT_REFIT_OWN_HD
#endif
