// The BVH refit's per-node arithmetic (csrc/bvh_refit.h) restated serially on
// the host, against the host builders.  For seeded triangle soups of 1, 9, 200
// and 5000 triangles and each node format (80-B eight-wide, 64-B six-wide,
// BVH2):
//   identity   refitting with the vertices the tree was built from leaves
//              every node word as the builder wrote it;
//   perturbed  after a refit with moved vertices (noise, a far outlier, a
//              triangle collapsed to a point, or every z equal: a flat axis)
//              the box each node stores for a child encloses every triangle
//              below that child, empty slots stay inverted and the topology
//              words are untouched.
// Host-only, its own main: tests/test_refit_host.py builds it with the host
// C++ compiler together with bvh_build.cpp and bvh8_build.cpp.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bvh_build.h"
#include "bvh_refit.h"
#include "node6.h"

using namespace spt;

namespace {

long g_bad = 0, g_cases = 0;
void expect(bool ok, const char* what, int fmt, uint64_t n) {
    g_cases++;
    if (ok) return;
    if (g_bad < 20) std::fprintf(stderr, "FAIL %s (format %d, %llu triangles)\n", what, fmt, (unsigned long long)n);
    g_bad++;
}

struct Lcg {
    uint64_t s;
    float next() {  // [0, 1)
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((s >> 40) & 0xffffffu) / 16777216.0f;
    }
};

std::vector<float> soup(uint64_t n, uint64_t seed) {
    Lcg r{seed};
    std::vector<float> tv(n * 9);
    for (uint64_t t = 0; t < n; t++) {
        float c[3] = {r.next() * 10.0f - 5.0f, r.next() * 4.0f, r.next() * 10.0f - 5.0f};
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++) tv[t * 9 + k * 3 + a] = c[a] + (r.next() - 0.5f) * 0.6f;
    }
    return tv;
}

// the 16-float triangle record (vertex k at floats 5 k .. 5 k + 2, then x y again)
std::vector<float> records(const std::vector<float>& tv, const std::vector<uint32_t>& slot2tri) {
    std::vector<float> rec(slot2tri.size() * 16, 0.0f);
    for (size_t s = 0; s < slot2tri.size(); s++) {
        const float* v = &tv[(size_t)slot2tri[s] * 9];
        for (int k = 0; k < 3; k++) {
            float* r = &rec[s * 16 + 5 * k];
            r[0] = v[3 * k]; r[1] = v[3 * k + 1]; r[2] = v[3 * k + 2]; r[3] = v[3 * k]; r[4] = v[3 * k + 1];
        }
    }
    return rec;
}

// the compact 80-B nodes as 64-B nodes (node6.h)
std::vector<uint32_t> node6_of(const std::vector<uint32_t>& n8) {
    bool over = false;
    std::vector<uint32_t> out = to_node6(n8, &over);
    expect(!over, "more than six children", 6, n8.size() / 20);
    return out;
}

struct Tree {
    int fmt;
    uint32_t stride, shift;
    std::vector<uint32_t> nodes;
    std::vector<float> rec;
};

// the serial refit: children first
struct HostBoxes {
    Tree* t;
    RefitBox leaf(uint32_t first, uint32_t count) const {
        RefitBox b = refit_box_empty();
        for (uint32_t i = 0; i < count; i++) refit_box_grow(b, refit_tri_box(&t->rec[(size_t)(first + i) * 16]));
        return b;
    }
    RefitBox inner(uint32_t node) const;
};
RefitBox refit(Tree& t, uint32_t node) {
    RefitKid kid[8];
    return refit_node(t.fmt, &t.nodes[(size_t)node * t.stride], t.shift, HostBoxes{&t}, kid);
}
RefitBox HostBoxes::inner(uint32_t node) const { return refit(*t, node); }

// The box node words store for child c, decoded in double.
void stored_box(const Tree& t, const uint32_t* w, int c, double lo[3], double hi[3], bool& inverted) {
    inverted = t.fmt != kRefitFmt2;
    for (int a = 0; a < 3; a++) {
        if (t.fmt == kRefitFmt2) {
            const int at[2][3][2] = {{{0, 1}, {2, 3}, {8, 9}}, {{4, 5}, {6, 7}, {10, 11}}};
            lo[a] = refit_u2f(w[at[c][a][0]]);
            hi[a] = refit_u2f(w[at[c][a][1]]);
            continue;
        }
        uint32_t e, ql, qh;
        if (t.fmt == kRefitFmt8) {
            const uint32_t sh = (uint32_t)(c & 3) * 8u;
            e = (w[3] >> (8 * a)) & 0xffu;
            ql = (w[8 + 2 * a + (c >> 2)] >> sh) & 0xffu;
            qh = (w[14 + 2 * a + (c >> 2)] >> sh) & 0xffu;
        } else {
            e = a == 0 ? (w[5] >> 16) & 0xffu : (a == 1 ? w[5] >> 24 : w[6] >> 24);
            ql = c < 4 ? (w[7 + 2 * a] >> (c * 8)) & 0xffu : (w[13 + a] >> ((c - 4) * 8)) & 0xffu;
            qh = c < 4 ? (w[8 + 2 * a] >> (c * 8)) & 0xffu : (w[13 + a] >> (16 + (c - 4) * 8)) & 0xffu;
        }
        inverted = inverted && ql == 255u && qh == 0u;
        const double p = refit_u2f(w[a]), step = std::ldexp(1.0, (int)e - 127);
        lo[a] = p + ql * step;
        hi[a] = p + qh * step;
    }
}

// Every triangle below `node` lies inside the box each ancestor stores for
// the child leading to it; returns the exact box of the subtree.
RefitBox check_contains(const Tree& t, uint32_t node, uint64_t n) {
    const uint32_t* w = &t.nodes[(size_t)node * t.stride];
    RefitKid kid[8];
    const int nk = t.fmt == kRefitFmt8 ? 8 : (t.fmt == kRefitFmt6 ? 6 : 2);
    if (t.fmt == kRefitFmt8) refit_kids8(w, t.shift, kid);
    else if (t.fmt == kRefitFmt6) refit_kids6(w, t.shift, kid);
    else refit_kids2(w, kid);
    RefitBox all = refit_box_empty();
    for (int c = 0; c < nk; c++) {
        double lo[3], hi[3];
        bool inverted;
        stored_box(t, w, c, lo, hi, inverted);
        if (!kid[c].inner && !kid[c].count) {
            expect(inverted, "an empty slot is not inverted", t.fmt, n);
            continue;
        }
        if (t.fmt == kRefitFmt2 && c == 1 && w[12] == w[13] && !kid[0].inner) continue;  // the far copy of a root leaf
        RefitBox sub;
        if (kid[c].inner) {
            sub = check_contains(t, kid[c].index, n);
        } else {
            sub = refit_box_empty();
            for (uint32_t i = 0; i < kid[c].count; i++)
                for (int k = 0; k < 3; k++)
                    for (int a = 0; a < 3; a++) {
                        const float x = t.rec[(size_t)(kid[c].index + i) * 16 + 5 * k + a];
                        sub.lo[a] = std::fmin(sub.lo[a], x);
                        sub.hi[a] = std::fmax(sub.hi[a], x);
                    }
        }
        bool in = true;
        for (int a = 0; a < 3; a++) in = in && lo[a] <= (double)sub.lo[a] && (double)sub.hi[a] <= hi[a];
        expect(in, "a child's stored box does not enclose its triangles", t.fmt, n);
        refit_box_grow(all, sub);
    }
    return all;
}

bool topology_kept(const Tree& a, const std::vector<uint32_t>& before) {
    for (size_t i = 0; i < a.nodes.size() / a.stride; i++) {
        const uint32_t *x = &a.nodes[i * a.stride], *y = &before[i * a.stride];
        bool ok;
        if (a.fmt == kRefitFmt8) ok = (x[3] >> 24) == (y[3] >> 24) && !std::memcmp(x + 4, y + 4, 16);
        else if (a.fmt == kRefitFmt6)
            ok = x[3] == y[3] && x[4] == y[4] && (x[5] & 0xffffu) == (y[5] & 0xffffu) &&
                 (x[6] & 0xffffffu) == (y[6] & 0xffffffu);
        else ok = !std::memcmp(x + 12, y + 12, 16);
        if (!ok) return false;
    }
    return true;
}

void run(int fmt, uint64_t n, uint64_t seed) {
    const std::vector<float> tv = soup(n, seed);
    Tree t;
    t.fmt = fmt;
    std::vector<uint32_t> slot2tri;
    if (fmt == kRefitFmt2) {
        BvhBuildResult b = build_bvh(tv.data(), n);
        t.nodes.resize(b.nodes.size());
        std::memcpy(t.nodes.data(), b.nodes.data(), b.nodes.size() * 4);
        slot2tri = b.slot2tri;
        t.stride = 16;
        t.shift = 0;
    } else {
        Bvh8BuildResult b = build_bvh8(tv.data(), n, false, fmt);
        t.nodes = fmt == kRefitFmt6 ? node6_of(b.nodes) : b.nodes;
        slot2tri = b.slot2tri;
        t.stride = fmt == kRefitFmt6 ? 16 : 20;
        t.shift = kRefitCompact;
    }
    const std::vector<uint32_t> built = t.nodes;
    // identity
    t.rec = records(tv, slot2tri);
    refit(t, 0);
    expect(t.nodes == built, "an identity refit changed node words", fmt, n);
    check_contains(t, 0, n);
    // perturbed: noise + a far outlier + a collapsed triangle, then a flat axis
    for (int variant = 0; variant < 2; variant++) {
        std::vector<float> mv = tv;
        Lcg r{seed * 77 + (uint64_t)variant};
        for (float& x : mv) x += (r.next() - 0.5f) * 1.5f;
        if (variant == 0) {
            const uint64_t far = n / 2, flat = n / 3;
            for (int k = 0; k < 9; k++) mv[far * 9 + k] += 1.0e4f;
            if (flat != far)
                for (int k = 3; k < 9; k++) mv[flat * 9 + k] = mv[flat * 9 + k % 3];
        } else {
            for (uint64_t i = 0; i < n * 3; i++) mv[i * 3 + 2] = 0.5f;
        }
        t.nodes = built;
        t.rec = records(mv, slot2tri);
        refit(t, 0);
        check_contains(t, 0, n);
        expect(topology_kept(t, built), "a refit changed topology words", fmt, n);
        // and back: nothing accumulates
        t.rec = records(tv, slot2tri);
        refit(t, 0);
        expect(t.nodes == built, "refitting back did not restore the built nodes", fmt, n);
    }
}

}  // namespace

int main() {
    for (int fmt : {kRefitFmt8, kRefitFmt6, kRefitFmt2})
        for (uint64_t n : {1ull, 9ull, 200ull, 5000ull}) run(fmt, n, 1234 + n);
    std::printf("{\"cases\": %ld, \"bad\": %ld}\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
