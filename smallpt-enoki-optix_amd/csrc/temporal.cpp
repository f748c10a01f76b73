// temporal.cpp — spt_temporal_accumulate's host side: the argument checks that
// come before any device work, the camera constants of both views and the one
// launch (temporal.hip).  No scene, no allocation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <vector>

#include "camera_make.h"
#include "scene_state.h"
#include "temporal.h"

namespace spt_temporal {
hipError_t launch_temporal(const TemporalArgs& a, hipStream_t s);
}

using namespace spt;

namespace {

struct Range {
    uintptr_t lo, hi;
    const char* name;
};

bool overlap(const Range& a, const Range& b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" {

void spt_default_temporal_params(spt_temporal_params* p) {
    if (!p) return;
    spt_render_params rp;
    spt_default_params(&rp);
    p->width = p->height = 0;
    p->camera = rp.camera;
    p->prev_camera = rp.camera;
    p->samples = 1.0f;
    p->max_history = 64.0f;
    p->sigma_depth = 0.1f;
    p->normal_min = 0.9f;
    p->reserved[0] = p->reserved[1] = 0;
}

spt_status spt_debug_camera_constants(const spt_camera* camera, uint32_t width, uint32_t height, float* out) {
    if (!camera || !out) return fail(SPT_ERR_INVALID, "spt_debug_camera_constants: NULL argument");
    if (width == 0 || height == 0) return fail(SPT_ERR_INVALID, "spt_debug_camera_constants: width/height must be > 0");
    const Camera c = make_camera(*camera, width, height);
    const float v[22] = {c.origin.x, c.origin.y, c.origin.z, c.frame.bx.x, c.frame.bx.y, c.frame.bx.z,
                         c.frame.by.x, c.frame.by.y, c.frame.by.z, c.frame.bz.x, c.frame.bz.y, c.frame.bz.z,
                         c.lens_radius, c.focal_dist, c.dist_lens_to_film, c.ratio, c.film_y, c.fw, c.fh,
                         c.inv_fw, c.inv_fh, c.focal_z};
    for (int k = 0; k < 22; k++) out[k] = v[k];
    return SPT_OK;
}

spt_status spt_temporal_accumulate(const spt_temporal_params* pp, const float* sum, const float* sum_sq,
                                   const spt_aov* cur, const spt_history* prev, const spt_aov* prev_guides,
                                   const spt_history* out, float* film, float* variance, void* stream_) {
    if (!pp) return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: NULL params");
    const spt_temporal_params& p = *pp;
    if (!sum || !sum_sq || !cur || !out)
        return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: NULL sum / sum_sq / cur / out");
    if (!out->color || !out->moment2 || !out->length)
        return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: out needs color, moment2 and length");
    if (!cur->depth || !cur->coverage)
        return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: cur needs depth and coverage");
    if (!prev != !prev_guides)
        return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: prev and prev_guides go together");
    if (prev && (!prev->color || !prev->moment2 || !prev->length))
        return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: prev needs color, moment2 and length");
    if (prev_guides && (!prev_guides->depth || !prev_guides->coverage))
        return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: prev_guides needs depth and coverage");
    if (p.width == 0 || p.height == 0)
        return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: width/height must be > 0");
    if (p.reserved[0] != 0 || p.reserved[1] != 0)
        return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: reserved must be 0");
    if (!(p.samples >= 1.0f) || !std::isfinite(p.samples))
        return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: samples must be finite and >= 1");
    if (!(p.max_history >= 0.0f))
        return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: max_history must be >= 0 (+inf: no cap)");
    if ((uint64_t)p.width * p.height >= (1ull << 31))
        return fail(SPT_ERR_LIMIT, "spt_temporal_accumulate: image too large");
    const size_t P = (size_t)p.width * p.height;

    // every plane the kernel may read, and every plane it writes
    std::vector<Range> in, outs;
    const auto add = [P](std::vector<Range>& v, const float* ptr, size_t planes, const char* name) {
        if (ptr) v.push_back({(uintptr_t)ptr, (uintptr_t)ptr + planes * P * sizeof(float), name});
    };
    add(in, sum, 3, "sum");
    add(in, sum_sq, 3, "sum_sq");
    add(in, cur->depth, 1, "cur.depth");
    add(in, cur->coverage, 1, "cur.coverage");
    add(in, cur->normal_x, 1, "cur.normal_x");
    add(in, cur->normal_y, 1, "cur.normal_y");
    add(in, cur->normal_z, 1, "cur.normal_z");
    if (prev) {
        add(in, prev->color, 3, "prev.color");
        add(in, prev->moment2, 3, "prev.moment2");
        add(in, prev->length, 1, "prev.length");
        add(in, prev_guides->depth, 1, "prev_guides.depth");
        add(in, prev_guides->coverage, 1, "prev_guides.coverage");
        add(in, prev_guides->normal_x, 1, "prev_guides.normal_x");
        add(in, prev_guides->normal_y, 1, "prev_guides.normal_y");
        add(in, prev_guides->normal_z, 1, "prev_guides.normal_z");
    }
    add(outs, out->color, 3, "out.color");
    add(outs, out->moment2, 3, "out.moment2");
    add(outs, out->length, 1, "out.length");
    add(outs, film, 3, "film");
    add(outs, variance, 3, "variance");
    for (size_t a = 0; a < outs.size(); a++) {
        for (const Range& r : in)
            if (overlap(outs[a], r))
                return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: %s overlaps %s", outs[a].name, r.name);
        for (size_t b = a + 1; b < outs.size(); b++)
            if (overlap(outs[a], outs[b]))
                return fail(SPT_ERR_INVALID, "spt_temporal_accumulate: %s overlaps %s", outs[a].name, outs[b].name);
    }

    spt_temporal::TemporalArgs a{};
    a.cam = make_camera(p.camera, p.width, p.height);
    a.prev_cam = make_camera(p.prev_camera, p.width, p.height);
    a.width = p.width;
    a.height = p.height;
    a.samples = p.samples;
    a.max_history = p.max_history;
    a.sigma_depth = p.sigma_depth;
    a.normal_min = p.normal_min;
    a.has_prev = prev ? 1u : 0u;
    a.depth_test = p.sigma_depth > 0.0f ? 1u : 0u;
    a.sum = sum;
    a.sum_sq = sum_sq;
    a.depth = cur->depth;
    a.coverage = cur->coverage;
    a.normal_x = cur->normal_x; a.normal_y = cur->normal_y; a.normal_z = cur->normal_z;
    bool normals = cur->normal_x && cur->normal_y && cur->normal_z;
    if (prev) {
        a.prev_color = prev->color;
        a.prev_moment2 = prev->moment2;
        a.prev_length = prev->length;
        a.prev_depth = prev_guides->depth;
        a.prev_coverage = prev_guides->coverage;
        a.prev_normal_x = prev_guides->normal_x;
        a.prev_normal_y = prev_guides->normal_y;
        a.prev_normal_z = prev_guides->normal_z;
        normals = normals && prev_guides->normal_x && prev_guides->normal_y && prev_guides->normal_z;
    }
    a.normal_test = normals && p.normal_min > -1.0f ? 1u : 0u;
    a.out_color = out->color;
    a.out_moment2 = out->moment2;
    a.out_length = out->length;
    a.film = film;
    a.variance = variance;
    HIP_TRY(spt_temporal::launch_temporal(a, (hipStream_t)stream_));
    return SPT_OK;
}

}  // extern "C"
