// capi.cpp — the C ABI (include/spt.h): scene upload and setters, geometry
// updates, public intersect, hit reconstruction and the denoisers.  The render
// loop is render.cpp, the scene cache scene_cache.cpp (scene_state.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/spt.h"
#include "bvh_build.h"
#include "gpu_build.h"
#include "host_error.h"
#include "render_plan.h"
#include "light_table.h"
#include "sky_table.h"
#include "scene_state.h"
#include "spt_internal.h"

#include "bvh_refit.h"

// Diagnostic build only (make BUILD=build_dbg EXTRA="-g -DSPT_SEGV_TRACE=1"):
// a host segmentation fault prints the native backtrace (library offsets for
// addr2line) before the default action.  Not in the product build.
#ifndef SPT_SEGV_TRACE
#define SPT_SEGV_TRACE 0
#endif
#if SPT_SEGV_TRACE
#include <execinfo.h>
#include <signal.h>
namespace {
void segv_trace(int sig) {
    void* bt[64];
    const int n = backtrace(bt, 64);
    backtrace_symbols_fd(bt, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
struct SegvTraceInstall {
    SegvTraceInstall() { signal(SIGSEGV, segv_trace); }
} segv_trace_install;
}  // namespace
#endif

using namespace spt;

namespace {

thread_local std::string g_last_error;

// LDS stack entries per lane for a BVH8 of `depth` node levels (root = 1).
// Tracer8 pushes the group of node X (level L) only when descending into one
// of X's inner children (level L + 1 <= depth), and the stack then holds one
// group per node on the path root..X: at most depth - 1 entries.  A tight
// stack is LDS, and LDS sets the occupancy (spt_config.stack_slack adds entries).
#ifndef SPT_STACK_CAP
#define SPT_STACK_CAP 0  // experiment only (no overflow handling): cap the LDS stack entries
#endif
uint32_t bvh8_stack_entries(uint32_t depth, uint32_t slack) {
    const uint32_t n = std::max<uint32_t>(1, depth > 1 ? depth - 1 + slack : 1 + slack);
    return SPT_STACK_CAP ? std::min<uint32_t>(n, SPT_STACK_CAP) : n;
}

// The most LDS a workgroup of any trace kernel asks for with `stack_depth`
// entries per lane (kernels.hip launch_*): the stack rows, for the wide
// tracers the per-lane Woop and hit records behind them (Tracer8T::kExtraLds),
// and the fused kernel's parked throughput / radiance (launch_fused_t), with
// light sampling also its parked bounce ray and contribution (nee).
uint64_t stack_lds_bytes(uint32_t stack_depth, uint32_t width, bool nee) {
    return (uint64_t)stack_depth * kIsectBlock * sizeof(uint32_t) + (width != 2 ? 2u * kIsectBlock * 16u : 0u) +
           kIsectBlock * (nee ? 64u : 32u);
}

}  // namespace

namespace spt {

// After a public call's launch on `s` (caller holds sc->mu).  At most 64
// streams are tracked: beyond that the list is drained and restarted.
spt_status record_public_use(spt_scene_t* sc, hipStream_t s) {
    for (auto& u : sc->pub)
        if (u.stream == s) {
            HIP_TRY(hipEventRecord(u.ev, s));
            return SPT_OK;
        }
    if (sc->pub.size() >= 64) {
        for (auto& u : sc->pub) {
            HIP_TRY(hipEventSynchronize(u.ev));
            (void)hipEventDestroy(u.ev);
        }
        sc->pub.clear();
    }
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    sc->pub.push_back({s, e});
    HIP_TRY(hipEventRecord(e, s));
    return SPT_OK;
}

spt_status ensure_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return fail(SPT_ERR_NO_DEVICE, "no HIP device visible (%s)", hipGetErrorString(e));
    return SPT_OK;
}

// Refuses a stack that does not fit the current device's LDS per workgroup,
// before any kernel can be launched with it: the builders do not bound the
// depth of a tree by what the device holds (the GPU builder does not bound it
// at all), and a cache file may claim any stack_depth.
spt_status check_stack_lds(const char* what, uint32_t stack_depth, uint32_t width, bool nee) {
    int dev = 0, cap = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || cap <= 0)
        cap = 64 << 10;
    const uint64_t need = stack_lds_bytes(stack_depth, width, nee);
    if (need > (uint64_t)cap)
        return fail(SPT_ERR_LIMIT, "%s: a traversal stack of depth %u (BVH width %u)%s needs %llu B of LDS per workgroup, "
                    "the device has %d B", what, stack_depth, width, nee ? " with light sampling" : "",
                    (unsigned long long)need, cap);
    return SPT_OK;
}

// Range checks of spt_scene_set_config / spt_scene_create_cfg.
spt_status check_config(const spt_config& c) {
#define CFG_RANGE(f, lo, hi)                                                                         \
    if ((uint64_t)c.f < (uint64_t)(lo) || (uint64_t)c.f > (uint64_t)(hi))                           \
        return fail(SPT_ERR_INVALID, "spt_config.%s = %llu outside [%llu, %llu]", #f, (unsigned long long)c.f, \
                    (unsigned long long)(lo), (unsigned long long)(hi));
    CFG_RANGE(build, 0, SPT_BUILD_GPU_PLOC)
    if (c.bvh_width != 2 && c.bvh_width != 6 && c.bvh_width != 8)
        return fail(SPT_ERR_INVALID, "spt_config.bvh_width must be 2, 6 or 8");
    CFG_RANGE(collapse, 0, 1)
    if (c.ploc_radius != 8 && c.ploc_radius != 16 && c.ploc_radius != 32 && c.ploc_radius != 64)
        return fail(SPT_ERR_INVALID, "spt_config.ploc_radius must be 8, 16, 32 or 64");
    CFG_RANGE(stack_slack, 0, 64)
    CFG_RANGE(pipeline, 0, SPT_PIPELINE_FUSED)
    CFG_RANGE(wavefront_paths, 1, 0x7fffffffu)
    CFG_RANGE(streams, 1, kMaxStreams)
    CFG_RANGE(isect_refill_idle, 1, 64)
    CFG_RANGE(isect_static_share_q8, 0, 255)
    CFG_RANGE(isect_chunk, 1, 4096)
    CFG_RANGE(isect_grid_q8, 0, 4096)
    CFG_RANGE(xcd_remap, 0, 7)
    CFG_RANGE(fused_refill_idle, 1, 64)
    CFG_RANGE(fused_static_share_q8, 0, 255)
    CFG_RANGE(fused_grid_q8, 0, 4096)
    CFG_RANGE(plane_pad, 0, 1u << 20)
    CFG_RANGE(film_budget_bytes, 12, UINT64_MAX)
    CFG_RANGE(public_persistent, 0, 1)
    CFG_RANGE(public_refill_idle, 1, 64)
    CFG_RANGE(pack_groups, 0, 2)
    CFG_RANGE(pixel_block, 0, 64)
    CFG_RANGE(work_order, 0, SPT_WORK_PIXEL_MAJOR)
    CFG_RANGE(queue_cache, 0, SPT_QUEUE_CACHE_STREAM)
    CFG_RANGE(drain_q8, 0, 65535)
    CFG_RANGE(drain_grid_q8, 0, 4096)
    CFG_RANGE(drain_casts, 0, 64)
    CFG_RANGE(fit_streams, 1, kMaxStreams)
    CFG_RANGE(fit_paths, 0, 1ull << 31)
    CFG_RANGE(sub_queues, 0, 1)
    CFG_RANGE(drain_sort, 0, 1)
    CFG_RANGE(lockstep_first, 0, 3)
    CFG_RANGE(fit_chunks, 0, 1)
    CFG_RANGE(drain_refill_idle, 0, 64)
#undef CFG_RANGE
    return SPT_OK;
}

// Rebuild the texture device arrays from the host copies (caller holds sc->mu):
// one texel array, one (first, w, h, has) entry per material.
spt_status upload_textures(spt_scene_t* sc) {
    std::vector<uint4> info(sc->tex_img.size());
    std::vector<float4> all;
    uint32_t used = 0;
    for (size_t m = 0; m < sc->tex_img.size(); m++) {
        const bool has = !sc->tex_img[m].empty();
        info[m] = make_uint4((uint32_t)all.size(), sc->tex_w[m], sc->tex_h[m], has ? 1u : 0u);
        all.insert(all.end(), sc->tex_img[m].begin(), sc->tex_img[m].end());
        if (has) used = (uint32_t)m + 1;
    }
    hfree(sc->tex_info);
    hfree(sc->texels);
    sc->ntex = 0;
    if (used) {
        spt_status us = upload(&sc->tex_info, info.data(), sizeof(uint4) * used);
        if (!us) us = upload(&sc->texels, all.data(), sizeof(float4) * all.size());
        if (us) return us;
        sc->ntex = used;
    }
    return SPT_OK;
}

}  // namespace spt

namespace {

// spt_scene_create on the GPU: upload the indexed mesh as is, assemble the
// triangle soup, PLOC + collapse (gpu_build.hip), slot-ordered arrays.
spt_status create_scene_gpu(const int32_t* pos_tri, const float* pos, uint64_t nvert, uint64_t ntri,
                            const int32_t* nrm_tri, const float* nrm, uint64_t nnrm, const int32_t* tc_tri,
                            const float* tc, uint64_t ntc, const int32_t* mat_id, const spt_config& cfg, double t0,
                            spt_scene* out) {
    struct Raw {
        int32_t *pt = nullptr, *nt = nullptr, *tt = nullptr, *mat = nullptr;
        float *p = nullptr, *n = nullptr, *t = nullptr, *tv = nullptr;
        ~Raw() { hfree(pt); hfree(nt); hfree(tt); hfree(mat); hfree(p); hfree(n); hfree(t); hfree(tv); }
    } raw;
    spt_status us = SPT_OK;
    if (!us) us = upload(&raw.pt, pos_tri, ntri * 3 * sizeof(int32_t));
    if (!us) us = upload(&raw.p, pos, nvert * 3 * sizeof(float));
    if (!us && nrm_tri) us = upload(&raw.nt, nrm_tri, ntri * 3 * sizeof(int32_t));
    if (!us && nrm_tri) us = upload(&raw.n, nrm, nnrm * 3 * sizeof(float));
    const bool with_tc = tc_tri && tc;
    if (!us && with_tc) us = upload(&raw.tt, tc_tri, ntri * 3 * sizeof(int32_t));
    if (!us && with_tc) us = upload(&raw.t, tc, ntc * 2 * sizeof(float));
    if (!us && mat_id) us = upload(&raw.mat, mat_id, ntri * sizeof(int32_t));
    if (us) return us;
    HIP_TRY(hipMalloc((void**)&raw.tv, sizeof(float) * 9 * std::max<uint64_t>(ntri, 1)));
    DeviceMeshIn m{raw.pt, raw.p, raw.nt, raw.n, raw.tt, raw.t, raw.mat, (uint32_t)ntri};
    hipStream_t s = nullptr;  // the null stream: scene creation is synchronous
    HIP_TRY(gpu_mesh_soup(m, raw.tv, s));
    GpuBvh8 g;
    const int width = (int)cfg.bvh_width;
    HIP_TRY(gpu_build_bvh8(raw.tv, (uint32_t)ntri, s, &g, (int)cfg.ploc_radius, cfg.collapse == 1, width));
    if ((us = check_stack_lds("spt_scene_create (GPU build)", bvh8_stack_entries(g.depth, cfg.stack_slack), cfg.bvh_width))) {
        (void)hipFree(g.nodes8);
        (void)hipFree(g.slot2tri);
        return us;
    }
    spt_scene_t* sc = new spt_scene_t();
    sc->cfg = cfg;
    (void)hipGetDevice(&sc->device);
    sc->ntri = ntri;
    sc->stack_depth = bvh8_stack_entries(g.depth, cfg.stack_slack);
    uint32_t nslots = 0;
    {
        uint32_t* holes = nullptr;
        const hipError_t he = gpu_bvh8_holes(g.nodes8, g.nnodes, s, &holes, &nslots, width,
                                             cfg.pack_groups ? &sc->group_shift : nullptr, cfg.pack_groups == 2);
        (void)hipFree(g.nodes8);
        if (he) {
            (void)hipFree(g.slot2tri);
            delete sc;
            return fail(he == hipErrorOutOfMemory ? SPT_ERR_OOM : SPT_ERR_HIP, "spt_scene_create (BVH8 layout): %s",
                        hipGetErrorString(he));
        }
        sc->nodes8 = (uint4*)holes;
        sc->node6 = width == 6;
        sc->node_bytes = holes ? (uint64_t)nslots * (width == 6 ? kNode6Quads : kNode8Quads) * 16 : 0;
    }
    auto bail = [&](hipError_t e) {
        (void)hipFree(g.slot2tri);
        sc->release();
        delete sc;
        return fail(e == hipErrorOutOfMemory ? SPT_ERR_OOM : SPT_ERR_HIP, "spt_scene_create (GPU build): %s",
                    hipGetErrorString(e));
    };
    hipError_t e = hipSuccess;
    if (!e) e = hipMalloc((void**)&sc->tris, sizeof(float4) * kTriQuads * std::max<uint64_t>(ntri, 1));
    if (!e) e = hipMalloc((void**)&sc->snrm, sizeof(float4) * 3 * std::max<uint64_t>(ntri, 1));
    if (!e && with_tc) e = hipMalloc((void**)&sc->tc, sizeof(float) * 6 * ntri);
    if (!e) e = hipMalloc((void**)&sc->orig2slot, sizeof(int32_t) * std::max<uint64_t>(ntri, 1));
    if (!e) e = gpu_scene_slots(m, raw.tv, g.slot2tri, sc->tris, sc->snrm, with_tc ? sc->tc : nullptr,
                                sc->orig2slot, s);
    if (!e) e = hipStreamSynchronize(s);
    if (e) return bail(e);
    (void)hipFree(g.slot2tri);
    const float one[3] = {1.0f, 1.0f, 1.0f};
    if ((us = upload(&sc->albedo, one, sizeof(one)))) {
        sc->release();
        delete sc;
        return us;
    }
    sc->nmat = 1;
    spt_scene_stats& ss = sc->stats;
    ss.ntri = ntri;
    ss.nodes = g.nnodes;
    ss.leaves = g.leaves;
    ss.max_depth = g.depth;
    ss.max_leaf = 3;
    ss.bvh_width = (uint32_t)width;
    ss.builder = SPT_BUILD_GPU_PLOC;
    ss.device_bytes = (uint64_t)nslots * (width == 6 ? kNode6Quads : kNode8Quads) * 16 + ntri * (kTriQuads + 3) * 16 +
                      (with_tc ? ntri * 24 : 0) + ntri * 4;
    ss.build_ms = now_ms() - t0;
    ss.sah_cost = g.sah_cost;
    *out = sc;
    return SPT_OK;
}

}  // namespace

spt_status spt_set_error(spt_status code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

extern "C" {

const char* spt_last_error(void) { return g_last_error.c_str(); }
const char* spt_version(void) { return "spt-mi355x 0.1 (gfx950 wavefront path tracer)"; }

#ifndef SPT_BUILD_ID
#define SPT_BUILD_ID "unknown"
#endif
const char* spt_build_id(void) { return SPT_BUILD_ID; }

spt_status spt_init(int32_t device) {
    spt_status st = ensure_device();
    if (st) return st;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(nullptr));  // create the context now, not in the first timed call
    return SPT_OK;
}

void spt_default_params(spt_render_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->width = 512; p->height = 512; p->spp = 100; p->max_depth = 2;  // main.cpp:357-361
    const float from[3] = {0.0f, 3.03f, 5.0f}, at[3] = {0.0f, 0.03f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    std::memcpy(p->camera.look_from, from, sizeof(from));               // main.cpp:383
    std::memcpy(p->camera.look_at, at, sizeof(at));
    std::memcpy(p->camera.up, up, sizeof(up));
    p->camera.lens_radius = 0.0f;
    p->camera.focal_dist = 1.0f;
    p->camera.fov_y = 40.0f / 180.0f * (float)M_PI;
    p->camera.film_size_y = 0.035f;                                    // pinhole.h:11
    p->tile_index = 0; p->tile_count = 1; p->rows_per_group = 1;
    p->wavefront_paths = 0;
    p->rr_start_depth = 1;
    p->rng_order = SPT_RNG_Y_FIRST;
    p->rng_initstate = kPcgDefaultState;
    p->env[0] = p->env[1] = p->env[2] = 1.0f;
    p->flags = 0;
}

uint32_t spt_tile_rows(uint32_t height, uint32_t tile_index, uint32_t tile_count, uint32_t rows_per_group,
                       uint32_t* rows, uint32_t cap) {
    if (tile_count == 0 || rows_per_group == 0 || tile_index >= tile_count) return 0;
    uint32_t n = 0;
    for (uint32_t r = 0; r < height; r++) {
        if ((r / rows_per_group) % tile_count != tile_index) continue;
        if (rows && n < cap) rows[n] = r;
        n++;
    }
    return n;
}

spt_status spt_scene_create(const int32_t* pos_tri, const float* pos, uint64_t nvert, uint64_t ntri,
                            const int32_t* nrm_tri, const float* nrm, uint64_t nnrm, const int32_t* tc_tri,
                            const float* tc, uint64_t ntc, const int32_t* mat_id, spt_scene* out) {
    return spt_scene_create_ex(pos_tri, pos, nvert, ntri, nrm_tri, nrm, nnrm, tc_tri, tc, ntc, mat_id, SPT_BUILD_AUTO,
                               out);
}

spt_status spt_scene_create_ex(const int32_t* pos_tri, const float* pos, uint64_t nvert, uint64_t ntri,
                               const int32_t* nrm_tri, const float* nrm, uint64_t nnrm, const int32_t* tc_tri,
                               const float* tc, uint64_t ntc, const int32_t* mat_id, uint32_t build,
                               spt_scene* out) {
    if (build > SPT_BUILD_GPU_PLOC) return fail(SPT_ERR_INVALID, "spt_scene_create: unknown builder %u", build);
    spt_config cfg;
    spt_default_config(&cfg);
    cfg.build = build;
    return spt_scene_create_cfg(pos_tri, pos, nvert, ntri, nrm_tri, nrm, nnrm, tc_tri, tc, ntc, mat_id, &cfg, out);
}

spt_status spt_scene_create_cfg(const int32_t* pos_tri, const float* pos, uint64_t nvert, uint64_t ntri,
                                const int32_t* nrm_tri, const float* nrm, uint64_t nnrm, const int32_t* tc_tri,
                                const float* tc, uint64_t ntc, const int32_t* mat_id, const spt_config* cfg_in,
                                spt_scene* out) {
    if (!out) return fail(SPT_ERR_INVALID, "spt_scene_create: out is NULL");
    *out = nullptr;
    spt_config cfg;
    if (cfg_in) cfg = *cfg_in;
    else spt_default_config(&cfg);
    spt_status st = check_config(cfg);
    if (st) return st;
    if (ntri > 0 && (!pos_tri || !pos)) return fail(SPT_ERR_INVALID, "spt_scene_create: NULL positions");
    if (ntri >= kMaxTriangles) return fail(SPT_ERR_LIMIT, "spt_scene_create: %llu triangles exceeds 2^28", (unsigned long long)ntri);
    if (nrm_tri && !nrm && nnrm) return fail(SPT_ERR_INVALID, "spt_scene_create: normal indices without normals");
    st = ensure_device();
    if (st) return st;
    uint32_t build = cfg.build;
    if (build == SPT_BUILD_AUTO) build = ntri >= cfg.gpu_build_min_tris ? SPT_BUILD_GPU_PLOC : SPT_BUILD_HOST_SAH;
    const bool use8 = cfg.bvh_width != 2;  // compressed wide BVH (8 or 6 children per node)
    const int width = (int)cfg.bvh_width;
    if (build == SPT_BUILD_GPU_PLOC && !use8) build = SPT_BUILD_HOST_SAH;  // the GPU builder makes BVH8 only
    const double t0 = now_ms();
    const bool host = build == SPT_BUILD_HOST_SAH;
    std::vector<float> tv(host ? (size_t)ntri * 9 : 0);
    for (uint64_t t = 0; t < ntri; t++) {
        for (int k = 0; k < 3; k++) {
            int64_t pi = pos_tri[t * 3 + k];
            if (pi < 0 || (uint64_t)pi >= nvert)
                return fail(SPT_ERR_INVALID, "spt_scene_create: triangle %llu position index %lld out of range [0,%llu)",
                            (unsigned long long)t, (long long)pi, (unsigned long long)nvert);
            if (host)
                for (int c = 0; c < 3; c++) tv[t * 9 + k * 3 + c] = pos[pi * 3 + c];
        }
        if (nrm_tri)
            for (int k = 0; k < 3; k++) {
                int64_t ni = nrm_tri[t * 3 + k];
                if (ni < -1 || (ni >= 0 && (uint64_t)ni >= nnrm))
                    return fail(SPT_ERR_INVALID, "spt_scene_create: triangle %llu normal index %lld out of range",
                                (unsigned long long)t, (long long)ni);
            }
        if (tc_tri && tc)
            for (int k = 0; k < 3; k++) {
                int64_t ti = tc_tri[t * 3 + k];
                if (ti < -1 || (ti >= 0 && (uint64_t)ti >= ntc))
                    return fail(SPT_ERR_INVALID, "spt_scene_create: triangle %llu texcoord index %lld out of range",
                                (unsigned long long)t, (long long)ti);
            }
    }
    if (!host)
        return create_scene_gpu(pos_tri, pos, nvert, ntri, nrm_tri, nrm, nnrm, tc_tri, tc, ntc, mat_id, cfg, t0, out);
    // Acceleration structure: the compressed 8-wide BVH by default;
    // spt_config.bvh_width = 2 selects the plain BVH2 (the simple reference layout).
    BvhBuildResult bvh;
    Bvh8BuildResult bvh8;
    if (use8)
        bvh8 = build_bvh8(tv.data(), ntri, cfg.collapse == 1, width);
    else
        bvh = build_bvh(tv.data(), ntri);
    const std::vector<uint32_t>& slot2tri = use8 ? bvh8.slot2tri : bvh.slot2tri;
    const double t1 = now_ms();
    const uint32_t stack_depth =
        use8 ? bvh8_stack_entries(bvh8.depth, cfg.stack_slack) : std::max<uint32_t>(1, bvh.max_depth + 1);
    if ((st = check_stack_lds("spt_scene_create", stack_depth, cfg.bvh_width))) return st;

    // Slot-ordered device arrays.
    std::vector<float4> h_tris((size_t)ntri * kTriQuads), h_snrm((size_t)ntri * 3);
    std::vector<float> h_tc(tc_tri && tc ? (size_t)ntri * 6 : 0);
    std::vector<int32_t> h_o2s((size_t)ntri);
    for (uint64_t s = 0; s < ntri; s++) {
        const uint32_t t = slot2tri[s];
        h_o2s[t] = (int32_t)s;
        const float* v = &tv[(size_t)t * 9];
        tri_record_fill((float*)&h_tris[s * kTriQuads], v, t);
        // Geometric normal fallback for a missing vertex normal (index -1).
        V3 g = normalize(cross(v3(v[3] - v[0], v[4] - v[1], v[5] - v[2]), v3(v[6] - v[0], v[7] - v[1], v[8] - v[2])));
        int32_t mat = mat_id ? mat_id[t] : 0;
        for (int k = 0; k < 3; k++) {
            int64_t ni = nrm_tri ? nrm_tri[t * 3 + k] : -1;
            V3 n = ni >= 0 ? v3(nrm[ni * 3], nrm[ni * 3 + 1], nrm[ni * 3 + 2]) : g;
            float w = 0.0f;
            if (k == 0) std::memcpy(&w, &mat, 4);
            h_snrm[s * 3 + k] = make_float4(n.x, n.y, n.z, w);
        }
        if (!h_tc.empty())
            for (int k = 0; k < 3; k++) {
                int64_t ti = tc_tri[t * 3 + k];
                h_tc[s * 6 + k * 2] = ti >= 0 ? tc[ti * 2] : 0.0f;
                h_tc[s * 6 + k * 2 + 1] = ti >= 0 ? tc[ti * 2 + 1] : 0.0f;
            }
    }

    spt_scene_t* sc = new spt_scene_t();
    sc->cfg = cfg;
    (void)hipGetDevice(&sc->device);
    sc->ntri = ntri;
    sc->stack_depth = stack_depth;
    const float one[3] = {1.0f, 1.0f, 1.0f};
    spt_status us = SPT_OK;
    uint32_t nslots = 0;
    if (use8) {
        // pad each 80-B node to its own 128-B cache line (kNode8Quads x 16 B),
        // then re-lay it on the device with the children at w4 + slot
        const size_t nn = bvh8.nodes.size() / 20;
        std::vector<uint32_t> padded(nn * kNode8Quads * 4, 0u);
        for (size_t i = 0; i < nn; i++)
            std::memcpy(&padded[i * kNode8Quads * 4], &bvh8.nodes[i * 20], 80);
        uint32_t* compact = nullptr;
        if (!us) us = upload(&compact, padded.data(), padded.size() * sizeof(uint32_t));
        if (!us) {
            uint32_t* holes = nullptr;
            const hipError_t he = gpu_bvh8_holes(compact, (uint32_t)nn, nullptr, &holes, &nslots, width,
                                                 cfg.pack_groups ? &sc->group_shift : nullptr, cfg.pack_groups == 2);
            if (he) us = fail(he == hipErrorOutOfMemory ? SPT_ERR_OOM : SPT_ERR_HIP,
                              "spt_scene_create (BVH8 layout): %s", hipGetErrorString(he));
            else {
                sc->nodes8 = (uint4*)holes;
                sc->node6 = width == 6;
                sc->node_bytes = holes ? (uint64_t)nslots * (width == 6 ? kNode6Quads : kNode8Quads) * 16 : 0;
            }
        }
        hfree(compact);
    } else {
        if (!us) us = upload(&sc->nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(float));
        if (!us && sc->nodes) sc->node_bytes = bvh.nodes.size() * sizeof(float);
    }
    if (!us) us = upload(&sc->tris, h_tris.data(), h_tris.size() * sizeof(float4));
    if (!us) us = upload(&sc->snrm, h_snrm.data(), h_snrm.size() * sizeof(float4));
    if (!us) us = upload(&sc->tc, h_tc.data(), h_tc.size() * sizeof(float));
    if (!us) us = upload(&sc->orig2slot, h_o2s.data(), h_o2s.size() * sizeof(int32_t));
    if (!us) us = upload(&sc->albedo, one, sizeof(one));
    if (us) {
        sc->release();
        delete sc;
        return us;
    }
    sc->nmat = 1;
    spt_scene_stats& ss = sc->stats;
    ss.ntri = ntri;
    ss.nodes = use8 ? bvh8.nodes.size() / 20 : bvh.nodes.size() / 16;
    ss.leaves = use8 ? bvh8.leaves : bvh.leaves;
    ss.max_depth = use8 ? bvh8.depth : bvh.max_depth;
    ss.max_leaf = use8 ? 3 : bvh.max_leaf;
    ss.bvh_width = (uint32_t)width;
    ss.device_bytes = (use8 ? (uint64_t)nslots * (width == 6 ? kNode6Quads : kNode8Quads) * 16 : bvh.nodes.size() * 4) +
                      (h_tris.size() + h_snrm.size()) * 16 +
                      h_tc.size() * 4 + h_o2s.size() * 4;
    ss.build_ms = t1 - t0;
    ss.sah_cost = use8 ? bvh8.sah_cost : bvh.sah_cost;
    ss.builder = SPT_BUILD_HOST_SAH;
    *out = sc;
    return SPT_OK;
}

spt_status spt_scene_set_albedo(spt_scene sc, const float* albedo_rgb, uint32_t nmat) {
    if (!sc || !albedo_rgb || nmat == 0) return fail(SPT_ERR_INVALID, "spt_scene_set_albedo: bad arguments");
    DeviceGuard dg(sc->device);
    float* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, sizeof(float) * 3 * nmat));
    HIP_TRY(hipMemcpy(d, albedo_rgb, sizeof(float) * 3 * nmat, hipMemcpyHostToDevice));
    std::lock_guard<std::mutex> lk(sc->mu);
    spt_status qs = quiesce_scene(sc);  // queued renders / calls may still read the old table
    if (qs) {
        hfree(d);
        return qs;
    }
    hfree(sc->albedo);
    sc->albedo = d;
    sc->nmat = nmat;
    bool unit = true;
    for (uint32_t i = 0; i < 3 * nmat; i++) unit = unit && albedo_rgb[i] == 1.0f;
    sc->albedo_unit = unit;
    return SPT_OK;
}

namespace {

// The scene's light table from its own records (light_table.h; caller holds
// sc->mu, has made the device current and quiesced the scene).  *out: null for
// an empty table; the scene is not touched.
spt_status build_scene_lights(spt_scene_t* sc, const char* what, DeviceLights** out, uint32_t* nout) {
    *out = nullptr;
    *nout = 0;
    if (!sc->emission || sc->nemit == 0 || sc->ntri == 0) return SPT_OK;
    const uint32_t ntri = (uint32_t)sc->ntri;
    std::vector<float> emi((size_t)sc->nemit * 3);
    HIP_TRY(hipMemcpy(emi.data(), sc->emission, emi.size() * sizeof(float), hipMemcpyDeviceToHost));
    struct Tmp {
        int32_t* mat = nullptr;
        uint32_t* ids = nullptr;
        float* tv = nullptr;
        ~Tmp() { hfree(mat); hfree(ids); hfree(tv); }
    } d;
    std::vector<int32_t> mat(ntri);
    HIP_TRY(hipMalloc((void**)&d.mat, sizeof(int32_t) * ntri));
    HIP_TRY(launch_light_mats(sc->snrm, sc->orig2slot, ntri, d.mat, nullptr));
    HIP_TRY(hipMemcpy(mat.data(), d.mat, sizeof(int32_t) * ntri, hipMemcpyDeviceToHost));
    std::vector<uint32_t> ids;
    std::vector<int32_t> lmat;
    for (uint32_t t = 0; t < ntri; t++) {
        const int32_t m = mat[t];
        if (m < 0 || (uint32_t)m >= sc->nemit) continue;
        if (emi[(size_t)m * 3] == 0.0f && emi[(size_t)m * 3 + 1] == 0.0f && emi[(size_t)m * 3 + 2] == 0.0f) continue;
        ids.push_back(t);
        lmat.push_back(m);
    }
    if (ids.empty()) return SPT_OK;
    if (ids.size() > kMaxLights)
        return fail(SPT_ERR_LIMIT, "%s: %zu emissive triangles (at most %u)", what, ids.size(), kMaxLights);
    const uint32_t n = (uint32_t)ids.size();
    std::vector<float> tv((size_t)n * 9);
    spt_status us = upload(&d.ids, ids.data(), sizeof(uint32_t) * n);
    if (us) return us;
    HIP_TRY(hipMalloc((void**)&d.tv, sizeof(float) * 9 * n));
    HIP_TRY(launch_light_tris(sc->tris, sc->orig2slot, d.ids, n, d.tv, nullptr));
    HIP_TRY(hipMemcpy(tv.data(), d.tv, sizeof(float) * 9 * n, hipMemcpyDeviceToHost));
    LightTable lt;
    light_table_build(tv.data(), lmat.data(), n, emi.data(), sc->nemit, lt);
    if (lt.empty()) return SPT_OK;
    // (every compacted triangle is a member: the table's ids index `ids`)
    std::vector<uint32_t> orig(lt.ids.size());
    for (size_t i = 0; i < orig.size(); i++) orig[i] = ids[lt.ids[i]];
    const size_t rec_bytes = lt.rec.size() * sizeof(float), cdf_bytes = lt.cdf.size() * sizeof(float);
    std::vector<unsigned char> buf(sizeof(DeviceLights) + rec_bytes + cdf_bytes + orig.size() * sizeof(uint32_t));
    DeviceLights h{};
    h.n = (uint32_t)lt.ids.size();
    std::memcpy(buf.data(), &h, sizeof(h));
    std::memcpy(buf.data() + sizeof(h), lt.rec.data(), lt.rec.size() * sizeof(float));
    std::memcpy(buf.data() + sizeof(h) + rec_bytes, lt.cdf.data(), cdf_bytes);
    std::memcpy(buf.data() + sizeof(h) + rec_bytes + cdf_bytes, orig.data(), orig.size() * sizeof(uint32_t));
    DeviceLights* dl = nullptr;
    if ((us = upload(&dl, buf.data(), buf.size()))) return us;
    *out = dl;
    *nout = h.n;
    return SPT_OK;
}

// After a change of the emission table or the geometry of a scene with the
// switch on: the table again.  A table that cannot be rebuilt (or whose
// kernels' LDS the device cannot hold) turns the switch off with the error.
spt_status rebuild_scene_lights(spt_scene_t* sc, const char* what) {
    if (!sc->light_sampling) return SPT_OK;
    DeviceLights* dl = nullptr;
    uint32_t n = 0;
    spt_status st = build_scene_lights(sc, what, &dl, &n);
    if (!st && dl && (st = check_stack_lds(what, sc->stack_depth, sc->cfg.bvh_width, true))) hfree(dl);
    hfree(sc->lights);
    sc->lights = st ? nullptr : dl;
    sc->nlights = st ? 0 : n;
    if (st) sc->light_sampling = false;
    return st;
}

spt_status set_emission_locked(spt_scene_t* sc, const float* emission_rgb, uint32_t nmat);

}  // namespace

spt_status spt_scene_set_light_sampling(spt_scene sc, uint32_t on) {
    static const char* what = "spt_scene_set_light_sampling";
    if (!sc) return fail(SPT_ERR_INVALID, "%s: NULL scene", what);
    if (on > 1) return fail(SPT_ERR_INVALID, "%s: on = %u (0 or 1)", what, on);
    DeviceGuard dg(sc->device);
    std::lock_guard<std::mutex> lk(sc->mu);
    spt_status st = quiesce_scene(sc);  // queued renders may still read the old table
    if (st) return st;
    DeviceLights* dl = nullptr;
    uint32_t n = 0;
    if (on) {
        if ((st = build_scene_lights(sc, what, &dl, &n))) return st;
        if (dl && (st = check_stack_lds(what, sc->stack_depth, sc->cfg.bvh_width, true))) {
            hfree(dl);
            return st;
        }
    }
    hfree(sc->lights);
    sc->lights = dl;
    sc->nlights = n;
    sc->light_sampling = on != 0;
    return SPT_OK;
}

spt_status spt_scene_get_light_sampling(spt_scene sc, uint32_t* on, uint32_t* nlights) {
    if (!sc) return fail(SPT_ERR_INVALID, "spt_scene_get_light_sampling: NULL scene");
    std::lock_guard<std::mutex> lk(sc->mu);
    if (on) *on = sc->light_sampling ? 1u : 0u;
    if (nlights) *nlights = sc->nlights;
    return SPT_OK;
}

spt_status spt_light_table_build(const float* tri_vertices, const int32_t* mat_id, uint64_t ntri,
                                 const float* emission_rgb, uint32_t nmat, uint32_t* ids, float* cdf, float* pdf_area,
                                 uint32_t capacity, uint32_t* n_out) {
    static const char* what = "spt_light_table_build";
    if (!n_out) return fail(SPT_ERR_INVALID, "%s: NULL n_out", what);
    if (ntri && !tri_vertices) return fail(SPT_ERR_INVALID, "%s: NULL vertices", what);
    if (nmat && !emission_rgb) return fail(SPT_ERR_INVALID, "%s: NULL emission with nmat = %u", what, nmat);
    if (ntri >= kMaxTriangles) return fail(SPT_ERR_LIMIT, "%s: %llu triangles exceeds 2^28", what, (unsigned long long)ntri);
    LightTable lt;
    light_table_build(tri_vertices, mat_id, ntri, emission_rgb, nmat, lt);
    if (lt.ids.size() > kMaxLights)
        return fail(SPT_ERR_LIMIT, "%s: %zu emissive triangles (at most %u)", what, lt.ids.size(), kMaxLights);
    *n_out = (uint32_t)lt.ids.size();
    if (!ids && !cdf && !pdf_area) return SPT_OK;  // the size call
    if (capacity < lt.ids.size())
        return fail(SPT_ERR_INVALID, "%s: capacity %u, the table has %zu lights", what, capacity, lt.ids.size());
    for (size_t i = 0; i < lt.ids.size(); i++) {
        if (ids) ids[i] = lt.ids[i];
        if (cdf) cdf[i] = lt.cdf[i];
        if (pdf_area) pdf_area[i] = lt.pdfA[i];
    }
    return SPT_OK;
}

spt_status spt_scene_set_emission(spt_scene sc, const float* emission_rgb, uint32_t nmat) {
    if (!sc) return fail(SPT_ERR_INVALID, "spt_scene_set_emission: NULL scene");
    DeviceGuard dg(sc->device);
    std::lock_guard<std::mutex> lk(sc->mu);
    spt_status st = set_emission_locked(sc, emission_rgb, nmat);
    if (st) return st;
    return rebuild_scene_lights(sc, "spt_scene_set_emission");  // (the switch off: nothing)
}

namespace {
spt_status set_emission_locked(spt_scene_t* sc, const float* emission_rgb, uint32_t nmat) {
    spt_status qs = quiesce_scene(sc);  // queued renders may still read the old table
    if (qs) return qs;
    hfree(sc->emission);
    sc->nemit = 0;
    if (!emission_rgb || nmat == 0) return SPT_OK;  // no emitters
    bool any = false;
    for (uint32_t i = 0; i < 3 * nmat; i++) any |= emission_rgb[i] != 0.0f;
    if (!any) return SPT_OK;
    float* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, sizeof(float) * 3 * nmat));
    HIP_TRY(hipMemcpy(d, emission_rgb, sizeof(float) * 3 * nmat, hipMemcpyHostToDevice));
    sc->emission = d;
    sc->nemit = nmat;
    return SPT_OK;
}
}  // namespace

void spt_default_config(spt_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->build = SPT_BUILD_AUTO;
    c->bvh_width = 6;
    c->gpu_build_min_tris = 2000000;
    c->collapse = 0;
    c->ploc_radius = 16;
    c->stack_slack = 0;
    c->pipeline = SPT_PIPELINE_AUTO;
    c->fused_max_paths = kDefaultFusedMaxPaths;
    c->wavefront_paths = kDefaultWavefrontPaths;
    c->streams = 4;
    c->isect_refill_idle = 24;
    c->isect_static_share_q8 = 128;
    c->isect_chunk = kIsectChunk;
    c->isect_grid_q8 = 0;
    c->xcd_remap = 3;
    c->fused_refill_idle = 32;
    c->fused_static_share_q8 = 32;
    c->fused_grid_q8 = 256;
    c->plane_pad = 0;
    c->film_budget_bytes = 4ull << 30;
    c->public_persistent = 0;
    c->public_refill_idle = kRefillIdle;
    c->pack_groups = 1;
    c->pixel_block = 0;
    c->work_order = SPT_WORK_AUTO;
    c->queue_cache = SPT_QUEUE_CACHE_AUTO;
    c->drain_q8 = kDefaultDrainQ8;
    c->drain_grid_q8 = 0;
    c->drain_casts = kDefaultDrainCasts;
    c->fit_streams = 1;
    c->drain_refill_idle = 0;
    c->fit_paths = kDefaultFitPaths;
    c->sub_queues = 1;
    c->drain_sort = 0;
    c->lockstep_first = 3;
    c->fit_chunks = 1;
}

spt_status spt_scene_set_config(spt_scene sc, const spt_config* cfg) {
    if (!sc || !cfg) return fail(SPT_ERR_INVALID, "spt_scene_set_config: NULL argument");
    spt_status st = check_config(*cfg);
    if (st) return st;
    std::lock_guard<std::mutex> lk(sc->mu);
    // (stack_slack stays as built, below: the stack checked is the one the scene has)
    {
        DeviceGuard dg(sc->device);
        if ((st = check_stack_lds("spt_scene_set_config", sc->stack_depth, sc->cfg.bvh_width, sc->lights != nullptr || sc->sky != nullptr)))
            return st;
    }
    const spt_config old = sc->cfg;
    sc->cfg = *cfg;
    // the scene keeps the build it has
    sc->cfg.build = old.build; sc->cfg.bvh_width = old.bvh_width; sc->cfg.gpu_build_min_tris = old.gpu_build_min_tris;
    sc->cfg.collapse = old.collapse; sc->cfg.ploc_radius = old.ploc_radius; sc->cfg.stack_slack = old.stack_slack;
    sc->cfg.pack_groups = old.pack_groups;
    return SPT_OK;
}

spt_status spt_scene_get_config(spt_scene sc, spt_config* out) {
    if (!sc || !out) return fail(SPT_ERR_INVALID, "spt_scene_get_config: NULL argument");
    std::lock_guard<std::mutex> lk(sc->mu);
    *out = sc->cfg;
    return SPT_OK;
}

spt_status spt_scene_set_texture(spt_scene sc, uint32_t material, const float* rgb, uint32_t width, uint32_t height) {
    if (!sc) return fail(SPT_ERR_INVALID, "spt_scene_set_texture: NULL scene");
    DeviceGuard dg(sc->device);
    if (rgb && (width == 0 || height == 0)) return fail(SPT_ERR_INVALID, "spt_scene_set_texture: empty image");
    if (rgb && (uint64_t)width * height > (1ull << 26))
        return fail(SPT_ERR_LIMIT, "spt_scene_set_texture: %u x %u texels exceeds 2^26", width, height);
    if (material >= (1u << 20)) return fail(SPT_ERR_LIMIT, "spt_scene_set_texture: material %u >= 2^20", material);
    std::lock_guard<std::mutex> lk(sc->mu);
    spt_status qs = quiesce_scene(sc);  // queued renders may still read the old images (upload_textures frees them)
    if (qs) return qs;
    if (material >= sc->tex_img.size()) {
        sc->tex_img.resize(material + 1);
        sc->tex_w.resize(material + 1, 0);
        sc->tex_h.resize(material + 1, 0);
    }
    std::vector<float4>& img = sc->tex_img[material];
    img.clear();
    sc->tex_w[material] = sc->tex_h[material] = 0;
    if (rgb) {
        img.resize((size_t)width * height);
        for (size_t i = 0; i < img.size(); i++) img[i] = make_float4(rgb[i * 3], rgb[i * 3 + 1], rgb[i * 3 + 2], 0.0f);
        sc->tex_w[material] = width;
        sc->tex_h[material] = height;
    }
    return upload_textures(sc);
}

spt_status spt_scene_set_spheres(spt_scene sc, const float* center_radius, const int32_t* mat_id, uint32_t n) {
    if (!sc) return fail(SPT_ERR_INVALID, "spt_scene_set_spheres: NULL scene");
    DeviceGuard dg(sc->device);
    if (n > 256) return fail(SPT_ERR_LIMIT, "spt_scene_set_spheres: %u spheres (at most 256)", n);
    if (n && !center_radius) return fail(SPT_ERR_INVALID, "spt_scene_set_spheres: NULL spheres");
    for (uint32_t k = 0; k < n; k++) {
        const float* c = center_radius + (size_t)k * 4;
        if (!std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2]))
            return fail(SPT_ERR_INVALID, "spt_scene_set_spheres: sphere %u centre must be finite", k);
        if (!(c[3] > 0.0f) || !std::isfinite(c[3]))
            return fail(SPT_ERR_INVALID, "spt_scene_set_spheres: sphere %u radius must be finite and > 0", k);
    }
    std::lock_guard<std::mutex> lk(sc->mu);
    spt_status qs = quiesce_scene(sc);  // queued renders / calls may still read the old spheres
    if (qs) return qs;
    hfree(sc->spheres);
    hfree(sc->sph_mat);
    sc->nsph = 0;
    if (!n) return SPT_OK;
    std::vector<int32_t> mats(n, 0);
    if (mat_id) std::memcpy(mats.data(), mat_id, sizeof(int32_t) * n);
    spt_status us = upload(&sc->spheres, center_radius, sizeof(float4) * n);
    if (!us) us = upload(&sc->sph_mat, mats.data(), sizeof(int32_t) * n);
    if (us) return us;
    sc->nsph = n;
    return SPT_OK;
}

spt_status spt_scene_set_material_kinds(spt_scene sc, const uint32_t* kinds, uint32_t nmat) {
    if (!sc) return fail(SPT_ERR_INVALID, "spt_scene_set_material_kinds: NULL scene");
    DeviceGuard dg(sc->device);
    for (uint32_t i = 0; kinds && i < nmat; i++)
        if (kinds[i] > SPT_MAT_GLASS) return fail(SPT_ERR_INVALID, "spt_scene_set_material_kinds: kind %u of material %u", kinds[i], i);
    std::lock_guard<std::mutex> lk(sc->mu);
    spt_status qs = quiesce_scene(sc);  // queued renders may still read the old kinds
    if (qs) return qs;
    hfree(sc->mat_kind);
    sc->nkind = 0;
    bool any = false;
    for (uint32_t i = 0; kinds && i < nmat; i++) any = any || kinds[i] != SPT_MAT_DIFFUSE;
    if (!any) return SPT_OK;  // all diffuse: the default
    spt_status us = upload(&sc->mat_kind, kinds, sizeof(uint32_t) * nmat);
    if (us) return us;
    sc->nkind = nmat;
    return SPT_OK;
}

namespace {

// The sampling table of an n x n sky image on the device (sky_table.h; caller
// has made the device current).  *out: null for an empty table.  The sampler
// turns a map direction into the world with R^T, so R must be orthonormal:
// max |R R^T - I| <= 1e-4 in f64 (a rotation rounded to f32 stands near 1e-7).
spt_status build_sky(const char* what, const float* rgb, uint32_t n, const float* rot, float share, DeviceSky** out,
                     uint32_t* cells) {
    *out = nullptr;
    *cells = 0;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++) s += (double)rot[3 * r + k] * (double)rot[3 * c + k];
            if (!(std::fabs(s - (r == c ? 1.0 : 0.0)) <= 1e-4))
                return fail(SPT_ERR_INVALID, "%s: the map's rotation is not orthonormal ((R R^T)[%d][%d] = %g): sky "
                            "sampling turns map directions into the world with its transpose", what, r, c, s);
        }
    SkyTable t;
    sky_table_build(rgb, n, t);
    if (t.empty()) return SPT_OK;
    const size_t nn = (size_t)n * n;
    std::vector<unsigned char> buf(sizeof(DeviceSky) + sizeof(float) * (n + 2 * nn));
    DeviceSky h{};
    h.share = share;
    unsigned char* p = buf.data();
    std::memcpy(p, &h, sizeof(h));
    p += sizeof(h);
    std::memcpy(p, t.marg.data(), sizeof(float) * n);
    p += sizeof(float) * n;
    std::memcpy(p, t.cond.data(), sizeof(float) * nn);
    p += sizeof(float) * nn;
    std::memcpy(p, t.pdf.data(), sizeof(float) * nn);
    spt_status us = upload(out, buf.data(), buf.size());
    if (us) return us;
    *cells = (uint32_t)nn;
    return SPT_OK;
}

}  // namespace

spt_status spt_scene_set_envmap(spt_scene sc, const float* rgb, uint32_t n, const float* rotation) {
    static const char* what = "spt_scene_set_envmap";
    if (!sc) return fail(SPT_ERR_INVALID, "%s: NULL scene", what);
    // every refusal comes before the scene or the device is touched
    if (rgb) {
        if (n == 0) return fail(SPT_ERR_INVALID, "%s: n = 0 with an image", what);
        if (n > kEnvMapMaxN) return fail(SPT_ERR_LIMIT, "%s: n = %u (at most %u)", what, n, kEnvMapMaxN);
        for (int k = 0; rotation && k < 9; k++)
            if (!std::isfinite(rotation[k])) return fail(SPT_ERR_INVALID, "%s: rotation entry %d is not finite", what, k);
        for (size_t k = 0; k < (size_t)n * n * 3; k++)
            if (!std::isfinite(rgb[k]))
                return fail(SPT_ERR_INVALID, "%s: texel (%zu, %zu) channel %zu is not finite", what, (k / 3) % n,
                            (k / 3) / n, k % 3);
    }
    DeviceGuard dg(sc->device);
    std::lock_guard<std::mutex> lk(sc->mu);
    DeviceEnvMap* d_map = nullptr;
    float4* d_tex = nullptr;
    // sky sampling on: the table of the new map (a failure turns the switch off
    // and is returned once the map itself is set)
    DeviceSky* d_sky = nullptr;
    uint32_t cells = 0;
    spt_status sky_st = SPT_OK;
    static const float ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (rgb && sc->sky_sampling) {
        sky_st = build_sky(what, rgb, n, rotation ? rotation : ident, sc->sky_share, &d_sky, &cells);
        if (!sky_st && d_sky && (sky_st = check_stack_lds(what, sc->stack_depth, sc->cfg.bvh_width, true))) {
            hfree(d_sky);
            d_sky = nullptr;
            cells = 0;
        }
    }
    if (rgb) {
        // the image inside its gutter (DeviceEnvMap): gutter texels by the edge rule
        const int32_t ni = (int32_t)n;
        const size_t pitch = (size_t)n + 2;
        std::vector<float4> tex(pitch * pitch);
        for (int32_t j = -1; j <= ni; j++)
            for (int32_t i = -1; i <= ni; i++) {
                int32_t si = i, sj = j;
                envmap_wrap(ni, si, sj);
                const float* t = rgb + ((size_t)sj * n + (size_t)si) * 3;
                tex[(size_t)(j + 1) * pitch + (size_t)(i + 1)] = make_float4(t[0], t[1], t[2], 0.0f);
            }
        DeviceEnvMap h;
        h.n = n;
        std::memcpy(h.rot, rotation ? rotation : ident, sizeof(h.rot));
        spt_status us = upload(&d_tex, tex.data(), sizeof(float4) * tex.size());
        h.texels = d_tex;
        h.sky = d_sky;
        if (!us) us = upload(&d_map, &h, sizeof(h));
        if (us) {
            hfree(d_tex);
            hfree(d_map);
            hfree(d_sky);
            return us;
        }
    }
    spt_status qs = quiesce_scene(sc);  // queued renders may still read the old map
    if (qs) {
        hfree(d_tex);
        hfree(d_map);
        hfree(d_sky);
        return qs;
    }
    hfree(sc->envmap);
    hfree(sc->env_texels);
    hfree(sc->sky);
    sc->envmap = d_map;
    sc->env_texels = d_tex;
    sc->env_n = rgb ? n : 0;
    std::memcpy(sc->env_rot, rgb && rotation ? rotation : ident, sizeof(sc->env_rot));
    sc->sky = d_sky;  // (the map removed: the table is empty, the switch stays)
    sc->sky_cells = cells;
    if (sky_st) sc->sky_sampling = false;
    return sky_st;
}

spt_status spt_scene_set_sky_sampling(spt_scene sc, uint32_t on, float share) {
    static const char* what = "spt_scene_set_sky_sampling";
    if (!sc) return fail(SPT_ERR_INVALID, "%s: NULL scene", what);
    if (on > 1) return fail(SPT_ERR_INVALID, "%s: on = %u (0 or 1)", what, on);
    if (!(share > 0.0f && share < 1.0f))
        return fail(SPT_ERR_INVALID, "%s: share = %g (inside (0, 1))", what, (double)share);
    DeviceGuard dg(sc->device);
    std::lock_guard<std::mutex> lk(sc->mu);
    spt_status st = quiesce_scene(sc);  // queued renders may still read the old table
    if (st) return st;
    DeviceSky* d_sky = nullptr;
    DeviceEnvMap* d_map = nullptr;
    uint32_t cells = 0;
    if (sc->envmap) {
        const uint32_t n = sc->env_n;
        if (on) {
            // the texels back from the scene's own gutter array (the host keeps no copy)
            const size_t pitch = (size_t)n + 2;
            std::vector<float4> tex(pitch * pitch);
            HIP_TRY(hipMemcpy(tex.data(), sc->env_texels, sizeof(float4) * tex.size(), hipMemcpyDeviceToHost));
            std::vector<float> rgb((size_t)n * n * 3);
            for (uint32_t j = 0; j < n; j++)
                for (uint32_t i = 0; i < n; i++) {
                    const float4 t = tex[(size_t)(j + 1) * pitch + (i + 1)];
                    float* o = &rgb[((size_t)j * n + i) * 3];
                    o[0] = t.x; o[1] = t.y; o[2] = t.z;
                }
            if ((st = build_sky(what, rgb.data(), n, sc->env_rot, share, &d_sky, &cells))) return st;
            if (d_sky && (st = check_stack_lds(what, sc->stack_depth, sc->cfg.bvh_width, true))) {
                hfree(d_sky);
                return st;
            }
        }
        // the map's header again, with the new table (or none) behind it
        DeviceEnvMap h;
        h.n = n;
        std::memcpy(h.rot, sc->env_rot, sizeof(h.rot));
        h.texels = sc->env_texels;
        h.sky = d_sky;
        if ((st = upload(&d_map, &h, sizeof(h)))) {
            hfree(d_sky);
            return st;
        }
        hfree(sc->envmap);
        sc->envmap = d_map;
    }
    hfree(sc->sky);
    sc->sky = d_sky;
    sc->sky_cells = cells;
    sc->sky_sampling = on != 0;
    sc->sky_share = share;
    return SPT_OK;
}

spt_status spt_scene_get_sky_sampling(spt_scene sc, uint32_t* on, float* share, uint32_t* cells) {
    if (!sc) return fail(SPT_ERR_INVALID, "spt_scene_get_sky_sampling: NULL scene");
    std::lock_guard<std::mutex> lk(sc->mu);
    if (on) *on = sc->sky_sampling ? 1u : 0u;
    if (share) *share = sc->sky_share;
    if (cells) *cells = sc->sky_cells;
    return SPT_OK;
}

spt_status spt_scene_set_mis(spt_scene sc, uint32_t on) {
    static const char* what = "spt_scene_set_mis";
    if (!sc) return fail(SPT_ERR_INVALID, "%s: NULL scene", what);
    if (on > 1) return fail(SPT_ERR_INVALID, "%s: on = %u (0 or 1)", what, on);
    DeviceGuard dg(sc->device);
    std::lock_guard<std::mutex> lk(sc->mu);
    spt_status st = quiesce_scene(sc);  // as the other setters (a queued render took its DeviceScene by value)
    if (st) return st;
    sc->mis = on != 0;
    return SPT_OK;
}

spt_status spt_scene_get_mis(spt_scene sc, uint32_t* on) {
    if (!sc) return fail(SPT_ERR_INVALID, "spt_scene_get_mis: NULL scene");
    std::lock_guard<std::mutex> lk(sc->mu);
    if (on) *on = sc->mis ? 1u : 0u;
    return SPT_OK;
}

spt_status spt_sky_table_build(const float* rgb, uint32_t n, float* marginal, float* conditional, float* density,
                               uint32_t* cells_out) {
    static const char* what = "spt_sky_table_build";
    if (!cells_out) return fail(SPT_ERR_INVALID, "%s: NULL cells_out", what);
    if (!rgb) return fail(SPT_ERR_INVALID, "%s: NULL image", what);
    if (n == 0) return fail(SPT_ERR_INVALID, "%s: n = 0", what);
    if (n > kSkyMaxN) return fail(SPT_ERR_LIMIT, "%s: n = %u (at most %u)", what, n, kSkyMaxN);
    SkyTable t;
    sky_table_build(rgb, n, t);
    *cells_out = t.empty() ? 0u : n * n;
    if (t.empty()) return SPT_OK;
    if (marginal) std::memcpy(marginal, t.marg.data(), sizeof(float) * n);
    if (conditional) std::memcpy(conditional, t.cond.data(), sizeof(float) * t.cond.size());
    if (density) std::memcpy(density, t.pdf.data(), sizeof(float) * t.pdf.size());
    return SPT_OK;
}

namespace {

// spt_scene_update_geometry[_device] once the arrays are on the device
// (caller holds sc->mu and has made the scene's device current).
spt_status update_geometry_locked(spt_scene_t* sc, const RefitMeshIn& m, bool validate, hipStream_t s, double t0) {
    static const char* what = "spt_scene_update_geometry";
    spt_status qs = quiesce_scene(sc);  // queued renders / calls see the geometry they were queued with
    if (qs) return qs;
    RefitScene rs{};
    rs.nodes = sc->nodes8 ? sc->nodes8 : (uint4*)sc->nodes;
    rs.fmt = sc->nodes8 ? (sc->node6 ? kRefitFmt6 : kRefitFmt8) : kRefitFmt2;
    rs.group_shift = sc->group_shift;
    rs.node_bytes = sc->node_bytes;
    rs.tris = sc->tris;
    rs.snrm = sc->snrm;
    rs.orig2slot = sc->orig2slot;
    rs.ntri = (uint32_t)sc->ntri;
    if (validate) {  // before anything is written
        if (!sc->refit_bad) HIP_TRY(hipMalloc((void**)&sc->refit_bad, sizeof(uint32_t)));
        uint32_t bad = 0;
        HIP_TRY(launch_refit_validate(rs, m, sc->refit_bad, s));
        HIP_TRY(hipMemcpyAsync(&bad, sc->refit_bad, sizeof(bad), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (bad)
            return fail(SPT_ERR_INVALID, "%s: %u position / normal indices out of range [0,%llu) / [-1,%llu)", what,
                        bad, (unsigned long long)m.nvert, (unsigned long long)m.nnrm);
    }
    if (!sc->refit.built) {
        const char* why = nullptr;
        const hipError_t e = refit_plan_build(rs, sc->stats.nodes, s, &sc->refit, &why);
        if (why) return fail(SPT_ERR_HIP, "%s: refit plan: %s (%llu nodes expected)", what, why,
                             (unsigned long long)sc->stats.nodes);
        if (e) return fail(e == hipErrorOutOfMemory ? SPT_ERR_OOM : SPT_ERR_HIP, "%s: refit plan: %s", what,
                           hipGetErrorString(e));
    }
    RefitPlan& p = sc->refit;
    double area = 0.0;
    float ms = 0.0f;
    sc->geom_epoch++;  // the boxes move from here on, whatever becomes of the call
    HIP_TRY(hipEventRecord(p.ev0, s));
    HIP_TRY(launch_refit_update(rs, &m, p, true, s));
    HIP_TRY(hipEventRecord(p.ev1, s));
    HIP_TRY(hipMemcpyAsync(&area, p.area, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&ms, p.ev0, p.ev1));
    spt_refit_stats& st = sc->refit_stats;
    st.updates++;
    st.nodes = p.nodes;
    st.tris = sc->ntri;
    st.levels = p.levels;
    st.plan_bytes = p.bytes;
    st.plan_ms = p.plan_ms;
    st.refit_ms = ms;
    st.area_built = p.area_built;
    st.area_now = area;
    st.update_ms = now_ms() - t0;
    return rebuild_scene_lights(sc, what);  // the lights moved with the rest (the switch off: nothing)
}

spt_status update_geometry_args(spt_scene sc, const int32_t* pos_tri, const float* pos, uint64_t ntri,
                                const int32_t* nrm_tri, const float* nrm, uint64_t nnrm) {
    static const char* what = "spt_scene_update_geometry";
    if (!sc) return fail(SPT_ERR_INVALID, "%s: NULL scene", what);
    if (ntri != sc->ntri)
        return fail(SPT_ERR_INVALID, "%s: %llu triangles given, the scene has %llu (the topology is fixed)", what,
                    (unsigned long long)ntri, (unsigned long long)sc->ntri);
    if (ntri > 0 && (!pos_tri || !pos)) return fail(SPT_ERR_INVALID, "%s: NULL positions", what);
    if (nrm_tri && !nrm && nnrm) return fail(SPT_ERR_INVALID, "%s: normal indices without normals", what);
    return SPT_OK;
}

}  // namespace

spt_status spt_scene_update_geometry(spt_scene sc, const int32_t* pos_tri, const float* pos, uint64_t nvert,
                                     uint64_t ntri, const int32_t* nrm_tri, const float* nrm, uint64_t nnrm) {
    static const char* what = "spt_scene_update_geometry";
    const double t0 = now_ms();
    spt_status st = update_geometry_args(sc, pos_tri, pos, ntri, nrm_tri, nrm, nnrm);
    if (st || ntri == 0) return st;
    for (uint64_t t = 0; t < ntri; t++)
        for (int k = 0; k < 3; k++) {
            const int64_t pi = pos_tri[t * 3 + k];
            if (pi < 0 || (uint64_t)pi >= nvert)
                return fail(SPT_ERR_INVALID, "%s: triangle %llu position index %lld out of range [0,%llu)", what,
                            (unsigned long long)t, (long long)pi, (unsigned long long)nvert);
            const int64_t ni = nrm_tri ? nrm_tri[t * 3 + k] : -1;
            if (ni < -1 || (ni >= 0 && (uint64_t)ni >= nnrm))
                return fail(SPT_ERR_INVALID, "%s: triangle %llu normal index %lld out of range", what,
                            (unsigned long long)t, (long long)ni);
        }
    DeviceGuard dg(sc->device);
    struct Raw {
        int32_t *pt = nullptr, *nt = nullptr;
        float *p = nullptr, *n = nullptr;
        ~Raw() { hfree(pt); hfree(nt); hfree(p); hfree(n); }
    } raw;
    if (!st) st = upload(&raw.pt, pos_tri, ntri * 3 * sizeof(int32_t));
    if (!st) st = upload(&raw.p, pos, nvert * 3 * sizeof(float));
    if (!st && nrm_tri) st = upload(&raw.nt, nrm_tri, ntri * 3 * sizeof(int32_t));
    if (!st && nrm_tri) st = upload(&raw.n, nrm, nnrm * 3 * sizeof(float));
    if (st) return st;
    const RefitMeshIn m{raw.pt, raw.p, raw.nt, raw.n, nvert, nnrm};
    std::lock_guard<std::mutex> lk(sc->mu);
    return update_geometry_locked(sc, m, false, nullptr, t0);  // the null stream; the call is synchronous
}

spt_status spt_scene_update_geometry_device(spt_scene sc, const int32_t* pos_tri, const float* pos, uint64_t nvert,
                                            uint64_t ntri, const int32_t* nrm_tri, const float* nrm, uint64_t nnrm,
                                            void* stream) {
    const double t0 = now_ms();
    const spt_status st = update_geometry_args(sc, pos_tri, pos, ntri, nrm_tri, nrm, nnrm);
    if (st || ntri == 0) return st;
    DeviceGuard dg(sc->device);
    const RefitMeshIn m{pos_tri, pos, nrm_tri, nrm, nvert, nnrm};
    std::lock_guard<std::mutex> lk(sc->mu);
    return update_geometry_locked(sc, m, true, (hipStream_t)stream, t0);
}

spt_status spt_scene_get_refit_stats(spt_scene sc, spt_refit_stats* out) {
    if (!sc || !out) return fail(SPT_ERR_INVALID, "spt_scene_get_refit_stats: NULL argument");
    std::lock_guard<std::mutex> lk(sc->mu);
    *out = sc->refit_stats;
    return SPT_OK;
}

spt_status spt_scene_get_stats(spt_scene sc, spt_scene_stats* out) {
    if (!sc || !out) return fail(SPT_ERR_INVALID, "spt_scene_get_stats: NULL argument");
    *out = sc->stats;
    return SPT_OK;
}

spt_status spt_bvh_build_stats(const float* tv, uint64_t ntri, const spt_config* cfg_in, spt_scene_stats* out) {
    if (!out || (ntri > 0 && !tv)) return fail(SPT_ERR_INVALID, "spt_bvh_build_stats: NULL argument");
    if (ntri >= kMaxTriangles) return fail(SPT_ERR_LIMIT, "spt_bvh_build_stats: %llu triangles exceeds 2^28",
                                           (unsigned long long)ntri);
    spt_config cfg;
    if (cfg_in) cfg = *cfg_in;
    else spt_default_config(&cfg);
    spt_status st = check_config(cfg);
    if (st) return st;
    spt_scene_stats ss{};
    const double t0 = now_ms();
    if (cfg.bvh_width != 2) {
        const Bvh8BuildResult b = build_bvh8(tv, ntri, cfg.collapse == 1, (int)cfg.bvh_width);
        ss.nodes = b.nodes.size() / 20; ss.leaves = b.leaves; ss.max_depth = b.depth; ss.max_leaf = 3;
        ss.sah_cost = b.sah_cost;
        if (b.slot2tri.size() != ntri) return fail(SPT_ERR_HIP, "spt_bvh_build_stats: BVH8 lost triangles");
    } else {
        const BvhBuildResult b = build_bvh(tv, ntri);
        ss.nodes = b.nodes.size() / 16; ss.leaves = b.leaves; ss.max_depth = b.max_depth; ss.max_leaf = b.max_leaf;
        ss.sah_cost = b.sah_cost;
        if (b.slot2tri.size() != ntri) return fail(SPT_ERR_HIP, "spt_bvh_build_stats: BVH2 lost triangles");
    }
    ss.ntri = ntri;
    ss.bvh_width = cfg.bvh_width;
    ss.builder = SPT_BUILD_HOST_SAH;
    ss.build_ms = now_ms() - t0;
    *out = ss;
    return SPT_OK;
}

spt_status spt_scene_destroy(spt_scene sc) {
    if (!sc) return SPT_OK;
    DeviceGuard dg(sc->device);
    {
        std::lock_guard<std::mutex> lk(sc->mu);
        (void)quiesce_scene(sc);  // nothing queued may still read what is freed
    }
    sc->release();
    delete sc;
    return SPT_OK;
}

spt_status spt_intersect(spt_scene sc, const spt_rays* rays, const uint8_t* mask, uint32_t mask_size,
                         const spt_hits* hits, uint32_t n, int32_t do_closest, void* stream) {
    if (!sc || !rays || !hits) return fail(SPT_ERR_INVALID, "spt_intersect: NULL argument");
    if (n == 0) return SPT_OK;
    if (!rays->ox || !rays->oy || !rays->oz || !rays->dx || !rays->dy || !rays->dz)
        return fail(SPT_ERR_INVALID, "spt_intersect: NULL ray plane");
    if (!hits->tri_id || !hits->t || !hits->u || !hits->v) return fail(SPT_ERR_INVALID, "spt_intersect: NULL hit plane");
    if (mask && mask_size != 1 && mask_size != n)
        return fail(SPT_ERR_INVALID, "spt_intersect: mask_size %u must be 1 or n=%u", mask_size, n);
    IsectPublicArgs a;
    a.ox = rays->ox; a.oy = rays->oy; a.oz = rays->oz;
    a.dx = rays->dx; a.dy = rays->dy; a.dz = rays->dz;
    a.tmin = rays->tmin; a.tmax = rays->tmax;
    a.mask = mask; a.mask_size = mask_size;
    a.tri_id = hits->tri_id; a.t = hits->t; a.u = hits->u; a.v = hits->v;
    a.n = n;
    a.closest = do_closest;
    // a consistent snapshot of the device arrays and knobs, launched and
    // recorded under the mutex: a scene mutator waits for this launch before it
    // frees an array the snapshot holds (quiesce_scene)
    DeviceGuard dg(sc->device);
    std::lock_guard<std::mutex> lock(sc->mu);
    a.sc = sc->dev();
    a.refill_idle = sc->cfg.public_refill_idle;
    a.persistent = sc->cfg.public_persistent;
    HIP_TRY(launch_isect_public(a, (hipStream_t)stream));
    return record_public_use(sc, (hipStream_t)stream);
}

spt_status spt_hit_info_compute(spt_scene sc, const spt_rays* rays, const spt_hits* hits, const uint8_t* mask,
                                uint32_t mask_size, uint32_t n, const spt_hit_info* out, void* stream) {
    if (!sc || !rays || !hits || !out) return fail(SPT_ERR_INVALID, "spt_hit_info_compute: NULL argument");
    if (n == 0) return SPT_OK;
    if (!hits->tri_id || !hits->t || !hits->u || !hits->v)
        return fail(SPT_ERR_INVALID, "spt_hit_info_compute: NULL hit plane");
    // the rays are read for the position (o + t d), and on a scene with
    // spheres for their normals too (the normal of a sphere hit is (p - c) / r)
    const bool no_rays = !rays->ox || !rays->oy || !rays->oz || !rays->dx || !rays->dy || !rays->dz;
    if ((out->px || out->py || out->pz) && no_rays)
        return fail(SPT_ERR_INVALID, "spt_hit_info_compute: NULL ray plane (needed for the position)");
    if (no_rays && sc->nsph > 0 && (out->gnx || out->gny || out->gnz || out->snx || out->sny || out->snz))
        return fail(SPT_ERR_INVALID, "spt_hit_info_compute: NULL ray plane (a sphere hit's normal needs the hit point)");
    if (mask && mask_size != 1 && mask_size != n)
        return fail(SPT_ERR_INVALID, "spt_hit_info_compute: mask_size %u must be 1 or n=%u", mask_size, n);
    if (sc->ntri == 0 && sc->nsph == 0) return SPT_OK;
    HitInfoArgs a;
    DeviceGuard dg(sc->device);
    std::lock_guard<std::mutex> lock(sc->mu);  // as spt_intersect: launched and recorded under the mutex
    a.sc = sc->dev();
    a.ox = rays->ox; a.oy = rays->oy; a.oz = rays->oz;
    a.dx = rays->dx; a.dy = rays->dy; a.dz = rays->dz;
    a.tri_id = hits->tri_id; a.t = hits->t; a.u = hits->u; a.v = hits->v;
    a.mask = mask; a.mask_size = mask_size; a.n = n;
    a.px = out->px; a.py = out->py; a.pz = out->pz;
    a.gnx = out->gnx; a.gny = out->gny; a.gnz = out->gnz;
    a.snx = out->snx; a.sny = out->sny; a.snz = out->snz;
    a.tcu = out->tcu; a.tcv = out->tcv;
    a.mat_id = out->mat_id;
    a.ntri = sc->ntri;
    HIP_TRY(launch_hit_info(a, (hipStream_t)stream));
    return record_public_use(sc, (hipStream_t)stream);
}

void spt_default_denoise_params(spt_denoise_params* p) {
    if (!p) return;
    p->width = p->height = 0;
    p->iterations = 5;
    p->sigma_color = 0.6f;
    p->sigma_normal = 0.5f;
    p->sigma_albedo = 0.2f;
    p->sigma_depth = 0.1f;
}

size_t spt_denoise_scratch_bytes(uint32_t width, uint32_t height) {
    return (size_t)2 * 3 * sizeof(float) * (size_t)width * (size_t)height;
}

spt_status spt_denoise(const spt_denoise_params* pp, const float* color, const spt_aov* guides, float* out,
                       void* scratch, void* stream_) {
    if (!pp) return fail(SPT_ERR_INVALID, "spt_denoise: NULL params");
    const spt_denoise_params& p = *pp;
    if (p.width == 0 || p.height == 0) return fail(SPT_ERR_INVALID, "spt_denoise: width/height must be > 0");
    if (p.iterations > 8) return fail(SPT_ERR_INVALID, "spt_denoise: iterations %u > 8", p.iterations);
    if (!color || !out) return fail(SPT_ERR_INVALID, "spt_denoise: NULL color / out");
    if (color == out) return fail(SPT_ERR_INVALID, "spt_denoise: out must not alias color");
    if (p.iterations > 0 && !scratch) return fail(SPT_ERR_INVALID, "spt_denoise: NULL scratch");
    if ((uint64_t)p.width * p.height >= (1ull << 31)) return fail(SPT_ERR_LIMIT, "spt_denoise: image too large");
    const hipStream_t stream = (hipStream_t)stream_;
    const size_t P = (size_t)p.width * p.height;
    if (p.iterations == 0) {
        HIP_TRY(hipMemcpyAsync(out, color, 3 * P * sizeof(float), hipMemcpyDeviceToDevice, stream));
        return SPT_OK;
    }
    DenoiseArgs a{};
    a.width = p.width;
    a.height = p.height;
    // 1 / sigma^2, finite (the centre tap's 0 x inf would be NaN); 0: the term is off
    const auto inv_sq = [](float sigma) { return sigma > 0.0f ? std::min(1.0f / (sigma * sigma), 3.0e38f) : 0.0f; };
    if (guides && guides->normal_x && guides->normal_y && guides->normal_z) {
        a.normal_x = guides->normal_x; a.normal_y = guides->normal_y; a.normal_z = guides->normal_z;
        a.inv_normal = inv_sq(p.sigma_normal);
    }
    if (guides && guides->albedo_r && guides->albedo_g && guides->albedo_b) {
        a.albedo_r = guides->albedo_r; a.albedo_g = guides->albedo_g; a.albedo_b = guides->albedo_b;
        a.inv_albedo = inv_sq(p.sigma_albedo);
    }
    if (guides && guides->depth) {
        a.depth = guides->depth;
        a.inv_depth = inv_sq(p.sigma_depth);
    }
    float* const ping[2] = {(float*)scratch, (float*)scratch + 3 * P};
    const float* src = color;
    for (uint32_t i = 0; i < p.iterations; i++) {
        a.src = src;
        a.dst = i + 1 == p.iterations ? out : ping[i & 1u];
        a.step = 1u << i;
        a.inv_color = inv_sq(p.sigma_color / (float)(1u << i));  // sigma_color 2^-i
        HIP_TRY(launch_denoise(a, stream));
        src = a.dst;
    }
    return SPT_OK;
}

void spt_default_denoise_var_params(spt_denoise_var_params* p) {
    if (!p) return;
    p->width = p->height = 0;
    p->iterations = 5;
    p->sigma_variance = 4.0f;
    p->sigma_normal = 0.5f;
    p->sigma_albedo = 0.2f;
    p->sigma_depth = 0.1f;
}

size_t spt_denoise_var_scratch_bytes(uint32_t width, uint32_t height) {
    return (size_t)2 * (3 + 1) * sizeof(float) * (size_t)width * (size_t)height;
}

spt_status spt_denoise_var(const spt_denoise_var_params* pp, const float* color, const float* variance,
                           const spt_aov* guides, float* out, float* variance_out, void* scratch, void* stream_) {
    if (!pp) return fail(SPT_ERR_INVALID, "spt_denoise_var: NULL params");
    const spt_denoise_var_params& p = *pp;
    if (p.width == 0 || p.height == 0) return fail(SPT_ERR_INVALID, "spt_denoise_var: width/height must be > 0");
    if (p.iterations > 8) return fail(SPT_ERR_INVALID, "spt_denoise_var: iterations %u > 8", p.iterations);
    if (!color || !out || !variance) return fail(SPT_ERR_INVALID, "spt_denoise_var: NULL color / variance / out");
    if (color == out) return fail(SPT_ERR_INVALID, "spt_denoise_var: out must not alias color");
    if (variance == out || (variance_out && (variance_out == out || variance_out == color || variance_out == variance)))
        return fail(SPT_ERR_INVALID, "spt_denoise_var: out / variance_out must not alias an input or each other");
    if (p.iterations > 0 && !scratch) return fail(SPT_ERR_INVALID, "spt_denoise_var: NULL scratch");
    if ((uint64_t)p.width * p.height >= (1ull << 31)) return fail(SPT_ERR_LIMIT, "spt_denoise_var: image too large");
    const hipStream_t stream = (hipStream_t)stream_;
    const size_t P = (size_t)p.width * p.height;
    if (p.iterations == 0) {
        HIP_TRY(hipMemcpyAsync(out, color, 3 * P * sizeof(float), hipMemcpyDeviceToDevice, stream));
        if (variance_out) HIP_TRY(launch_denoise_var_init(variance, variance_out, (uint32_t)P, stream));
        return SPT_OK;
    }
    DenoiseVarArgs a{};
    a.width = p.width;
    a.height = p.height;
    const auto inv_sq = [](float sigma) { return sigma > 0.0f ? std::min(1.0f / (sigma * sigma), 3.0e38f) : 0.0f; };
    a.sv2 = p.sigma_variance > 0.0f ? std::min(p.sigma_variance * p.sigma_variance, 3.0e38f) : 0.0f;
    if (guides && guides->normal_x && guides->normal_y && guides->normal_z) {
        a.normal_x = guides->normal_x; a.normal_y = guides->normal_y; a.normal_z = guides->normal_z;
        a.inv_normal = inv_sq(p.sigma_normal);
    }
    if (guides && guides->albedo_r && guides->albedo_g && guides->albedo_b) {
        a.albedo_r = guides->albedo_r; a.albedo_g = guides->albedo_g; a.albedo_b = guides->albedo_b;
        a.inv_albedo = inv_sq(p.sigma_albedo);
    }
    if (guides && guides->depth) {
        a.depth = guides->depth;
        a.inv_depth = inv_sq(p.sigma_depth);
    }
    // two images of 3 colour planes + 1 variance plane; v_0 starts in the second
    // image's variance plane, which iteration 1 is the first to overwrite
    float* const ping[2] = {(float*)scratch, (float*)scratch + 4 * P};
    HIP_TRY(launch_denoise_var_init(variance, ping[1] + 3 * P, (uint32_t)P, stream));
    const float* src = color;
    const float* vsrc = ping[1] + 3 * P;
    for (uint32_t i = 0; i < p.iterations; i++) {
        const bool last = i + 1 == p.iterations;
        a.src = src;
        a.vsrc = vsrc;
        a.dst = last ? out : ping[i & 1u];
        a.vdst = last ? variance_out : ping[i & 1u] + 3 * P;
        a.step = 1u << i;
        HIP_TRY(launch_denoise_var(a, stream));
        src = a.dst;
        vsrc = a.vdst;
    }
    return SPT_OK;
}

void spt_default_adapt_params(spt_adapt_params* p) {
    if (!p) return;
    // chosen on tests/adaptive_ref.py's schedules
    p->min_spp = 8;
    p->max_spp = 1024;
    p->tolerance = 0.05f;
    p->floor = 0.03f;
    p->reserved[0] = p->reserved[1] = 0;
}

size_t spt_adapt_select_scratch_bytes(uint32_t npix) {
    const size_t waves = ((size_t)npix + 63) / 64, blocks = ((size_t)npix + kAdaptBlock - 1) / kAdaptBlock;
    return (8 * waves + 4 * (blocks + 1) + 15) & ~(size_t)15;
}

spt_status spt_adapt_select(const spt_adapt_params* pp, uint32_t npix, uint32_t sample_base, const float* sum,
                            const float* sum_sq, const uint32_t* count, uint32_t* list, uint32_t* n_active,
                            void* scratch, void* stream_) {
    if (!pp || !list || !n_active || !scratch)
        return fail(SPT_ERR_INVALID, "spt_adapt_select: NULL params / list / n_active / scratch");
    const spt_adapt_params& p = *pp;
    if (sample_base > 0 && (!sum || !sum_sq || !count))
        return fail(SPT_ERR_INVALID, "spt_adapt_select: NULL sum / sum_sq / count with sample_base > 0");
    if (p.reserved[0] != 0 || p.reserved[1] != 0) return fail(SPT_ERR_INVALID, "spt_adapt_select: reserved must be 0");
    if (p.min_spp > p.max_spp)
        return fail(SPT_ERR_INVALID, "spt_adapt_select: min_spp %u > max_spp %u", p.min_spp, p.max_spp);
    if (!(p.tolerance >= 0.0f) || !std::isfinite(p.tolerance) || !(p.floor >= 0.0f) || !std::isfinite(p.floor))
        return fail(SPT_ERR_INVALID, "spt_adapt_select: tolerance and floor must be finite and >= 0");
    if (((uintptr_t)list | (uintptr_t)scratch | (uintptr_t)sum | (uintptr_t)sum_sq | (uintptr_t)count) & 3u)
        return fail(SPT_ERR_INVALID, "spt_adapt_select: buffers must be 4-byte aligned");
    if (sample_base >= (1u << 24)) return fail(SPT_ERR_LIMIT, "spt_adapt_select: sample_base must be < 2^24");
    if (npix >= (1u << 31)) return fail(SPT_ERR_LIMIT, "spt_adapt_select: too many pixels");
    *n_active = 0;
    if (npix == 0) return SPT_OK;
    const hipStream_t stream = (hipStream_t)stream_;
    const uint32_t blocks = (npix + kAdaptBlock - 1) / kAdaptBlock;
    AdaptArgs a{};
    a.sum = sum; a.sum_sq = sum_sq; a.count = count;
    a.list = list;
    a.masks = (uint32_t*)scratch;
    a.totals = a.masks + 2 * (size_t)((npix + 63u) / 64u);
    a.npix = npix; a.n = sample_base;
    a.min_spp = p.min_spp; a.max_spp = p.max_spp;
    a.tolerance = p.tolerance; a.floor = p.floor;
    HIP_TRY(launch_adapt_select(a, stream));
    if (sample_base == 0) {
        HIP_TRY(hipStreamSynchronize(stream));
        *n_active = npix;
        return SPT_OK;
    }
    uint32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, a.totals + blocks, sizeof(n), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *n_active = n;
    return SPT_OK;
}

}  // extern "C"
