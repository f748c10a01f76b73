// scene_state.h — the scene behind the C ABI's handle and the helpers its
// three host units share: capi.cpp (scene creation, setters, refit, intersect,
// denoisers), render.cpp (the render loop and its working memory) and
// scene_cache.cpp (spt_scene_save / spt_scene_load).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <mutex>
#include <vector>

#include "../../include/spt.h"
#include "host_error.h"
#include "spt_internal.h"

namespace spt {

// Formats the message into spt_last_error() and returns code.
template <typename... Args>
spt_status fail(spt_status code, const char* fmt, Args... args) {
    return spt_set_error(code, fmt, args...);
}

#define HIP_TRY(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorOutOfMemory ? SPT_ERR_OOM : SPT_ERR_HIP, "HIP call '%s' failed: %s (%s:%d)", \
                        #call, hipGetErrorString(e_), __FILE__, __LINE__);                         \
    } while (0)

template <typename T>
void hfree(T*& p) {
    if (p) (void)hipFree((void*)p);
    p = nullptr;
}

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The renders' working memory of a scene (render.cpp): working sets, jump
// tables and the ring of queued renders.
struct Workspace;
Workspace* workspace_new();
void workspace_release(Workspace& ws);  // frees what it holds; tickets stay unique over the scene's life
void workspace_delete(Workspace* ws);

// Before a scene mutator frees or replaces a device array that queued work may
// still read (materials, textures, spheres, kinds): wait for every render of
// both working sets (free_ev) and for the last public call on every stream
// that made one (spt_intersect / spt_hit_info_compute, record_public_use).  The
// caller holds the scene mutex, so nothing new is queued meanwhile.
struct PublicUse {
    hipStream_t stream;
    hipEvent_t ev;
};

}  // namespace spt

struct spt_scene_t {
    int device = 0;
    spt_config cfg{};
    std::mutex mu;  // one workspace per scene: spt_render / spt_scene_set_config serialise here
    uint64_t ntri = 0;
    float4* nodes = nullptr;
    uint4* nodes8 = nullptr;
    uint32_t node6 = 0;  // nodes8 holds the 64-B six-wide nodes (spt_config.bvh_width 6)
    uint32_t group_shift = 3;  // 0: packed child groups, 3: aligned groups of eight slots
    float4* tris = nullptr;
    float4* snrm = nullptr;
    float* tc = nullptr;
    int32_t* orig2slot = nullptr;
    float* albedo = nullptr;
    uint32_t nmat = 1;
    float* emission = nullptr;
    uint32_t nemit = 0;
    bool albedo_unit = true;  // every albedo entry is exactly 1 (the reference's case)
    // per-material reflectance images (spt_scene_set_texture): host copies and
    // the device arrays rebuilt from them
    std::vector<std::vector<float4>> tex_img;
    std::vector<uint32_t> tex_w, tex_h;
    uint4* tex_info = nullptr;
    float4* texels = nullptr;
    uint32_t ntex = 0;      // entries of tex_info (0: no images)
    float4* spheres = nullptr;   // smallpt's analytic spheres (spt_scene_set_spheres)
    int32_t* sph_mat = nullptr;
    uint32_t nsph = 0;
    uint32_t* mat_kind = nullptr;  // SPT_MAT_* per material (spt_scene_set_material_kinds)
    uint32_t nkind = 0;
    // the sky image (spt_scene_set_envmap): the device struct and the texels behind it
    spt::DeviceEnvMap* envmap = nullptr;
    float4* env_texels = nullptr;
    uint32_t env_n = 0;  // the map's size and rotation as set (the sky table is built from them)
    float env_rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    // sky sampling (spt_scene_set_sky_sampling): the switch, the share, and the
    // table behind envmap->sky (null: off, no map, or an empty table)
    bool sky_sampling = false;
    float sky_share = 0.5f;
    spt::DeviceSky* sky = nullptr;
    uint32_t sky_cells = 0;
    // light sampling (spt_scene_set_light_sampling): the switch, and the table
    // built from the scene's emissive triangles (null: off, or an empty table)
    bool light_sampling = false;
    spt::DeviceLights* lights = nullptr;
    uint32_t nlights = 0;
    // MIS (spt_scene_set_mis): the switch alone; it acts where one of the two tables above is non-empty
    bool mis = false;
    uint64_t node_bytes = 0;  // bytes behind nodes / nodes8 (spt_scene_save)
    // counts the geometry's changes under the same device arrays (spt_scene_update_geometry's
    // refit): what was derived from the boxes — the renders' camera entry tables — is keyed on it
    uint64_t geom_epoch = 0;
    uint32_t stack_depth = 1;
    spt_scene_stats stats{};
    spt::Workspace& ws = *spt::workspace_new();
    std::vector<spt::PublicUse> pub;  // streams of public calls, with an event after the last one (quiesce)
    // spt_scene_update_geometry: the plan is built by the first update
    spt::RefitPlan refit;
    uint32_t* refit_bad = nullptr;  // the device validation's counter
    spt_refit_stats refit_stats{};

    ~spt_scene_t() { spt::workspace_delete(&ws); }

    spt::DeviceScene dev() const {
        spt::DeviceScene d;
        d.nodes = nodes; d.nodes8 = nodes8; d.node6 = node6; d.group_shift = group_shift; d.tris = tris; d.snrm = snrm; d.tc = tc; d.orig2slot = orig2slot;
        d.albedo = albedo; d.nmat = nmat; d.emission = emission; d.nemit = nemit; d.stack_depth = stack_depth; d.empty = ntri == 0;
        d.tex_info = tex_info; d.ntex = ntex; d.texels = texels;
        d.spheres = spheres; d.sph_mat = sph_mat; d.nsph = nsph;
        d.mat_kind = mat_kind; d.nkind = nkind;
        d.envmap = envmap;
        d.sky = sky != nullptr;
        d.lights = lights;
        d.mis = mis ? 1u : 0u;
        return d;
    }
    void release() {
        for (auto& u : pub) (void)hipEventDestroy(u.ev);
        pub.clear();
        spt::workspace_release(ws);
        spt::hfree(nodes); spt::hfree(nodes8); spt::hfree(emission); spt::hfree(tris); spt::hfree(snrm); spt::hfree(tc); spt::hfree(orig2slot); spt::hfree(albedo);
        spt::hfree(tex_info); spt::hfree(texels); spt::hfree(spheres); spt::hfree(sph_mat); spt::hfree(mat_kind);
        spt::hfree(envmap); spt::hfree(env_texels); spt::hfree(sky);
        spt::hfree(lights);
        spt::refit_plan_release(refit);
        spt::hfree(refit_bad);
    }
};

namespace spt {

// Makes the scene's device current for one API call and restores the
// caller's afterwards: a scene's arrays, streams and events live on the device
// it was committed on, whatever device the calling thread has current (the C++
// host destroys every rank's scene from one thread).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// (see PublicUse) caller holds sc->mu  [render.cpp]
spt_status quiesce_scene(spt_scene_t* sc);
// After a public call's launch on `s` (caller holds sc->mu).  At most 64
// streams are tracked: beyond that the list is drained and restarted.  [capi.cpp]
spt_status record_public_use(spt_scene_t* sc, hipStream_t s);

// [capi.cpp]
spt_status ensure_device();
spt_status upload_textures(spt_scene_t* sc);
// Range checks of spt_scene_set_config / spt_scene_create_cfg.
spt_status check_config(const spt_config& c);
// Refuses a stack that does not fit the current device's LDS per workgroup.
// nee: with the light-sampling kernels' larger park (launch_fused_t).
spt_status check_stack_lds(const char* what, uint32_t stack_depth, uint32_t width, bool nee = false);

template <typename T>
spt_status upload(T** dst, const void* src, size_t bytes) {
    *dst = nullptr;
    if (bytes == 0) return SPT_OK;
    HIP_TRY(hipMalloc((void**)dst, bytes));
    HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return SPT_OK;
}

}  // namespace spt
