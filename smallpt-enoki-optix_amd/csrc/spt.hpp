// spt.hpp — C++ host wrapper over include/spt.h keeping the reference's
// exception convention (OPTIX_CHECK / CUDA_CHECK throw std::runtime_error,
// optix_backend.h:25-66) and its Scene / backend call shape
// (Scene::add_triangle_mesh / commit / intersect, main.cpp:286-352).
#pragma once
#include <hip/hip_runtime_api.h>

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/spt.h"

namespace spt {

inline void check(spt_status s, const char* what) {
    if (s != SPT_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(s) + "): " + spt_last_error());
}

inline bool ends_with(const std::string& s, const char* suffix) {
    const size_t n = std::char_traits<char>::length(suffix);
    return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

// An OBJ (main.cpp:141-251) or a pbrt-v3 scene (the pbrt-parser path), by extension.
struct Mesh {
    spt_mesh m{};
    spt_pbrt_info pbrt{};
    explicit Mesh(const std::string& path) {
        if (ends_with(path, ".pbrt")) check(spt_pbrt_load(path.c_str(), &m, &pbrt), "spt_pbrt_load");
        else check(spt_obj_load(path.c_str(), &m), "spt_obj_load");
    }
    ~Mesh() { spt_mesh_free(&m); }
    Mesh(const Mesh&) = delete;
    Mesh& operator=(const Mesh&) = delete;
};

// main.cpp:286-352 Scene, minus the Enoki arrays: geometry lives on the GPU
// behind spt_scene.
class Scene {
  public:
    Scene() = default;
    ~Scene() { if (scene_) spt_scene_destroy(scene_); }
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;

    void add_triangle_mesh(const std::string& path) {  // main.cpp:288
        mesh_.reset(new Mesh(path));
        pbrt_ = mesh_->pbrt;
    }
    void commit(int device = 0) {                      // main.cpp:312
        if (!mesh_) throw std::runtime_error("Scene::commit: no mesh added");
        check(spt_init(device), "spt_init");
        const spt_mesh& m = mesh_->m;
        check(spt_scene_create(m.pos_tri, m.pos, m.nvert, m.ntri, m.nrm_tri, m.nrm, m.nnrm, m.tc_tri, m.tc, m.ntc,
                               m.mat_id, &scene_),
              "spt_scene_create");
    }
    // Binary scene cache (spt_scene_save / spt_scene_load): the committed
    // scene, with the pbrt camera / film / sky as its extra bytes.
    void save(const std::string& path) const {
        const bool has = pbrt_.has_camera || pbrt_.has_env;
        check(spt_scene_save(scene_, path.c_str(), has ? &pbrt_ : nullptr, has ? sizeof(pbrt_) : 0), "spt_scene_save");
    }
    void load(const std::string& path, int device = 0) {
        check(spt_init(device), "spt_init");
        if (scene_) spt_scene_destroy(scene_);
        scene_ = nullptr;
        mesh_.reset();
        pbrt_ = spt_pbrt_info{};
        uint64_t n = 0;
        check(spt_scene_load(path.c_str(), &scene_, &pbrt_, sizeof(pbrt_), &n), "spt_scene_load");
        if (n != 0 && n != sizeof(pbrt_)) throw std::runtime_error(path + ": extra bytes are not an spt_pbrt_info");
        if (n == 0) pbrt_ = spt_pbrt_info{};
    }
    // spt_render_async / spt_render_wait: queue the render on `stream` (the
    // stream's next work waits for it) and collect its statistics later
    uint64_t render_async(const spt_render_params& p, float* film_dev, void* stream) {
        uint64_t ticket = 0;
        check(spt_render_async(scene_, &p, film_dev, stream, &ticket), "spt_render_async");
        return ticket;
    }
    void render_wait(uint64_t ticket, spt_render_stats* stats) {
        check(spt_render_wait(scene_, ticket, stats), "spt_render_wait");
    }
    void render(const spt_render_params& p, float* film_dev, spt_render_stats* stats, void* stream = nullptr) {
        check(spt_render(scene_, &p, film_dev, stats, stream), "spt_render");
    }
    // spt_render_accum: samples [acc.sample_base, acc.sample_base + p.spp) added
    // onto the caller's running sums (progressive rendering)
    void render_accum(const spt_render_params& p, const spt_accum& acc, spt_render_stats* stats,
                      void* stream = nullptr) {
        check(spt_render_accum(scene_, &p, &acc, stats, stream), "spt_render_accum");
    }
    // spt_render_accum_list: the same pass over the listed tile pixels only
    void render_accum_list(const spt_render_params& p, const spt_accum& acc, const spt_pixel_list& list,
                           spt_render_stats* stats, void* stream = nullptr) {
        check(spt_render_accum_list(scene_, &p, &acc, &list, stats, stream), "spt_render_accum_list");
    }
    // spt_render_aov: the first-hit buffers of p's tile, queued on `stream`
    void render_aov(const spt_render_params& p, const spt_aov& planes, void* stream = nullptr) {
        check(spt_render_aov(scene_, &p, &planes, stream), "spt_render_aov");
    }
    // spt_scene_update_geometry: new positions / normals for the committed
    // triangles, the BVH refitted in place (host arrays; synchronous)
    void update_geometry(const int32_t* pos_tri, const float* pos, uint64_t nvert, uint64_t ntri,
                         const int32_t* nrm_tri = nullptr, const float* nrm = nullptr, uint64_t nnrm = 0) {
        check(spt_scene_update_geometry(scene_, pos_tri, pos, nvert, ntri, nrm_tri, nrm, nnrm),
              "spt_scene_update_geometry");
    }
    // ... device pointers, the kernels on `stream`
    void update_geometry(const int32_t* pos_tri, const float* pos, uint64_t nvert, uint64_t ntri,
                         const int32_t* nrm_tri, const float* nrm, uint64_t nnrm, void* stream) {
        check(spt_scene_update_geometry_device(scene_, pos_tri, pos, nvert, ntri, nrm_tri, nrm, nnrm, stream),
              "spt_scene_update_geometry_device");
    }
    // spt_scene_set_envmap: the octahedral sky image (n x n interleaved RGB; see
    // envmap_from_latlong) and its world -> map rotation (9 floats row-major,
    // nullptr: identity); rgb nullptr removes the map
    void set_envmap(const float* rgb, uint32_t n, const float* rotation = nullptr) {
        check(spt_scene_set_envmap(scene_, rgb, n, rotation), "spt_scene_set_envmap");
    }
    // spt_scene_set_light_sampling: next-event estimation on the emissive triangles
    void set_light_sampling(bool on = true) {
        check(spt_scene_set_light_sampling(scene_, on ? 1u : 0u), "spt_scene_set_light_sampling");
    }
    // spt_scene_set_sky_sampling: importance sampling of the sky image with shadow rays
    void set_sky_sampling(bool on = true, float share = 0.5f) {
        check(spt_scene_set_sky_sampling(scene_, on ? 1u : 0u, share), "spt_scene_set_sky_sampling");
    }
    // spt_scene_set_mis: the balance heuristic between those shadow rays and the bounce rays
    void set_mis(bool on = true) { check(spt_scene_set_mis(scene_, on ? 1u : 0u), "spt_scene_set_mis"); }
    spt_refit_stats refit_stats() const {
        spt_refit_stats st{};
        check(spt_scene_get_refit_stats(scene_, &st), "spt_scene_get_refit_stats");
        return st;
    }
    // Commit a mesh loaded elsewhere (read only: several devices' scenes may
    // be built from one host mesh, one thread per device).
    void commit_from(const Mesh& mesh, int device) {
        check(spt_init(device), "spt_init");
        const spt_mesh& m = mesh.m;
        check(spt_scene_create(m.pos_tri, m.pos, m.nvert, m.ntri, m.nrm_tri, m.nrm, m.nnrm, m.tc_tri, m.tc, m.ntc,
                               m.mat_id, &scene_),
              "spt_scene_create");
        pbrt_ = mesh.pbrt;
    }
    spt_scene handle() const { return scene_; }
    const spt_mesh& mesh() const { return mesh_->m; }  // not after load()
    const spt_pbrt_info& pbrt_info() const { return pbrt_; }

  private:
    std::unique_ptr<Mesh> mesh_;
    spt_pbrt_info pbrt_{};
    spt_scene scene_ = nullptr;
};

// A PFM image on the host (spt_pfm_read): w x h interleaved RGB, rows top-down.
struct PfmImage {
    float* rgb = nullptr;
    uint32_t w = 0, h = 0;
    explicit PfmImage(const std::string& path) { check(spt_pfm_read(path.c_str(), &rgb, &w, &h), "spt_pfm_read"); }
    ~PfmImage() { spt_pfm_free(rgb); }
    PfmImage(const PfmImage&) = delete;
    PfmImage& operator=(const PfmImage&) = delete;
};

// spt_envmap_from_latlong: a lat-long image resampled to n x n octahedral texels (host only).
inline std::vector<float> envmap_from_latlong(const float* rgb, uint32_t w, uint32_t h, uint32_t n) {
    std::vector<float> out((size_t)n * n * 3);
    check(spt_envmap_from_latlong(rgb, w, h, n, out.data()), "spt_envmap_from_latlong");
    return out;
}

// Device floats owned for a scope (hipMalloc / hipFree; throws like check()).
class DeviceFloats {
  public:
    explicit DeviceFloats(size_t n) : n_(n) {
        if (hipMalloc((void**)&p_, sizeof(float) * (n ? n : 1)) != hipSuccess)
            throw std::runtime_error("hipMalloc of " + std::to_string(n) + " floats failed");
    }
    ~DeviceFloats() { (void)hipFree(p_); }
    DeviceFloats(const DeviceFloats&) = delete;
    DeviceFloats& operator=(const DeviceFloats&) = delete;
    float* get() const { return p_; }
    size_t size() const { return n_; }
    std::vector<float> to_host() const {  // synchronises with the null stream's order
        std::vector<float> h(n_);
        if (n_ && hipMemcpy(h.data(), p_, sizeof(float) * n_, hipMemcpyDeviceToHost) != hipSuccess)
            throw std::runtime_error("hipMemcpy to the host failed");
        return h;
    }

  private:
    float* p_ = nullptr;
    size_t n_ = 0;
};

// The eight planes of spt_render_aov for a tile of npx pixels, in one
// allocation: albedo r g b, normal x y z, depth, coverage.
class AovBuffers {
  public:
    explicit AovBuffers(size_t npx) : npx_(npx), buf_(8 * npx) {
        float* b = buf_.get();
        aov_ = spt_aov{b, b + npx, b + 2 * npx, b + 3 * npx, b + 4 * npx, b + 5 * npx, b + 6 * npx, b + 7 * npx};
    }
    const spt_aov& planes() const { return aov_; }
    size_t pixels() const { return npx_; }
    std::vector<float> to_host() const { return buf_.to_host(); }  // 8 x npx, in the order above

  private:
    size_t npx_;
    DeviceFloats buf_;
    spt_aov aov_{};
};

// spt_denoise with its scratch allocated for the call: color, out = 3 planes of
// p.width x p.height device floats (out must not alias color); guides may be
// NULL.  Synchronises `stream` before the scratch is freed.
inline void denoise(const spt_denoise_params& p, const float* color, const spt_aov* guides, float* out,
                    void* stream = nullptr) {
    DeviceFloats scratch(spt_denoise_scratch_bytes(p.width, p.height) / sizeof(float));
    check(spt_denoise(&p, color, guides, out, scratch.get(), stream), "spt_denoise");
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) throw std::runtime_error("spt::denoise: stream failed");
}

// spt_denoise_var with its scratch allocated for the call: color, variance,
// out = 3 planes (out must not alias an input); guides and variance_out may be
// NULL.  Synchronises `stream` before the scratch is freed.
inline void denoise_var(const spt_denoise_var_params& p, const float* color, const float* variance,
                        const spt_aov* guides, float* out, float* variance_out = nullptr, void* stream = nullptr) {
    DeviceFloats scratch(spt_denoise_var_scratch_bytes(p.width, p.height) / sizeof(float));
    check(spt_denoise_var(&p, color, variance, guides, out, variance_out, scratch.get(), stream), "spt_denoise_var");
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        throw std::runtime_error("spt::denoise_var: stream failed");
}

// spt_adapt_select with scratch the caller sized (spt_adapt_select_scratch_bytes):
// the active pixels of an accumulation, ascending, in list; returns their number.
inline uint32_t adapt_select(const spt_adapt_params& p, uint32_t npix, uint32_t sample_base, const float* sum,
                             const float* sum_sq, const uint32_t* count, uint32_t* list, void* scratch,
                             void* stream = nullptr) {
    uint32_t n = 0;
    check(spt_adapt_select(&p, npix, sample_base, sum, sum_sq, count, list, &n, scratch, stream), "spt_adapt_select");
    return n;
}

}  // namespace spt
