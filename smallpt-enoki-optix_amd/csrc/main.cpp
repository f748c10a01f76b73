// main.cpp — C++ host driver mirroring the reference's main() (main.cpp:354-446):
// load an OBJ (or a pbrt-v3 scene), commit the scene, render, normalise, read
// back, write a PFM, print the wall time.  Every constant defaults to the
// reference's; a .pbrt file's camera, film size and infinite light replace
// them, and flags override both.  A .sptc file is a binary scene cache
// (spt_scene_load: no parse, no BVH build); --save-cache writes one after commit.
//
// --gpus N renders the image on N devices of this node (the
// reference is single-GPU): one host thread per device commits its own copy
// of the scene (replicated BVH) and renders its interleaved row-group tile
// (spt_render_params.tile_*), then ONE RCCL collective, ncclGather over xGMI
// from a communicator per device (ncclCommInitAll, driven from one thread in
// an ncclGroupStart/End), queued on each rank's stream behind its render
// (spt_render_async, no host synchronisation between them), brings the fp32
// tiles to device 0, whose rows are put back in place.  Pixel RNG streams are keyed by the global pixel, so
// the image is bit-identical for any N.  --rehearse-shared-gpu places every
// tile on device 0 and gathers with device copies instead (a one-GPU box
// cannot host two RCCL ranks), so the tiling and assembly run anywhere.
//
//   spt_render_cli [scene.obj|scene.pbrt|scene.sptc] [-w W] [-h H] [-s spp] [-d casts] [-o out.pfm]
//                  [--wavefront paths] [--rr depth] [--rng-x-first] [--device N] [--save-cache f.sptc]
//                  [--gpus N] [--rows-per-group R] [--rehearse-shared-gpu]
//                  [--aov PREFIX] [--denoise [--denoise-iters N]]
//                  [--passes N] [--variance FILE] [--denoise-var]
//                  [--envmap sky.pfm [--env-res N] | --envmap-oct sky.pfm] [--env-rotate-y DEG] [--nee]
//                  [--sky-nee [--sky-share X]] [--mis]
//                  [--frames K --orbit-deg D [--temporal [--max-history N]]]
//
// --aov PREFIX writes the first-hit buffers of the render (spt_render_aov) as
// PREFIX.albedo.pfm, PREFIX.normal.pfm, PREFIX.depth.pfm (depth in all three
// channels) and PREFIX.coverage.pfm.  --denoise filters the image with
// spt_denoise (default sigmas, --denoise-iters iterations) guided by those
// buffers: the denoised image goes to -o, the raw one to <out>.raw.pfm.
// Single-device only: neither combines with --gpus above 1.
//
// --passes N renders N passes of -s samples each with spt_render_accum (the
// image is the accumulated film: the same bytes as one render of N x s
// samples).  --variance FILE writes the per-channel variance of the pixel mean
// as a PFM.  --denoise-var filters the image with spt_denoise_var, guided by
// that variance and the first-hit buffers as --denoise is (raw image to
// <out>.raw.pfm; --denoise-iters applies); it implies the second moments.
// Single-device too.
//
// --frames K renders K frames, the camera of frame k turned k x D degrees
// (--orbit-deg D) about its up axis through look_at, and writes them as
// <out>.000.pfm, <out>.001.pfm, ... (<out> without its .pfm).  Each frame is
// the render of -s samples of its view, independent of the others; with
// --temporal frame k draws samples [k s, (k + 1) s) and is blended with the
// history reprojected from frame k - 1 (spt_temporal_accumulate; --max-history N
// caps the history's length, default 64), and --denoise-var then filters each
// written frame with the temporal variance (raw frames to <out>.NNN.raw.pfm).
// Single-device; not with --passes, --adaptive, --variance, --aov or --denoise.
//
// --envmap FILE lights the scene with a lat-long sky image (a PFM, pbrt's
// convention, z up), resampled to an --env-res N (default 512) octahedral map
// (spt_envmap_from_latlong, spt_scene_set_envmap); --envmap-oct FILE takes a
// square PFM that is octahedral already.  --env-rotate-y DEG turns the world
// about its y axis before the lookup.  The map is set after --save-cache has
// written its file (the cache does not store it), so the flags work with a
// .sptc scene too, and with --passes, --adaptive, --aov and --denoise*.
// Single-device.
//
// --nee switches light sampling on (spt_scene_set_light_sampling: a shadow ray
// to the emissive triangles at every diffuse vertex), after --save-cache for
// the same reason.  It works with every other flag, --gpus included: each
// rank builds the same table from the same triangles, and the side stream is
// keyed by the global pixel.
//
// --sky-nee switches sky sampling on (spt_scene_set_sky_sampling: a shadow ray
// toward a direction drawn from the sky image's brightness at every diffuse
// vertex); it needs --envmap or --envmap-oct and is refused without one.
// --sky-share X (default 0.5, inside (0, 1)) is the probability of the sky
// where --nee samples the emissive triangles too.
//
// --mis combines those shadow rays with the bounce rays by the balance
// heuristic (spt_scene_set_mis); it needs --nee or --sky-nee and is refused
// without either.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <iostream>
#include <memory>
#include <thread>
#include <vector>

#include "spt.hpp"

namespace {

using clock_t_ = std::chrono::steady_clock;
double ms_since(clock_t_::time_point t0) {
    return std::chrono::duration<double, std::milli>(clock_t_::now() - t0).count();
}

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
void nccl_check(ncclResult_t r, const char* what) {
    if (r != ncclSuccess) throw std::runtime_error(std::string(what) + ": " + ncclGetErrorString(r));
}

// One device's share of a multi-GPU render.
struct Rank {
    int index = 0;                // tile index (the rank)
    int device = 0;
    spt::Scene scene;
    std::vector<uint32_t> rows;   // this tile's image rows (spt_tile_rows)
    float* tile = nullptr;        // (3, max_rows, W) fp32, padded to the largest tile
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;    // recorded on `stream` behind the queued render
    uint64_t ticket = 0;          // spt_render_async's, collected after the gather
    spt_render_stats st{};
    std::exception_ptr err;
};

// Renders p over ranks.size() tiles and assembles the (3, H, W) image on the
// host.  The scene is committed on each device (or loaded from the cache).
void render_multi(const std::string& path, const spt::Mesh* mesh, spt_render_params p, int ngpu, bool shared,
                  uint32_t rows_per_group, std::vector<float>& image, spt_render_stats& total, double& ms,
                  bool nee = false, bool mis = false) {
    int ndev = 0;
    hip_check(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
    if (!shared && ngpu > ndev)
        throw std::runtime_error("--gpus " + std::to_string(ngpu) + " but " + std::to_string(ndev) + " devices visible");
    const uint32_t W = p.width, H = p.height;
    std::vector<std::unique_ptr<Rank>> ranks;
    uint32_t max_rows = 1;
    for (int r = 0; r < ngpu; r++) {
        ranks.emplace_back(new Rank);
        Rank& k = *ranks.back();
        k.index = r;
        k.device = shared ? 0 : r;
        const uint32_t n = spt_tile_rows(H, (uint32_t)r, (uint32_t)ngpu, rows_per_group, nullptr, 0);
        k.rows.resize(n);
        spt_tile_rows(H, (uint32_t)r, (uint32_t)ngpu, rows_per_group, k.rows.data(), n);
        max_rows = std::max(max_rows, n);
    }
    const size_t count = (size_t)3 * max_rows * W;  // floats per rank in the gather
    // set-up, one thread per device: scene commit (replicated BVH), film tile, stream
    auto each = [&](auto&& fn) {
        std::vector<std::thread> th;
        for (auto& k : ranks)
            th.emplace_back([&fn, &k] {
                try {
                    hip_check(hipSetDevice(k->device), "hipSetDevice");
                    fn(*k);
                } catch (...) {
                    k->err = std::current_exception();
                }
            });
        for (auto& t : th) t.join();
        for (auto& k : ranks)
            if (k->err) std::rethrow_exception(k->err);
    };
    each([&](Rank& k) {
        if (mesh) k.scene.commit_from(*mesh, k.device);
        else k.scene.load(path, k.device);
        if (nee) k.scene.set_light_sampling();  // every rank's own table: the same triangles, the same table
        if (mis) k.scene.set_mis();
        hip_check(hipStreamCreateWithFlags(&k.stream, hipStreamNonBlocking), "hipStreamCreate");
        hip_check(hipEventCreateWithFlags(&k.done, hipEventDisableTiming), "hipEventCreate");
        hip_check(hipMalloc((void**)&k.tile, sizeof(float) * count), "hipMalloc tile");
        hip_check(hipMemsetAsync(k.tile, 0, sizeof(float) * count, k.stream), "hipMemset tile");
        hip_check(hipStreamSynchronize(k.stream), "hipStreamSynchronize");
    });
    std::vector<ncclComm_t> comms;
    if (!shared) {
        std::vector<int> devs;
        for (auto& k : ranks) devs.push_back(k->device);
        comms.resize(ngpu);
        nccl_check(ncclCommInitAll(comms.data(), ngpu, devs.data()), "ncclCommInitAll");
    }
    float* recv = nullptr;  // device 0: ngpu x count floats
    hip_check(hipSetDevice(ranks[0]->device), "hipSetDevice");
    hip_check(hipMalloc((void**)&recv, sizeof(float) * count * ngpu), "hipMalloc gather");

    const auto t0 = clock_t_::now();
    // every rank queues its tile's render (main.cpp:385-429 on its rows) on its
    // stream and returns: the gather below is queued on the same streams behind
    // the renders (spt_render_async: the caller stream's next work waits for
    // the render), so no host synchronisation sits between render and gather
    each([&](Rank& k) {
        spt_render_params q = p;
        q.tile_index = (uint32_t)k.index;
        q.tile_count = (uint32_t)ngpu;
        q.rows_per_group = rows_per_group;
        if (!k.rows.empty()) k.ticket = k.scene.render_async(q, k.tile, k.stream);
        hip_check(hipEventRecord(k.done, k.stream), "hipEventRecord");
    });
    // the one exchange step: the fp32 tiles to device 0
    if (!shared) {
        nccl_check(ncclGroupStart(), "ncclGroupStart");
        for (int r = 0; r < ngpu; r++) {
            hip_check(hipSetDevice(ranks[r]->device), "hipSetDevice");
            nccl_check(ncclGather(ranks[r]->tile, r == 0 ? recv : nullptr, count, ncclFloat, 0, comms[r],
                                  ranks[r]->stream),
                       "ncclGather");
        }
        nccl_check(ncclGroupEnd(), "ncclGroupEnd");
        for (auto& k : ranks) {
            hip_check(hipSetDevice(k->device), "hipSetDevice");
            hip_check(hipStreamSynchronize(k->stream), "hipStreamSynchronize");
        }
    } else {
        hip_check(hipSetDevice(ranks[0]->device), "hipSetDevice");
        for (int r = 0; r < ngpu; r++) {
            // (device copies on rank 0's stream, each behind that rank's render)
            hip_check(hipStreamWaitEvent(ranks[0]->stream, ranks[r]->done, 0), "hipStreamWaitEvent");
            hip_check(hipMemcpyAsync(recv + (size_t)r * count, ranks[r]->tile, sizeof(float) * count,
                                     hipMemcpyDeviceToDevice, ranks[0]->stream),
                      "hipMemcpy gather");
        }
        hip_check(hipStreamSynchronize(ranks[0]->stream), "hipStreamSynchronize");
    }
    ms = ms_since(t0);
    each([&](Rank& k) {  // the renders' statistics (their work is done: the gather waited for it)
        if (!k.rows.empty()) k.scene.render_wait(k.ticket, &k.st);
    });

    // rank 0 puts every tile's rows back in place
    std::vector<float> gathered(count * ngpu);
    hip_check(hipSetDevice(ranks[0]->device), "hipSetDevice");
    hip_check(hipMemcpy(gathered.data(), recv, sizeof(float) * gathered.size(), hipMemcpyDeviceToHost), "hipMemcpy");
    image.assign((size_t)3 * H * W, 0.0f);
    total = spt_render_stats{};
    for (int r = 0; r < ngpu; r++) {
        const Rank& k = *ranks[r];
        const size_t n = k.rows.size();
        const float* t = gathered.data() + (size_t)r * count;
        for (int c = 0; c < 3; c++)
            for (size_t i = 0; i < n; i++)
                std::memcpy(&image[((size_t)c * H + k.rows[i]) * W], t + ((size_t)c * n + i) * W, sizeof(float) * W);
        total.paths += k.st.paths;
        total.ray_casts += k.st.ray_casts;
    }
    for (auto& c : comms) ncclCommDestroy(c);
    (void)hipFree(recv);
    for (auto& k : ranks) {
        hip_check(hipSetDevice(k->device), "hipSetDevice");
        (void)hipFree(k->tile);
        (void)hipEventDestroy(k->done);
        (void)hipStreamDestroy(k->stream);
    }
}

// `camera` turned `degrees` about its up axis through look_at (0: the camera as it is).
spt_camera orbit(const spt_camera& camera, double degrees) {
    if (degrees == 0.0) return camera;
    const double t = degrees * 3.14159265358979323846 / 180.0, c = std::cos(t), s = std::sin(t);
    double u[3], v[3];
    double ul = 0.0;
    for (int k = 0; k < 3; k++) ul += (double)camera.up[k] * camera.up[k];
    ul = std::sqrt(ul);
    for (int k = 0; k < 3; k++) {
        u[k] = camera.up[k] / ul;
        v[k] = (double)camera.look_from[k] - camera.look_at[k];
    }
    const double uv = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
    const double x[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    spt_camera r = camera;  // Rodrigues: v cos + (u x v) sin + u (u.v) (1 - cos)
    for (int k = 0; k < 3; k++) r.look_from[k] = (float)(camera.look_at[k] + (v[k] * c + x[k] * s + u[k] * uv * (1.0 - c)));
    return r;
}

// --frames: K frames of p's view turned orbit_deg per frame, written to
// <out>.NNN.pfm.  Without `temporal` frame k is spt_render of its view; with it,
// the frame's own samples [k spp, (k + 1) spp) on zeroed sums, its first-hit
// buffers, and spt_temporal_accumulate onto ping-pong histories.
void render_frames(spt::Scene& scene, spt_render_params p, int frames, double orbit_deg, bool temporal, float max_history,
                   bool do_denoise_var, int denoise_iters, const std::string& out, spt_render_stats& st, double& ms) {
    const size_t npx = (size_t)p.width * p.height;
    if ((uint64_t)p.spp * (uint64_t)frames >= (1ull << 24))
        throw std::runtime_error("--frames x -s must stay below 2^24 samples");
    const std::string stem = spt::ends_with(out, ".pfm") ? out.substr(0, out.size() - 4) : out;
    const spt_camera base = p.camera;
    spt::DeviceFloats film(3 * npx), sums(temporal ? 3 * npx : 0), sums_sq(temporal ? 3 * npx : 0);
    // two histories (colour 3, moment 3, length 1, film 3, variance 3 planes) and two sets of guides
    std::unique_ptr<spt::DeviceFloats> hist[2];
    std::unique_ptr<spt::AovBuffers> aov[2];
    spt_camera cams[2] = {base, base};
    if (temporal)
        for (int k = 0; k < 2; k++) {
            hist[k].reset(new spt::DeviceFloats(13 * npx));
            aov[k].reset(new spt::AovBuffers(npx));
        }
    std::vector<float> host(3 * npx);
    for (int k = 0; k < frames; k++) {
        p.camera = orbit(base, orbit_deg * k);
        const auto t0 = clock_t_::now();
        spt_render_stats fs{};
        const float* shown = film.get();
        const float* variance = nullptr;
        const int cur = k & 1;
        if (!temporal) {
            scene.render(p, film.get(), &fs);
        } else {
            hip_check(hipMemset(sums.get(), 0, sizeof(float) * 3 * npx), "hipMemset sum");
            hip_check(hipMemset(sums_sq.get(), 0, sizeof(float) * 3 * npx), "hipMemset sum_sq");
            spt_accum acc{};
            acc.sample_base = (uint32_t)k * p.spp;
            acc.sum = sums.get();
            acc.sum_sq = sums_sq.get();
            scene.render_accum(p, acc, &fs);
            scene.render_aov(p, aov[cur]->planes());
            cams[cur] = p.camera;
            spt_temporal_params tp;
            spt_default_temporal_params(&tp);
            tp.width = p.width;
            tp.height = p.height;
            tp.camera = p.camera;
            tp.prev_camera = cams[k ? 1 - cur : cur];
            tp.samples = (float)p.spp;
            tp.max_history = max_history;
            const auto history = [npx](float* b) { return spt_history{b, b + 3 * npx, b + 6 * npx}; };
            float* const now = hist[cur]->get();
            const spt_history h_out = history(now), h_prev = history(hist[1 - cur]->get());
            spt::check(spt_temporal_accumulate(&tp, sums.get(), sums_sq.get(), &aov[cur]->planes(), k ? &h_prev : nullptr,
                                               k ? &aov[1 - cur]->planes() : nullptr, &h_out, now + 7 * npx,
                                               now + 10 * npx, nullptr),
                       "spt_temporal_accumulate");
            shown = now + 7 * npx;
            variance = now + 10 * npx;
        }
        hip_check(hipMemcpy(host.data(), shown, sizeof(float) * 3 * npx, hipMemcpyDeviceToHost), "hipMemcpy film");
        char num[16];
        std::snprintf(num, sizeof(num), ".%03d", k);
        if (do_denoise_var) {
            spt::check(spt_pfm_write((stem + num + ".raw.pfm").c_str(), host.data(), host.data() + npx,
                                     host.data() + 2 * npx, p.width, p.height),
                       "spt_pfm_write");
            spt_denoise_var_params dp;
            spt_default_denoise_var_params(&dp);
            dp.width = p.width;
            dp.height = p.height;
            if (denoise_iters >= 0) dp.iterations = (uint32_t)denoise_iters;
            spt::DeviceFloats clean(3 * npx);
            spt::denoise_var(dp, shown, variance, &aov[cur]->planes(), clean.get());
            host = clean.to_host();
        }
        ms += ms_since(t0);
        st.paths += fs.paths;
        st.ray_casts += fs.ray_casts;
        spt::check(spt_pfm_write((stem + num + ".pfm").c_str(), host.data(), host.data() + npx, host.data() + 2 * npx,
                                 p.width, p.height),
                   "spt_pfm_write");
    }
}

}  // namespace

int main(int argc, char** argv) {
    std::string obj = "mitsuba.obj";  // main.cpp:365
    std::string out = "wurst.pfm";    // main.cpp:442
    std::string cache_out, aov_prefix;
    bool do_denoise = false, do_denoise_var = false;
    std::string variance_out;
    int passes = 0;  // 0: one spt_render
    // --adaptive TOL: passes of -s, 2 -s, 4 -s, ... samples (each pass as long as
    // all before it) over the pixels spt_adapt_select still finds unconverged
    bool adaptive = false;
    spt_adapt_params ap;
    spt_default_adapt_params(&ap);
    std::string spp_map_out;
    std::string envmap_in;      // --envmap (lat-long) or --envmap-oct
    bool envmap_oct = false, env_rotate = false;
    int env_res = 512;
    double env_rotate_y = 0.0;  // degrees
    bool nee = false;           // --nee: spt_scene_set_light_sampling
    bool sky_nee = false, set_sky_share = false;  // --sky-nee: spt_scene_set_sky_sampling
    float sky_share = 0.5f;     // --sky-share
    bool mis = false;           // --mis: spt_scene_set_mis
    int denoise_iters = -1;  // -1: spt_default_denoise_params
    int frames = 0;             // --frames: 0 = one image
    double orbit_deg = 0.0;     // --orbit-deg, per frame
    bool set_orbit = false, temporal = false, set_max_history = false;
    float max_history = 64.0f;  // --max-history (spt_default_temporal_params)
    int device = 0, ngpu = 0;
    uint32_t rows_per_group = 8;
    bool shared = false;
    spt_render_params p;
    spt_default_params(&p);            // 512 x 512, 100 spp, 2 casts (main.cpp:357-361)
    bool set_w = false, set_h = false;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) { std::cerr << "missing value for " << a << "\n"; std::exit(2); }
            return argv[++i];
        };
        if (a == "-w") { p.width = (uint32_t)std::atoi(next()); set_w = true; }
        else if (a == "-h") { p.height = (uint32_t)std::atoi(next()); set_h = true; }
        else if (a == "-s") p.spp = (uint32_t)std::atoi(next());
        else if (a == "-d") p.max_depth = (uint32_t)std::atoi(next());
        else if (a == "-o") out = next();
        else if (a == "--wavefront") p.wavefront_paths = (uint32_t)std::atoi(next());
        else if (a == "--rr") p.rr_start_depth = (uint32_t)std::atoi(next());
        else if (a == "--rng-x-first") p.rng_order = SPT_RNG_X_FIRST;
        else if (a == "--device") device = std::atoi(next());
        else if (a == "--save-cache") cache_out = next();
        else if (a == "--gpus") ngpu = std::atoi(next());
        else if (a == "--rows-per-group") rows_per_group = (uint32_t)std::atoi(next());
        else if (a == "--rehearse-shared-gpu") shared = true;
        else if (a == "--aov") aov_prefix = next();
        else if (a == "--denoise") do_denoise = true;
        else if (a == "--denoise-iters") denoise_iters = std::atoi(next());
        else if (a == "--denoise-var") do_denoise_var = true;
        else if (a == "--passes") passes = std::atoi(next());
        else if (a == "--variance") variance_out = next();
        else if (a == "--adaptive") { adaptive = true; ap.tolerance = (float)std::atof(next()); }
        else if (a == "--min-spp") ap.min_spp = (uint32_t)std::atoi(next());
        else if (a == "--max-spp") ap.max_spp = (uint32_t)std::atoi(next());
        else if (a == "--spp-map") spp_map_out = next();
        else if (a == "--envmap") { envmap_in = next(); envmap_oct = false; }
        else if (a == "--envmap-oct") { envmap_in = next(); envmap_oct = true; }
        else if (a == "--env-res") env_res = std::atoi(next());
        else if (a == "--env-rotate-y") { env_rotate_y = std::atof(next()); env_rotate = true; }
        else if (a == "--nee") nee = true;
        else if (a == "--sky-nee") sky_nee = true;
        else if (a == "--mis") mis = true;
        else if (a == "--sky-share") { sky_share = (float)std::atof(next()); set_sky_share = true; }
        else if (a == "--frames") frames = std::atoi(next());
        else if (a == "--orbit-deg") { orbit_deg = std::atof(next()); set_orbit = true; }
        else if (a == "--temporal") temporal = true;
        else if (a == "--max-history") { max_history = (float)std::atof(next()); set_max_history = true; }
        else if (!a.empty() && a[0] != '-') obj = a;
        else { std::cerr << "unknown flag " << a << "\n"; return 2; }
    }
    if (ngpu < 0 || rows_per_group == 0) { std::cerr << "--gpus must be >= 1, --rows-per-group >= 1\n"; return 2; }
    const bool want_aov = !aov_prefix.empty() || do_denoise || do_denoise_var;
    if (want_aov && ngpu > 1) {
        std::cerr << "--aov / --denoise render on one device: not with --gpus " << ngpu
                  << " (the multi-GPU gather of the feature buffers is not implemented)\n";
        return 2;
    }
    if (passes < 0 || ((passes > 0 || !variance_out.empty()) && ngpu > 1)) {
        std::cerr << "--passes takes N >= 1; --passes / --variance render on one device: not with --gpus above 1\n";
        return 2;
    }
    if (adaptive && (ngpu > 1 || passes > 0)) {
        std::cerr << "--adaptive renders on one device and sets its own passes: not with --gpus above 1 or --passes\n";
        return 2;
    }
    if (!adaptive && !spp_map_out.empty()) {
        std::cerr << "--spp-map goes with --adaptive\n";
        return 2;
    }
    if (adaptive && (ap.min_spp > ap.max_spp || !(ap.tolerance >= 0.0f) || ap.max_spp >= (1u << 24))) {
        std::cerr << "--adaptive takes TOL >= 0, --min-spp <= --max-spp < 2^24\n";
        return 2;
    }
    if (envmap_in.empty() && env_rotate) {
        std::cerr << "--env-rotate-y goes with --envmap / --envmap-oct\n";
        return 2;
    }
    if (!envmap_in.empty() && (ngpu > 1 || env_res < 1 || env_res > 4096 || !std::isfinite(env_rotate_y))) {
        std::cerr << "--envmap renders on one device (not with --gpus above 1); --env-res takes 1..4096\n";
        return 2;
    }
    if (sky_nee && envmap_in.empty()) {
        std::cerr << "--sky-nee samples the sky image: it goes with --envmap / --envmap-oct\n";
        return 2;
    }
    if ((set_sky_share && !sky_nee) || !(sky_share > 0.0f && sky_share < 1.0f)) {
        std::cerr << "--sky-share takes a number inside (0, 1) and goes with --sky-nee\n";
        return 2;
    }
    if (mis && !nee && !sky_nee) {
        std::cerr << "--mis weighs the shadow rays of --nee / --sky-nee against the bounce rays: it goes with one of them\n";
        return 2;
    }
    if (do_denoise && do_denoise_var) {
        std::cerr << "--denoise and --denoise-var: choose one\n";
        return 2;
    }
    if (denoise_iters > 8 || (denoise_iters >= 0 && !do_denoise && !do_denoise_var)) {
        std::cerr << "--denoise-iters takes 0..8 and goes with --denoise / --denoise-var\n";
        return 2;
    }
    if (frames < 0 || (frames == 0 && (set_orbit || temporal)) || (set_max_history && !temporal) ||
        !std::isfinite(orbit_deg) || !(max_history >= 0.0f)) {
        std::cerr << "--frames takes K >= 1; --orbit-deg and --temporal go with it, --max-history N >= 0 with --temporal\n";
        return 2;
    }
    if (frames > 0 && (ngpu > 1 || passes > 0 || adaptive || !variance_out.empty() || !aov_prefix.empty() || do_denoise ||
                       (do_denoise_var && !temporal))) {
        std::cerr << "--frames renders on one device; not with --passes, --adaptive, --variance, --aov or --denoise, and "
                     "--denoise-var needs --temporal\n";
        return 2;
    }
    if (frames > 0 && ngpu == 1) ngpu = 0;
    // the accumulating path: asked for, or needed for the variance
    const bool accum = passes > 0 || !variance_out.empty() || do_denoise_var || adaptive;
    const bool moments = !variance_out.empty() || do_denoise_var || adaptive;
    if (passes == 0) passes = 1;
    if ((want_aov || accum || !envmap_in.empty()) && ngpu == 1) ngpu = 0;  // one tile: the single-device path below (the same image)
    try {
        const bool cache = spt::ends_with(obj, ".sptc");
        std::unique_ptr<spt::Mesh> mesh;
        spt_pbrt_info pi{};
        spt::Scene scene;  // the single-device path
        auto tl = clock_t_::now();
        if (ngpu >= 1) {  // multi-GPU: the host mesh once, a scene per device in render_multi
            if (cache) {
                spt::Scene probe;  // the cache's pbrt camera / film / sky
                probe.load(obj, device);
                pi = probe.pbrt_info();
            } else {
                mesh.reset(new spt::Mesh(obj));
                pi = mesh->pbrt;
            }
        } else if (cache) {
            scene.load(obj, device);
            pi = scene.pbrt_info();
        } else {
            scene.add_triangle_mesh(obj);  // main.cpp:365
            scene.commit(device);          // main.cpp:366
            pi = scene.pbrt_info();
        }
        std::cerr << "scene ready in " << ms_since(tl) << " ms" << std::endl;
        if (!cache_out.empty()) {
            if (ngpu >= 1) throw std::runtime_error("--save-cache: use it without --gpus");
            scene.save(cache_out);
        }
        if (!envmap_in.empty()) {  // after the save: the cache does not store the map
            const spt::PfmImage img(envmap_in);
            const double t = env_rotate_y * 3.14159265358979323846 / 180.0, c = std::cos(t), sn = std::sin(t);
            const float rot[9] = {(float)c, 0.0f, (float)sn, 0.0f, 1.0f, 0.0f, (float)-sn, 0.0f, (float)c};
            if (envmap_oct) {
                if (img.w != img.h) throw std::runtime_error("--envmap-oct: " + envmap_in + " is not square");
                scene.set_envmap(img.rgb, img.w, env_rotate ? rot : nullptr);
            } else {
                const std::vector<float> oct = spt::envmap_from_latlong(img.rgb, img.w, img.h, (uint32_t)env_res);
                scene.set_envmap(oct.data(), (uint32_t)env_res, env_rotate ? rot : nullptr);
            }
        }
        if (nee && ngpu < 1) scene.set_light_sampling();  // after the save: the cache does not store the switch
        if (sky_nee) scene.set_sky_sampling(true, sky_share);  // (a map renders on one device: this scene)
        if (mis && ngpu < 1) scene.set_mis();
        if (pi.has_camera) {
            p.camera = pi.camera;
            if (!set_w) p.width = pi.xres;
            if (!set_h) p.height = pi.yres;
        }
        if (pi.has_env)
            for (int c = 0; c < 3; c++) p.env[c] = pi.env[c];
        const size_t npx = (size_t)p.width * p.height;
        std::vector<float> host(3 * npx);
        spt_render_stats st{};
        double ms = 0.0;
        if (frames > 0) {
            render_frames(scene, p, frames, orbit_deg, temporal, max_history, do_denoise_var, denoise_iters, out, st, ms);
            std::cout << ms << std::endl;
            std::cout << "wrote " << frames << " frames" << std::endl;
            std::cout << "paths " << st.paths << " casts " << st.ray_casts << " Mpaths/s " << st.paths / (ms * 1e3)
                      << std::endl;
            std::cout << "done" << std::endl;
            return 0;
        }
        if (ngpu >= 1) {
            render_multi(obj, mesh.get(), p, ngpu, shared, rows_per_group, host, st, ms, nee, mis);
            std::cout << ms << std::endl;  // main.cpp:431 (render + gather)
        } else {
            float* film = nullptr;
            hip_check(hipMalloc((void**)&film, sizeof(float) * 3 * npx), "hipMalloc film");
            // spt_render_accum's planes: sum, sum_sq, variance (the film is `film`)
            std::unique_ptr<spt::DeviceFloats> sums, sums_sq, variance;
            // the feature buffers line up with the samples of one render of every pass's samples
            spt_render_params whole = p;
            auto t0 = clock_t_::now();
            if (accum) {
                if (!adaptive && (uint64_t)p.spp * (uint64_t)passes >= (1ull << 24))
                    throw std::runtime_error("--passes x -s must stay below 2^24 samples");
                whole.spp = p.spp * (uint32_t)passes;
                sums.reset(new spt::DeviceFloats(3 * npx));
                if (moments) {
                    sums_sq.reset(new spt::DeviceFloats(3 * npx));
                    variance.reset(new spt::DeviceFloats(3 * npx));
                }
                spt_accum acc{};
                acc.sum = sums->get();
                acc.sum_sq = moments ? sums_sq->get() : nullptr;
                acc.film = film;
                acc.variance = moments ? variance->get() : nullptr;
                if (adaptive) {
                    // per-pixel sample counts, the active list and the selection's scratch
                    spt::DeviceFloats count(npx), list(npx);
                    spt::DeviceFloats scratch(spt_adapt_select_scratch_bytes((uint32_t)npx) / sizeof(float));
                    hip_check(hipMemset(count.get(), 0, sizeof(uint32_t) * npx), "hipMemset count");
                    spt_pixel_list pl{};
                    pl.pixels = (const uint32_t*)list.get();
                    pl.count = (uint32_t*)count.get();
                    spt_render_params q = p;
                    uint32_t base = 0, npass = 0;
                    uint64_t next = p.spp;
                    for (;; npass++, next *= 2) {
                        // passes grow: -s, 2 -s, 4 -s, ... samples, the last cut at max_spp
                        if (base >= ap.max_spp) break;
                        q.spp = (uint32_t)std::min<uint64_t>(next, ap.max_spp - base);
                        pl.n = spt::adapt_select(ap, (uint32_t)npx, base, acc.sum, acc.sum_sq, pl.count,
                                                 (uint32_t*)list.get(), scratch.get());
                        if (pl.n == 0) break;
                        spt_render_stats ps{};
                        acc.sample_base = base;
                        scene.render_accum_list(q, acc, pl, &ps);
                        st.paths += ps.paths;
                        st.ray_casts += ps.ray_casts;
                        base += q.spp;
                    }
                    whole.spp = std::max<uint32_t>(base, 1);
                    std::cout << "adaptive passes " << npass << " samples up to " << base << " total paths " << st.paths
                              << std::endl;
                    if (!spp_map_out.empty()) {
                        const std::vector<float> c = count.to_host();  // uint32 bits
                        std::vector<float> f(npx);
                        for (size_t i = 0; i < npx; i++) {
                            uint32_t u;
                            std::memcpy(&u, &c[i], sizeof(u));
                            f[i] = (float)u;
                        }
                        spt::check(spt_pfm_write(spp_map_out.c_str(), f.data(), f.data(), f.data(), p.width, p.height),
                                   "spt_pfm_write");
                    }
                } else {
                    for (int k = 0; k < passes; k++) {
                        spt_render_stats ps{};
                        acc.sample_base = (uint32_t)k * p.spp;
                        scene.render_accum(p, acc, &ps);
                        st.paths += ps.paths;
                        st.ray_casts += ps.ray_casts;
                    }
                }
            } else {
                scene.render(p, film, &st);    // main.cpp:385-429
            }
            ms = ms_since(t0);
            std::cout << ms << std::endl;  // main.cpp:431
            if (!variance_out.empty()) {
                const std::vector<float> v = variance->to_host();
                spt::check(spt_pfm_write(variance_out.c_str(), v.data(), v.data() + npx, v.data() + 2 * npx, p.width,
                                         p.height),
                           "spt_pfm_write");
            }
            hip_check(hipMemcpy(host.data(), film, sizeof(float) * 3 * npx, hipMemcpyDeviceToHost), "hipMemcpy film");
            if (want_aov) {
                spt::AovBuffers aov(npx);
                scene.render_aov(whole, aov.planes());
                if (!aov_prefix.empty()) {
                    const std::vector<float> a = aov.to_host();  // albedo r g b, normal x y z, depth, coverage
                    const float* d = a.data();
                    auto write = [&](const char* name, const float* r, const float* g, const float* b) {
                        spt::check(spt_pfm_write((aov_prefix + name).c_str(), r, g, b, p.width, p.height), "spt_pfm_write");
                    };
                    write(".albedo.pfm", d, d + npx, d + 2 * npx);
                    write(".normal.pfm", d + 3 * npx, d + 4 * npx, d + 5 * npx);
                    write(".depth.pfm", d + 6 * npx, d + 6 * npx, d + 6 * npx);
                    write(".coverage.pfm", d + 7 * npx, d + 7 * npx, d + 7 * npx);
                }
                if (do_denoise) {
                    spt::check(spt_pfm_write((out + ".raw.pfm").c_str(), host.data(), host.data() + npx,
                                             host.data() + 2 * npx, p.width, p.height),
                               "spt_pfm_write");
                    spt_denoise_params dp;
                    spt_default_denoise_params(&dp);
                    dp.width = p.width;
                    dp.height = p.height;
                    if (denoise_iters >= 0) dp.iterations = (uint32_t)denoise_iters;
                    spt::DeviceFloats clean(3 * npx);
                    spt::denoise(dp, film, &aov.planes(), clean.get());
                    host = clean.to_host();
                }
                if (do_denoise_var) {
                    spt::check(spt_pfm_write((out + ".raw.pfm").c_str(), host.data(), host.data() + npx,
                                             host.data() + 2 * npx, p.width, p.height),
                               "spt_pfm_write");
                    spt_denoise_var_params dp;
                    spt_default_denoise_var_params(&dp);
                    dp.width = p.width;
                    dp.height = p.height;
                    if (denoise_iters >= 0) dp.iterations = (uint32_t)denoise_iters;
                    spt::DeviceFloats clean(3 * npx);
                    spt::denoise_var(dp, film, variance->get(), &aov.planes(), clean.get());
                    host = clean.to_host();
                }
            }
            (void)hipFree(film);
        }
        std::cout << "writing image" << std::endl;  // main.cpp:441
        spt::check(spt_pfm_write(out.c_str(), host.data(), host.data() + npx, host.data() + 2 * npx, p.width, p.height),
                   "spt_pfm_write");
        std::cout << "paths " << st.paths << " casts " << st.ray_casts << " Mpaths/s " << st.paths / (ms * 1e3)
                  << std::endl;
        std::cout << "done" << std::endl;  // main.cpp:444
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}
