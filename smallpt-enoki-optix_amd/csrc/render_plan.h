// render_plan.h — the render's policy as a pure function: which pipeline runs,
// whether the job fits in flight and in how many sample chunks, how many paths
// the memory allows, the work order, the queue caching, the drain's refill
// threshold, the sub-wavefront count and the film chunk (render.cpp
// render_enqueue consumes the plan).  Host only, no HIP: every constant below
// was measured (DESIGN.md §4–§6), and tests/native/plan_check.cpp runs the
// function on the CPU at the thresholds no test render can reach.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/spt.h"

namespace spt {

constexpr int kMaxStreams = 4;
// Path queue planes (spt_internal.h PathQueue): 2 (unit), 3 (albedo) or 4
// (emitters) 16-B quads per path.
constexpr uint64_t kHitBytes = 16;
// an out-of-memory render retries with half its paths in flight down to this many
constexpr uint64_t kMinRetryPaths = 1u << 16;
// SPT_WORK_AUTO: pixel-major for scenes beyond the Infinity Cache, and in the
// fused kernel for tiles of at least 16M paths (plan_render)
constexpr uint64_t kPixelMajorMinSceneBytes = 256ull << 20;
constexpr uint64_t kPixelMajorMinFusedPaths = 16ull << 20;
// ... and in the wavefront for scenes beyond one XCD's L2 on tiles of <= 4M
// pixels, with 24M paths in flight when the in-flight count is left at its
// default (32M)
constexpr uint64_t kPixelMajorMinWaveSceneBytes = 4ull << 20;
constexpr uint64_t kPixelMajorMaxWaveTilePx = 4ull << 20;
constexpr uint32_t kDefaultWavefrontPaths = 1u << 25;
constexpr uint64_t kPixelMajorWavefrontPaths = 24ull << 20;
// spt_config.drain_q8 default: a sub-wavefront's queue shorter than this many
// 1/256ths of its persistent isect lanes goes to the drain launch
constexpr uint32_t kDefaultDrainQ8 = 1024;
// spt_config.fused_max_paths default: AUTO runs the fused kernel only for jobs
// of at most 1M paths, fewer than two chip fills of lanes (config 0's 262k:
// the wavefront's launches and streams outweigh the work, 372 vs 823 Mpaths/s)
constexpr uint64_t kDefaultFusedMaxPaths = 1ull << 20;
// spt_config.fit_paths default: jobs (or sample chunks, fit_chunks) of at most
// 2^28 paths start every path at once: 21 GB of queues per working set in unit
// mode, 34 GB with emitters (HBM is 288 GB); config 3 +3.7 % over 2^27, config
// 2 -0.7 % (profiles/r05_exp/fit_paths_rgb_waves/)
constexpr uint64_t kDefaultFitPaths = 1ull << 28;
// spt_config.drain_casts default: the drain runs this many casts after a
// sub-wavefront's last work item started, whatever its queue holds
constexpr uint32_t kDefaultDrainCasts = 1;
// spt_config.drain_refill_idle AUTO (0): free lanes a drain wave waits for
// before it refills and shades — scenes with analytic spheres (tested in the
// shade, with smallpt's mirror / glass: the pass costs several trace steps),
// scenes whose queue is streamed (beyond the Infinity Cache), the rest
constexpr uint32_t kDrainIdleSpheres = 56;
constexpr uint32_t kDrainIdleStream = 40;
constexpr uint32_t kDrainIdleCached = 24;

// Everything plan_render reads.
struct RenderPlanIn {
    // the params: the tile's pixels, samples, SPT_FLAG_*, the explicit paths in flight (0: the config's)
    uint64_t P = 0;
    uint32_t spp = 0, flags = 0, wavefront_paths = 0;
    // spt_render_accum_list: the listed pixels, the only ones that take samples
    // (0: no list, every tile pixel).  The job is A x spp work items — the
    // pipeline, the fit and the paths in flight follow it — while the film
    // chunk keeps a slot per tile pixel and sample (P), since a path's slot is
    // indexed by its tile pixel
    uint64_t A = 0;
    const spt_config* cfg = nullptr;
    // the scene: its path mode (spt_internal.h PathMode) with the mode's 16-B
    // queue planes and film bytes per path, the bytes of its device arrays, its
    // analytic spheres, whether it has a wide BVH
    int mode = 0;
    uint32_t planes = 0, film_unit = 0;
    uint64_t device_bytes = 0;
    uint32_t nsph = 0;
    bool wide_nodes = false;
    // ... of 64-B six-wide nodes (bvh_build.h), and whether the render's camera
    // is a pinhole (lens_radius 0): what the camera entry table needs
    bool node6 = false;
    bool pinhole = false;
    // the scene samples its emissive triangles (spt_scene_set_light_sampling with
    // a non-empty table): only the fused lane loop has that estimator, so the
    // plan is the fused pipeline whatever spt_config.pipeline, the flags and the
    // job size say (the render refuses SPT_FLAG_WAVEFRONT / _TRAVERSAL_STATS first).
    // Likewise a scene that samples its sky image (spt_scene_set_sky_sampling, §15).
    bool nee = false;
    // the caller renders on a null stream (legacy or per-thread)
    bool null_caller = false;
    // what the working set bound to the caller's stream holds already (zeros:
    // none bound): the queues and hit records per sub-wavefront, the film chunk
    uint64_t held_sub[kMaxStreams] = {};
    uint64_t held_film = 0;
    uint64_t held_entry = 0;  // ... and the camera entry table
    // the device's free memory, asked at most once per plan and only when
    // fit_bytes is 0 and the set must grow; false: unknown
    bool (*free_bytes)(void* ctx, uint64_t* out) = nullptr;
    void* free_ctx = nullptr;
};

// Every decision the enqueue consumes.
struct RenderPlan {
    bool limit = false;       // C >= 2^31 (SPT_ERR_LIMIT): nothing below C is set
    bool fused = false;
    bool fit = false;         // every path of a chunk starts in the first refill
    uint32_t fit_chunk = 0;   // samples per chunk of a job run as fitting chunks
    uint64_t fit_paths = 0;   // spt_render_stats.fit_paths
    uint64_t mem_paths = 0;   // paths in flight the memory allows (queues + film chunk)
    uint64_t C = 0;           // paths in flight
    int K = 1;                // sub-wavefronts
    uint64_t Ck = 0;          // queue capacity of each
    uint32_t chunk = 1;       // samples per film chunk
    uint32_t pixel_major = 0, queue_nt = 0, drain_idle = 0;
    int mode = 0;
    bool own_queues = false;  // the set's streams get hardware queues of their own
    bool trav_stats = false;
    // from the config (and the flags) alone
    bool drain_on = false;    // the drain: not with traversal counters (isect kernel only)
    bool drain_sort = false;  // spt_config.drain_sort: a forced drain takes its queue sorted (wide-BVH scenes)
    bool sort_buffers = false;  // the working set keeps the sort's buffers
    // spt_config.lockstep_first = 2: the lockstep first cast also makes its
    // camera rays and shades its hits in the same launch (camera_cast_kernel;
    // wide-BVH scenes): no queue round trip for the first cast
    bool cam_cast = false;
    bool cam_shards = false;  // = 3: its survivors compacted per XCD shard, the drain's pools per shard
    bool lane_xcd = false;    // spt_config.xcd_remap bit 2: XCD-aware work distribution in the lane loops (drain, fused)
    // the camera cast ends a bounce ray that misses every child of the BVH root
    // instead of queueing it for the drain (camera_cast_kernel's kCull): with
    // cam_shards unless SPT_FLAG_NO_BOUNCE_CULL, in unit mode only (the albedo /
    // emitter instances stay as they are; analytic spheres, tested after the
    // BVH, never come in unit mode), for scenes the Infinity Cache holds
    bool bounce_cull = false;
    // ... and hands each surviving ray's root visit over to the forced drain
    // behind it, which starts the ray below the root instead of repeating the
    // visit (render_fused_kernel's kRoot): with the cull unless
    // SPT_FLAG_NO_ROOT_HANDOFF.  render.cpp uses it where the culling cast is
    // followed at once by the sharded drain of a cached queue
    bool root_handoff = false;
    // the camera cast starts each pixel's rays at the pixel's beam's entry node
    // instead of the root (camera_entry.h): where the camera cast runs, on a
    // tree of 64-B six-wide nodes, under a pinhole camera, unless
    // SPT_FLAG_NO_CAMERA_ENTRY.  The table is 4 B per tile pixel, in the working
    // set beside the film chunk (entry_bytes)
    bool camera_entry = false;
    uint64_t entry_bytes = 0;
};

// fit_limit: UINT64_MAX, or after a working set that could not be allocated
// half the paths that attempt had in flight.
inline RenderPlan plan_render(const RenderPlanIn& in, uint64_t fit_limit) {
    const spt_config& cfg = *in.cfg;
    const uint64_t P = in.P, A = in.A ? in.A : in.P, jobs = A * in.spp;
    RenderPlan pl;
    pl.mode = in.mode;
    bool& fused = pl.fused;
    uint64_t &C = pl.C, &fit_paths = pl.fit_paths, &mem_paths = pl.mem_paths;
    uint32_t& fit_chunk = pl.fit_chunk;
    // Wavefront capacity.  Each isect launch ends in a tail where its last rays
    // finish while most lanes idle, and every iteration pays launch gaps and a
    // shade + refill during which its stream's share of the chip is not
    // tracing; 32M paths in flight (~5 GB of queues: HBM is 288 GB) amortise
    // both.  Config 1, Mpaths/s: 8M 3235, 12M 3470, 16M 3463, 24M 3755,
    // 32M 3715, 48M 3722; configs 2 / 3 / 4: 8M 1712 / 3824 / 851 against
    // 32M 1790 / 4080 / 860.  Default: spt_config.wavefront_paths = 32M.
    // (a render whose working set could not be allocated comes back here with
    // half its paths in flight as the limit: fit_limit)
    C = in.wavefront_paths ? in.wavefront_paths : cfg.wavefront_paths;

    // Pipeline: the wavefront (isect / shade / refill over path queues, the
    // north-star design) or the fused persistent kernel (bit-identical).  The
    // flags choose; else spt_config.pipeline; else (AUTO) by job size: a job of at most
    // two wavefronts is mostly per-cast launch tails on the wavefront (queues
    // shrink cast by cast with no work left to refill them), where the fused
    // kernel's single tail wins — e.g. one rank's 1/8 of the headline image:
    // fused 2308 vs wavefront 1982 Mpaths/s; whole image: 2353 vs 2825.
    // Traversal counters exist in the wavefront isect kernel only.
    const bool trav_stats = pl.trav_stats = (in.flags & SPT_FLAG_TRAVERSAL_STATS) != 0;
    // the job-size rule: the fused kernel up to fused_max_paths = 2^20 paths
    // (fewer than two chip fills of lanes, config 0), the wavefront above: with
    // the drain and the fit rule it carries every tile of config 1 at 1.00-1.05x
    // the fused kernel; an explicit wavefront size moves the rule
    // with it
    const uint64_t fused_max = in.wavefront_paths ? in.wavefront_paths : cfg.fused_max_paths;
    fused = cfg.pipeline == SPT_PIPELINE_AUTO ? jobs <= fused_max : cfg.pipeline == SPT_PIPELINE_FUSED;
    if (in.flags & SPT_FLAG_FUSED) fused = true;
    if ((in.flags & SPT_FLAG_WAVEFRONT) || trav_stats) fused = false;
    if (in.nee) fused = true;  // light sampling: the fused kernel's kNee instances
    // Work order (spt_config.work_order).  AUTO, measured (DESIGN.md §4,
    // profiles/r02_workorder): pixel-major for a scene larger than the
    // Infinity Cache (config 4: +3.8 %; the paths in flight then cover a band
    // of the tile, whose scene working set is smaller); in the fused kernel
    // for tiles of >= 16M paths (config 1 tiles of N = 1 / 2 / 4: +6 / +3 /
    // +2.8 %, N = 8: -1.5 %); in the wavefront for a scene that outgrows an
    // XCD's L2 on a tile of <= 4M pixels, with 24M paths in flight unless
    // set (config 1 +5.5 %); sample-major otherwise (config 3's 16.7M-pixel
    // tile -2.1 %, smallpt's cache-resident scene -4.6 %).
    // A job that fits in flight (spt_config.fit_paths): every path starts in
    // the first refill on fit_streams sub-wavefronts, so its last work item
    // starts at once and the drain finishes it drain_casts casts later.  The
    // per-cast launches then run only while the whole job is in flight, and
    // a render is a handful of launches, which two renders queued on two
    // streams overlap without sub-wavefront streams of their own (DESIGN.md §6:
    // stable at the box's four hardware queues, where four sub-wavefront
    // streams per working set could share a queue with the other set's).
    // A larger job runs as sample chunks that each fit (spt_config.fit_chunks:
    // config 3 +8 %, config 2 +0.9 %, profiles/r05_exp/fit_chunks/).
    // (an explicit paths-in-flight count, in the params or the config, wins)
    // A fitting job's queues, hit records and film chunk must fit in device
    // memory (spt_config.fit_bytes; 0: the free memory plus what this caller's
    // set holds, less 1/16 — processes or scenes sharing the GPU): fit_paths
    // shrinks to what fits, into more sample chunks, and below one chunk of
    // the tile's pixels the job keeps the per-cast wavefront.  Asked only when
    // the set must grow; an allocation that fails all the same (another
    // process took the memory in between) halves the fit and tries again.
    // (the set's streams, below: a caller's null stream gets plain streams and
    // a fitting job one sub-wavefront on them)
    const bool own_queues = pl.own_queues = cfg.sub_queues != 0 && !in.null_caller;
    fit_paths = std::min<uint64_t>(cfg.fit_paths, fit_limit);
    mem_paths = fit_limit;  // paths in flight the memory allows (queues + film chunk)
    // The camera entry table: a pure rule of the config, the tree, the camera
    // and the flag (the render builds none for an empty scene)
    pl.camera_entry = !fused && cfg.lockstep_first >= 2 && in.wide_nodes && in.node6 && in.pinhole &&
                      !(in.flags & SPT_FLAG_NO_CAMERA_ENTRY);
    pl.entry_bytes = pl.camera_entry ? 4ull * P : 0;
    if (fit_paths && !fused) {
        const uint64_t per_path = 2ull * 16 * in.planes + kHitBytes + in.film_unit;
        const uint64_t want = std::min<uint64_t>(fit_paths, jobs) * per_path + pl.entry_bytes;
        // what this render may reuse of the set it will get: the queues and hit
        // records of the sub-wavefronts a fitting job runs on (as allocated,
        // plane padding included) and the film chunk; a sub-wavefront beyond
        // those keeps its buffers and is not counted
        uint64_t held = in.held_film + (pl.camera_entry ? in.held_entry : 0);
        const int kf = own_queues ? (int)cfg.fit_streams : 1;
        for (int k = 0; k < kf && k < kMaxStreams; k++) held += in.held_sub[k];
        uint64_t room = cfg.fit_bytes;
        uint64_t fr = 0;
        if (!room && want > held && in.free_bytes && in.free_bytes(in.free_ctx, &fr)) room = held + fr - fr / 16;
        if (room && want > room) mem_paths = fit_paths = std::max<uint64_t>(1, room / per_path);
    }
    const bool fit_ok = !fused && !in.wavefront_paths && cfg.wavefront_paths == kDefaultWavefrontPaths && fit_paths &&
                        cfg.drain_q8;
    if (fit_ok && jobs > fit_paths && cfg.fit_chunks && A <= fit_paths)
        fit_chunk = (uint32_t)std::min<uint64_t>(in.spp, fit_paths / A);
    const bool fit = pl.fit = fit_ok && (jobs <= fit_paths || fit_chunk != 0);
    const uint64_t scene_bytes = in.device_bytes;
    // (a fitting job of any tile size: pixel-major over scenes beyond an
    // XCD's L2 — config 3's 16.7M-pixel chunks +8 % with it, its per-cast
    // wavefront -2.1 %; smallpt's cache-resident scene -4 % either way)
    const bool wave_pm = !fused && scene_bytes >= kPixelMajorMinWaveSceneBytes && (P <= kPixelMajorMaxWaveTilePx || fit);
    pl.pixel_major =
        cfg.work_order == SPT_WORK_PIXEL_MAJOR ||
        (cfg.work_order == SPT_WORK_AUTO && (scene_bytes >= kPixelMajorMinSceneBytes ||
                                             (fused && jobs >= kPixelMajorMinFusedPaths) || wave_pm));
    // Queue caching (spt_config.queue_cache).  AUTO: non-temporal path-queue
    // and hit accesses for a scene beyond the Infinity Cache, so the caches
    // keep BVH nodes and triangles (config 4 +1.7 %); cached otherwise, where
    // the next kernel still finds the queue's lines (config 2 -3.7 %, config 3
    // -0.7 % streamed; config 1 within noise: profiles/r04_exp2/).
    pl.queue_nt =
        cfg.queue_cache == SPT_QUEUE_CACHE_STREAM ||
        (cfg.queue_cache == SPT_QUEUE_CACHE_AUTO && scene_bytes >= kPixelMajorMinSceneBytes);
    // The drain's refill threshold (spt_config.drain_refill_idle).  AUTO: a
    // wave refills and shades once per batch of free lanes, at a cost that
    // does not depend on how many lanes take part, while a trace step costs
    // in proportion to how long its busiest lane traverses.  With analytic
    // spheres the shade tests them and runs smallpt's mirror / glass, so a
    // pass costs several trace steps and batching more lanes pays (config 2:
    // 56 +20 % over 24); a scene beyond the Infinity Cache (config 4) +3 % at
    // 40; triangle scenes 24 (configs 1, 3, and the mitsuba mesh from 200 to
    // 231k triangles: 56 costs 13-17 %), though closed ones (the tessellated
    // Cornell spheres) gain 1-3 % at 40 (profiles/r06_exp/refill_idle/).
    pl.drain_idle = cfg.drain_refill_idle ? cfg.drain_refill_idle
                    : in.nsph > 0 ? kDrainIdleSpheres
                    : pl.queue_nt ? kDrainIdleStream : kDrainIdleCached;
    if (cfg.work_order == SPT_WORK_AUTO && wave_pm && !in.wavefront_paths && cfg.wavefront_paths == kDefaultWavefrontPaths)
        C = kPixelMajorWavefrontPaths;
    if (fit) C = fit_chunk ? (uint64_t)fit_chunk * A : jobs;
    C = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(C, mem_paths), jobs));
    if (C >= (1ull << 31)) {
        pl.limit = true;
        return pl;
    }
    // The wavefront is split into K sub-wavefronts on their own streams, so one
    // sub-wavefront's launch tail overlaps the others' work.
    // Measured on the headline config: 1 stream 1982, 2: 2649, 3: 2769, 4: 2791 Mpaths/s
    // (4 = the box's hardware queues per process, GPU_MAX_HW_QUEUES).
    // The set's streams get hardware queues of their own (CU-masked streams,
    // spt_config.sub_queues) unless the caller renders on the legacy null
    // stream: CU-masked streams are blocking, and every null-stream operation
    // (the event this render waits for, the one the caller waits on) would
    // wait for them — the other working set's render included — so renders
    // queued there would not overlap.  Such a set uses plain non-blocking
    // streams, which share the process's GPU_MAX_HW_QUEUES, and a fitting job
    // then runs on one sub-wavefront: more would share queues with the other
    // set's and serialise behind them.
    int& K = pl.K = fused ? 1 : fit ? (own_queues ? (int)cfg.fit_streams : 1) : (int)cfg.streams;
    if (fused) C = 64;  // no queues
    if ((uint64_t)K > C) K = (int)C;
    pl.Ck = (C + K - 1) / K;
    // Per-sample contribution film [chunk][P] bytes (unit) or [chunk][3][P]
    // floats, at most film_budget_bytes (4 GiB) per chunk; chunks carry the
    // running sum in acc.  (A chunk's work items are counted in 32 bits: at
    // most 2^31 per chunk.)
    const uint64_t budget = cfg.film_budget_bytes;
    uint32_t& chunk = pl.chunk = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>(std::min<uint64_t>(in.spp, budget / (in.film_unit * P)), 0x7fffffffull / P));
    if (fit_chunk) chunk = std::min(chunk, fit_chunk);  // each chunk fits in flight
    if (mem_paths != UINT64_MAX) chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, mem_paths / P));
    pl.drain_on = cfg.drain_q8 != 0 && !trav_stats;
    pl.lane_xcd = (cfg.xcd_remap & 4u) != 0;
    pl.drain_sort = pl.drain_on && cfg.drain_sort != 0 && in.wide_nodes;
    pl.sort_buffers = !fused && cfg.drain_q8 != 0 && cfg.drain_sort != 0 && in.wide_nodes;
    pl.cam_cast = cfg.lockstep_first >= 2 && in.wide_nodes;
    pl.cam_shards = pl.cam_cast && cfg.lockstep_first >= 3;
    // The bounce cull.  It pays where many bounce rays leave a flat child of
    // the root (a ground plane: config 1 culls 39 % of the camera cast's
    // survivors, +1.8 %; config 3 +3 %) and costs the root visit where none
    // does: config 4's city culls 5 paths of 123M and ran 0.35 % slower with
    // it, so scenes beyond the Infinity Cache (the streamed queue's rule) keep
    // the plain camera cast (profiles/bounce_cull/).
    pl.bounce_cull = pl.cam_shards && !(in.flags & SPT_FLAG_NO_BOUNCE_CULL) && in.mode == 0 && in.nsph == 0 &&
                     scene_bytes < kPixelMajorMinSceneBytes;
    pl.root_handoff = pl.bounce_cull && !(in.flags & SPT_FLAG_NO_ROOT_HANDOFF);
    return pl;
}

}  // namespace spt
