// plan_render (csrc/render_plan.h) for listed jobs (RenderPlanIn::A, the pass
// of spt_render_accum_list): the job the plan sizes is A x spp work items,
// while the film chunk keeps a slot per tile pixel.  Self-checking, host only;
// tests/test_render_plan_list.py builds it under the sanitizers.  Prints one
// line per failed check and exits 1, or "ok <checks>".
#include <cstdio>

#include "render_plan.h"

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        g_checks++;                           \
        if (!(cond)) {                        \
            g_failed++;                       \
            std::printf("FAIL %s: ", #cond);  \
            std::printf(__VA_ARGS__);         \
            std::printf("\n");                \
        }                                     \
    } while (0)

// spt_default_config's policy fields (capi.cpp)
static spt_config default_cfg() {
    spt_config c{};
    c.pipeline = SPT_PIPELINE_AUTO;
    c.fused_max_paths = spt::kDefaultFusedMaxPaths;
    c.wavefront_paths = spt::kDefaultWavefrontPaths;
    c.streams = 4;
    c.xcd_remap = 3;
    c.film_budget_bytes = 4ull << 30;
    c.work_order = SPT_WORK_AUTO;
    c.queue_cache = SPT_QUEUE_CACHE_AUTO;
    c.drain_q8 = spt::kDefaultDrainQ8;
    c.drain_casts = spt::kDefaultDrainCasts;
    c.fit_streams = 1;
    c.fit_paths = spt::kDefaultFitPaths;
    c.sub_queues = 1;
    c.lockstep_first = 3;
    c.fit_chunks = 1;
    return c;
}

static spt::RenderPlanIn inputs(const spt_config& cfg, uint64_t P, uint64_t A, uint32_t spp, int mode) {
    spt::RenderPlanIn in;
    in.P = P; in.A = A; in.spp = spp;
    in.cfg = &cfg;
    in.mode = mode;
    in.planes = mode == 0 ? 2u : mode == 1 ? 3u : 4u;
    in.film_unit = mode == 0 ? 1u : 12u;
    in.device_bytes = 64ull << 20;
    in.wide_nodes = true;
    return in;
}

static bool same_plan(const spt::RenderPlan& a, const spt::RenderPlan& b) {
    return a.limit == b.limit && a.fused == b.fused && a.fit == b.fit && a.fit_chunk == b.fit_chunk &&
           a.fit_paths == b.fit_paths && a.mem_paths == b.mem_paths && a.C == b.C && a.K == b.K && a.Ck == b.Ck &&
           a.chunk == b.chunk && a.pixel_major == b.pixel_major && a.queue_nt == b.queue_nt &&
           a.drain_idle == b.drain_idle && a.mode == b.mode && a.own_queues == b.own_queues &&
           a.trav_stats == b.trav_stats && a.drain_on == b.drain_on && a.drain_sort == b.drain_sort &&
           a.sort_buffers == b.sort_buffers && a.lane_xcd == b.lane_xcd && a.cam_cast == b.cam_cast &&
           a.cam_shards == b.cam_shards;
}

int main() {
    const uint64_t Ps[] = {1, 703, 1u << 16, 1u << 20, 1920ull * 1080, 4096ull * 4096, 1ull << 26};
    const uint32_t spps[] = {1, 2, 16, 64, 1024, 4096};
    for (int variant = 0; variant < 6; variant++) {
        spt_config cfg = default_cfg();
        uint32_t flags = 0;
        if (variant == 1) cfg.pipeline = SPT_PIPELINE_WAVEFRONT;
        if (variant == 2) cfg.pipeline = SPT_PIPELINE_FUSED;
        if (variant == 3) { cfg.pipeline = SPT_PIPELINE_WAVEFRONT; cfg.drain_q8 = 0; }
        if (variant == 4) { cfg.work_order = SPT_WORK_PIXEL_MAJOR; cfg.film_budget_bytes = 1u << 20; }
        if (variant == 5) { cfg.fit_paths = 1u << 22; cfg.lockstep_first = 2; flags = SPT_FLAG_WAVEFRONT; }
        for (int mode = 0; mode < 3; mode++)
            for (uint64_t P : Ps)
                for (uint32_t spp : spps) {
                    spt::RenderPlanIn full = inputs(cfg, P, 0, spp, mode);
                    full.flags = flags;
                    spt::RenderPlan pf{};
                    pf = spt::plan_render(full, UINT64_MAX);
                    // a list of every tile pixel: the full pass's plan
                    spt::RenderPlanIn all = full;
                    all.A = P;
                    spt::RenderPlan pa{};
                    pa = spt::plan_render(all, UINT64_MAX);
                    CHECK(pa.limit == pf.limit, "P %llu spp %u", (unsigned long long)P, spp);
                    if (!pf.limit) {
                        CHECK(same_plan(pa, pf), "A = P differs: variant %d mode %d P %llu spp %u", variant, mode,
                              (unsigned long long)P, spp);
                    }
                    const uint64_t As[] = {1, 63, P / 7 + 1, P - 1};
                    for (uint64_t A : As) {
                        if (A == 0 || A > P) continue;
                        spt::RenderPlanIn li = full;
                        li.A = A;
                        const spt::RenderPlan pl = spt::plan_render(li, UINT64_MAX);
                        // the job is A x spp: the decisions of a tile of A pixels
                        spt::RenderPlanIn small = inputs(cfg, A, 0, spp, mode);
                        small.flags = flags;
                        const spt::RenderPlan ps = spt::plan_render(small, UINT64_MAX);
                        CHECK(pl.limit == ps.limit, "limit: P %llu A %llu spp %u", (unsigned long long)P,
                              (unsigned long long)A, spp);
                        if (pl.limit) continue;
                        // (the per-cast wavefront's work order and its 24M paths in flight are
                        // rules about the tile's size: compared when both sizes fall on one side)
                        const bool same_side = (P <= spt::kPixelMajorMaxWaveTilePx) == (A <= spt::kPixelMajorMaxWaveTilePx);
                        CHECK(pl.fused == ps.fused && pl.fit == ps.fit && pl.fit_chunk == ps.fit_chunk && pl.K == ps.K &&
                                  pl.fit_paths == ps.fit_paths, "pipeline and fit");
                        if (same_side)
                            CHECK(pl.C == ps.C && pl.Ck == ps.Ck,
                                  "paths in flight: variant %d mode %d P %llu A %llu spp %u: C %llu/%llu", variant, mode,
                                  (unsigned long long)P, (unsigned long long)A, spp, (unsigned long long)pl.C,
                                  (unsigned long long)ps.C);
                        CHECK(pl.fused ? pl.C == 64 : pl.C <= A * spp, "paths in flight beyond the job");
                        CHECK(pl.cam_cast == ps.cam_cast && pl.cam_shards == ps.cam_shards, "camera cast");
                        // the film chunk: a slot per tile pixel and sample, inside the budget
                        // (one sample always), never more samples than a fitting chunk
                        const uint64_t budget = cfg.film_budget_bytes / ((uint64_t)li.film_unit * P);
                        uint64_t want = std::min<uint64_t>(std::min<uint64_t>(spp, budget), 0x7fffffffull / P);
                        want = std::max<uint64_t>(want, 1);
                        if (pl.fit_chunk) want = std::min<uint64_t>(want, pl.fit_chunk);
                        CHECK(pl.chunk == want, "film chunk %u, want %llu: P %llu A %llu spp %u", pl.chunk,
                              (unsigned long long)want, (unsigned long long)P, (unsigned long long)A, spp);
                        CHECK((uint64_t)pl.chunk * A < (1ull << 31), "a chunk's work items fit 32 bits");
                        if (same_side) CHECK(pl.pixel_major == ps.pixel_major, "work order");
                    }
                }
    }
    // the thresholds by number: a 4096 x 4096 tile at 64 spp is a 2^30-path
    // wavefront job in four fitting chunks; 1000 listed pixels of it are 64 000
    // paths, under fused_max_paths: the fused kernel, film chunk still per tile pixel
    {
        const spt_config cfg = default_cfg();
        const uint64_t P = 4096ull * 4096;
        spt::RenderPlanIn in = inputs(cfg, P, 0, 64, 1);
        const spt::RenderPlan full = spt::plan_render(in, UINT64_MAX);
        CHECK(!full.fused && full.fit && full.fit_chunk == 16 && full.C == 16 * P, "full: fit_chunk %u", full.fit_chunk);
        in.A = 1000;
        const spt::RenderPlan l = spt::plan_render(in, UINT64_MAX);
        CHECK(l.fused && l.K == 1 && l.C == 64, "1000 pixels: fused %d", l.fused);
        CHECK(l.chunk == (4ull << 30) / (12 * P), "chunk %u", l.chunk);  // 21
        in.A = (1u << 20) / 64 + 1;  // one pixel past fused_max_paths / spp
        const spt::RenderPlan w = spt::plan_render(in, UINT64_MAX);
        CHECK(!w.fused && w.fit && w.C == in.A * 64 && w.fit_chunk == 0, "wavefront above the fused rule");
        // 2^31 paths in flight: refused as for a tile
        spt_config big = default_cfg();
        big.fit_paths = 1ull << 40;
        spt::RenderPlanIn bi = inputs(big, 1ull << 26, 1ull << 25, 64, 0);
        CHECK(spt::plan_render(bi, UINT64_MAX).limit, "2^31 listed paths");
        bi.A = (1ull << 25) - 1;
        CHECK(!spt::plan_render(bi, UINT64_MAX).limit, "just below 2^31");
    }
    if (g_failed) return 1;
    std::printf("ok %d\n", g_checks);
    return 0;
}
