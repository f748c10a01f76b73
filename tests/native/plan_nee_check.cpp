// plan_render's light-sampling input (csrc/render_plan.h RenderPlanIn::nee) on
// tests/native/plan_check.cpp's rows with one more column in front: "nee" and
// then plan_check's 34 inputs in, plan_check's row of decisions out.  With
// nee = 0 the output must be plan_check's; with nee = 1 the plan must be the
// fused pipeline whatever the rest says.  Host-only; tests/test_render_plan_nee.py
// builds it under the sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "render_plan.h"

struct FreeMemory {
    bool known;
    uint64_t bytes;
    unsigned long long queries;
};
static bool free_memory(void* ctx, uint64_t* out) {
    FreeMemory* f = (FreeMemory*)ctx;
    f->queries++;
    if (f->known) *out = f->bytes;
    return f->known;
}

int main() {
    constexpr int kIn = 35;
    char line[4096];
    while (std::fgets(line, sizeof(line), stdin)) {
        unsigned long long c[kIn];
        int n = 0;
        for (char* t = std::strtok(line, " \t\n"); t && n < kIn; t = std::strtok(nullptr, " \t\n"))
            c[n++] = std::strtoull(t, nullptr, 10);
        if (n == 0) continue;
        if (n != kIn) {
            std::fprintf(stderr, "plan_nee_check: a row of %d columns, not %d\n", n, kIn);
            return 2;
        }
        spt_config cfg{};
        spt::RenderPlanIn in;
        int i = 0;
        in.nee = c[i++] != 0;
        in.P = c[i++]; in.spp = (uint32_t)c[i++]; in.flags = (uint32_t)c[i++]; in.wavefront_paths = (uint32_t)c[i++];
        cfg.pipeline = (uint32_t)c[i++]; cfg.fused_max_paths = c[i++]; cfg.wavefront_paths = (uint32_t)c[i++];
        cfg.streams = (uint32_t)c[i++]; cfg.sub_queues = (uint32_t)c[i++]; cfg.fit_paths = c[i++];
        cfg.fit_streams = (uint32_t)c[i++]; cfg.fit_bytes = c[i++]; cfg.fit_chunks = (uint32_t)c[i++];
        cfg.drain_q8 = (uint32_t)c[i++]; cfg.drain_sort = (uint32_t)c[i++]; cfg.lockstep_first = (uint32_t)c[i++];
        cfg.xcd_remap = (uint32_t)c[i++]; cfg.work_order = (uint32_t)c[i++]; cfg.queue_cache = (uint32_t)c[i++];
        cfg.drain_refill_idle = (uint32_t)c[i++]; cfg.film_budget_bytes = c[i++];
        in.cfg = &cfg;
        in.mode = (int)c[i++];
        in.planes = in.mode == 0 ? 2u : in.mode == 1 ? 3u : 4u;
        in.film_unit = in.mode == 0 ? 1u : 12u;
        in.device_bytes = c[i++]; in.nsph = (uint32_t)c[i++]; in.wide_nodes = c[i++] != 0; in.null_caller = c[i++] != 0;
        for (int k = 0; k < spt::kMaxStreams; k++) in.held_sub[k] = c[i++];
        in.held_film = c[i++];
        FreeMemory fm{c[i] != 0, c[i + 1], 0};
        i += 2;
        in.free_bytes = free_memory;
        in.free_ctx = &fm;
        const uint64_t fit_limit = c[i++];
        spt::RenderPlan pl = spt::plan_render(in, fit_limit);
        if (pl.limit) {  // as plan_check: only the limit, fit_paths and the refused C are decided
            const uint64_t fit_paths = pl.fit_paths, C = pl.C;
            pl = spt::RenderPlan{};
            pl.limit = true; pl.fit_paths = fit_paths; pl.C = C;
            pl.chunk = 0; pl.K = 0;
        }
        std::printf("%d %d %d %u %llu %llu %llu %d %llu %u %u %u %u %d %d %d %d %d %d %d %d %d %llu\n", pl.limit, pl.fused,
                    pl.fit, pl.fit_chunk, (unsigned long long)pl.fit_paths, (unsigned long long)pl.mem_paths,
                    (unsigned long long)pl.C, pl.K, (unsigned long long)pl.Ck, pl.chunk, pl.pixel_major, pl.queue_nt,
                    pl.drain_idle, pl.mode, pl.own_queues, pl.drain_on, pl.drain_sort, pl.sort_buffers, pl.cam_cast,
                    pl.cam_shards, pl.lane_xcd, pl.trav_stats, fm.queries);
    }
    return 0;
}
