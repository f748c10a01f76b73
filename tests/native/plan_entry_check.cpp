// plan_render's camera entry switch (csrc/render_plan.h RenderPlan::camera_entry)
// on rows of "lockstep_first flags wide_nodes node6 pinhole mode nsph P": one row
// of "fused cam_cast camera_entry entry_bytes" out.  Host-only;
// tests/test_render_plan_entry.py builds it under the sanitizers.  The rest of
// the plan is plan_check.cpp's.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "render_plan.h"

int main() {
    char line[256];
    while (std::fgets(line, sizeof(line), stdin)) {
        unsigned long long c[8];
        int n = 0;
        for (char* t = std::strtok(line, " \t\n"); t && n < 8; t = std::strtok(nullptr, " \t\n"))
            c[n++] = std::strtoull(t, nullptr, 10);
        if (n == 0) continue;
        if (n != 8) {
            std::fprintf(stderr, "plan_entry_check: a row of %d columns, not 8\n", n);
            return 2;
        }
        // config 1's job under the default config's render fields (capi.cpp spt_default_config)
        spt_config cfg{};
        cfg.pipeline = SPT_PIPELINE_AUTO; cfg.fused_max_paths = 1ull << 20; cfg.wavefront_paths = 1u << 25;
        cfg.streams = 4; cfg.sub_queues = 1; cfg.fit_paths = 1ull << 28; cfg.fit_streams = 1; cfg.fit_chunks = 1;
        cfg.drain_q8 = 1024; cfg.xcd_remap = 3; cfg.film_budget_bytes = 4ull << 30;
        cfg.lockstep_first = (uint32_t)c[0];
        spt::RenderPlanIn in;
        in.P = c[7]; in.spp = 64; in.flags = (uint32_t)c[1];
        in.cfg = &cfg;
        in.wide_nodes = c[2] != 0;
        in.node6 = c[3] != 0;
        in.pinhole = c[4] != 0;
        in.mode = (int)c[5];
        in.planes = in.mode == 0 ? 2u : in.mode == 1 ? 3u : 4u;
        in.film_unit = in.mode == 0 ? 1u : 12u;
        in.nsph = (uint32_t)c[6];
        in.device_bytes = 28ull << 20;
        const spt::RenderPlan pl = spt::plan_render(in, UINT64_MAX);
        if (pl.limit) {
            std::fprintf(stderr, "plan_entry_check: the job is over the limit\n");
            return 3;
        }
        std::printf("%d %d %d %llu\n", pl.fused, pl.cam_cast, pl.camera_entry, (unsigned long long)pl.entry_bytes);
    }
    return 0;
}
