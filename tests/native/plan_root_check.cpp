// plan_render's root hand-off switch (csrc/render_plan.h RenderPlan::root_handoff)
// on rows of "lockstep_first flags mode nsph wide_nodes scene_MiB": one row of
// "bounce_cull root_handoff" out.  Host-only; tests/test_render_plan_root.py
// builds it under the sanitizers.  The cull's own switch is
// tests/native/plan_cull_check.cpp's, the rest of the plan plan_check.cpp's.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "render_plan.h"

int main() {
    char line[256];
    while (std::fgets(line, sizeof(line), stdin)) {
        unsigned long long c[6];
        int n = 0;
        for (char* t = std::strtok(line, " \t\n"); t && n < 6; t = std::strtok(nullptr, " \t\n"))
            c[n++] = std::strtoull(t, nullptr, 10);
        if (n == 0) continue;
        if (n != 6) {
            std::fprintf(stderr, "plan_root_check: a row of %d columns, not 6\n", n);
            return 2;
        }
        // config 1's job under the default config's render fields (capi.cpp spt_default_config)
        spt_config cfg{};
        cfg.pipeline = SPT_PIPELINE_AUTO; cfg.fused_max_paths = 1ull << 20; cfg.wavefront_paths = 1u << 25;
        cfg.streams = 4; cfg.sub_queues = 1; cfg.fit_paths = 1ull << 28; cfg.fit_streams = 1; cfg.fit_chunks = 1;
        cfg.drain_q8 = 1024; cfg.xcd_remap = 3; cfg.film_budget_bytes = 4ull << 30;
        cfg.lockstep_first = (uint32_t)c[0];
        spt::RenderPlanIn in;
        in.P = 1u << 20; in.spp = 64; in.flags = (uint32_t)c[1];
        in.cfg = &cfg;
        in.mode = (int)c[2];
        in.planes = in.mode == 0 ? 2u : in.mode == 1 ? 3u : 4u;
        in.film_unit = in.mode == 0 ? 1u : 12u;
        in.device_bytes = c[5] << 20;
        in.nsph = (uint32_t)c[3];
        in.wide_nodes = c[4] != 0;
        const spt::RenderPlan pl = spt::plan_render(in, UINT64_MAX);
        if (pl.limit || pl.fused || !pl.fit) {
            std::fprintf(stderr, "plan_root_check: not a fitting wavefront job\n");
            return 3;
        }
        std::printf("%d %d\n", pl.bounce_cull, pl.root_handoff);
    }
    return 0;
}
