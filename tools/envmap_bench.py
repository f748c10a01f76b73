"""What the environment map costs: config 1's frame (mitsuba_synth, 1024^2 x 64
spp, 8 casts) with every albedo 0.8 (albedo mode) under the constant sky, under
an N = 1 map (the special-scene instances with one texel: the routing alone) and
under a 512^2 map (the gather), in one process, the legs interleaved.

    python tools/envmap_bench.py [--calls 9] [--n 512] [--out bench_out/envmap]

One JSON line per leg (also appended to OUT/envmap_bench.jsonl): the median,
minimum and maximum wall ms of --calls renders after a warm-up of each leg, for
the wavefront and the fused pipeline, and the ratio to the constant sky's median."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smallpt-enoki-optix_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sptamd  # noqa: E402
from sptamd import _lib, scenes  # noqa: E402

W = H = 1024
SPP, DEPTH = 64, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9, help="timed repetitions per leg (at least 7)")
    ap.add_argument("--n", type=int, default=512, help="the map's side")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "envmap"))
    a = ap.parse_args()
    assert a.calls >= 7, "medians of at least 7"
    assert torch.cuda.is_available(), "envmap_bench needs a GPU"
    os.makedirs(a.out, exist_ok=True)
    mesh = scenes.mitsuba_synth(detail=1.0)
    s = sptamd.Scene()
    s.add_arrays(mesh)
    s.commit(0)
    s.backend.set_albedo(np.full((max(1, len(mesh.get("kd", [0]))), 3), 0.8, np.float32))
    rng = np.random.default_rng(1)
    big = rng.uniform(0.2, 2.0, size=(a.n, a.n, 3)).astype(np.float32)
    legs = {"constant": None, "map_1": np.ones((1, 1, 3), np.float32), f"map_{a.n}": big}
    with open(os.path.join(a.out, "envmap_bench.jsonl"), "a") as f:
        for pipeline in ("wavefront", "fused"):
            p = sptamd.make_params(W, H, SPP, DEPTH, pipeline=pipeline)
            film = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
            ms = {k: [] for k in legs}
            for rep in range(a.calls + 1):              # the legs alternate; repetition 0 warms each up
                for name, img in legs.items():
                    s.backend.set_envmap(img)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    _, st = s.render(p, film=film)
                    torch.cuda.synchronize()
                    if rep:
                        ms[name].append((time.perf_counter() - t0) * 1e3)
            base = statistics.median(ms["constant"])
            for name in legs:
                m = statistics.median(ms[name])
                rec = {"what": "envmap", "pipeline": pipeline, "leg": name, "ms": round(m, 3),
                       "ms_min_max": [round(min(ms[name]), 3), round(max(ms[name]), 3)],
                       "mpaths": round(W * H * SPP / (m * 1e3), 1), "vs_constant": round(m / base, 4),
                       "calls": a.calls, "build_id": _lib.lib.spt_build_id().decode()}
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
