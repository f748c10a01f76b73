"""Light sampling on the GPU (spt_scene_set_light_sampling): what
the shadow rays cost and what they buy, in one process.

    python tools/nee_bench.py [--calls 9] [--out bench_out/nee]

Scene: cornell_spheres at detail 1.0 with smallpt's materials, 1024^2 x 64 spp,
8 casts, env 0, roulette from cast 2.  Three legs, alternated call by call after
one warm-up each: the fused pipeline with the switch off, the wavefront with it
off, the fused pipeline with it on (the only pipeline it has).  One JSON line
per leg (also appended to OUT/nee_bench.jsonl): the median frame time of --calls
spt_render_accum passes with min-max, shadow_casts / ray_casts, the image mean
of the variance plane; then a summary line with the efficiency 1 / (variance x
time) of the switch on against the better leg with it off.
"""
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
med = statistics.median


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9, help="timed repetitions per leg (at least 9)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "nee"))
    ap.add_argument("--size", type=int, default=W, help="image side (the recorded figures use 1024)")
    a = ap.parse_args()
    assert a.calls >= 9, "medians of at least 9"
    assert torch.cuda.is_available(), "nee_bench needs a GPU"
    os.makedirs(a.out, exist_ok=True)
    mesh = scenes.cornell_spheres(1.0)
    kd, ke = scenes.smallpt_materials(mesh)
    legs = {}
    for name, pipeline, on in (("fused_off", "fused", False), ("wavefront_off", "wavefront", False),
                               ("fused_on", None, True)):
        s = sptamd.Scene()
        s.add_arrays(mesh)
        s.commit(0)
        s.backend.set_albedo(kd)
        s.backend.set_emission(ke)
        s.backend.set_light_sampling(on)
        p = sptamd.make_params(a.size, a.size, SPP, DEPTH, camera=scenes.cornell_camera(), env=(0.0, 0.0, 0.0),
                               rr_start_depth=2, pipeline=pipeline)
        legs[name] = dict(scene=s, acc=s.accumulator(p), ms=[], st=None)

    def run(leg):
        leg["acc"].reset()
        t0 = time.perf_counter()
        leg["st"] = leg["acc"].add(SPP)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for leg in legs.values():
        run(leg)                                   # warm-up: working sets, jump tables
    for _ in range(a.calls):
        for leg in legs.values():
            leg["ms"].append(run(leg))
    recs = {}
    with open(os.path.join(a.out, "nee_bench.jsonl"), "a") as f:
        for name, leg in legs.items():
            st, ms = leg["st"], leg["ms"]
            var = float(leg["acc"].variance.cpu().numpy().astype(np.float64).mean())
            rec = {"what": "nee_bench", "leg": name, "size": [a.size, a.size], "spp": SPP, "depth": DEPTH,
                   "lights": leg["scene"].backend.light_sampling()[1], "fused": st["fused"],
                   "ms": round(med(ms), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
                   "mpaths": round(a.size * a.size * SPP / (med(ms) * 1e3), 1),
                   "ray_casts": st["ray_casts"], "shadow_casts": st["shadow_casts"],
                   "shadow_per_cast": round(st["shadow_casts"] / st["ray_casts"], 4),
                   "mean_variance": var, "mean_film": float(leg["acc"].film.mean()),
                   "build_id": _lib.lib.spt_build_id().decode()}
            recs[name] = rec
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
        off = min(("fused_off", "wavefront_off"), key=lambda k: recs[k]["ms"])
        on = recs["fused_on"]
        eff = (recs[off]["mean_variance"] * recs[off]["ms"]) / (on["mean_variance"] * on["ms"])
        rec = {"what": "nee_summary", "better_off_leg": off, "time_ratio_vs_fused_off": round(on["ms"] / recs["fused_off"]["ms"], 3),
               "time_ratio_vs_better_off": round(on["ms"] / recs[off]["ms"], 3),
               "variance_ratio_off_over_on": round(recs[off]["mean_variance"] / on["mean_variance"], 2),
               "efficiency_on_over_off": round(eff, 2), "same_ray_casts": on["ray_casts"] == recs["fused_off"]["ray_casts"],
               "build_id": on["build_id"]}
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
