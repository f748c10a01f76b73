"""Multiple importance sampling on the GPU (spt_scene_set_mis): what
the weights cost and what they buy, in one process.

    python tools/mis_bench.py [--calls 9] [--out bench_out/mis]

Three scenes, each with the legs off / sampler / sampler + mis in the fused
pipeline, alternated call by call after one warm-up each:

  nee        tools/nee_bench.py's: cornell_spheres at detail 1.0, smallpt's materials,
             env 0, light sampling
  sky        tools/sky_bench.py's: the mitsuba stand-in at detail 1.0, every albedo 0.8,
             under the 512^2 sky with a sun of 2.5 degrees, sky sampling
  flat_sky   the same scene under a 64^2 sky whose texels lie within 10 % of their
             mean, sky sampling — the case where the sampler alone is worse than off

All 1024^2 x 64 spp, 8 casts, roulette from cast 2.  One JSON line per leg (also
appended to OUT/mis_bench.jsonl): the median frame time of --calls spt_render_accum
passes with min-max, shadow_casts / ray_casts, the image means of the variance
plane and of the film; then a summary line per scene: mis against the sampler
alone in time and variance, and whether ray_casts are the same in all three.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smallpt-enoki-optix_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sptamd  # noqa: E402
from sptamd import _lib, scenes  # noqa: E402
from sky_bench import sun_sky  # noqa: E402

W = 1024
SPP, DEPTH = 64, 8
med = statistics.median


def flat_sky(n=64, seed=5):
    return (1.0 + 0.09 * np.random.default_rng(seed).uniform(-1, 1, size=(n, n, 3))).astype(np.float32)


def make(scene, sampler, mis, size):
    s = sptamd.Scene()
    if scene == "nee":
        mesh = scenes.cornell_spheres(1.0)
        kd, ke = scenes.smallpt_materials(mesh)
        s.add_arrays(mesh)
        s.commit(0)
        s.backend.set_albedo(kd)
        s.backend.set_emission(ke)
        s.backend.set_light_sampling(sampler)
        p = sptamd.make_params(size, size, SPP, DEPTH, camera=scenes.cornell_camera(), env=(0.0, 0.0, 0.0),
                               rr_start_depth=2, pipeline="fused")
    else:
        mesh = scenes.mitsuba_synth(detail=1.0)
        s.add_arrays(mesh)
        s.commit(0)
        s.backend.set_albedo(np.full((max(1, len(mesh.get("kd", [0]))), 3), 0.8, np.float32))
        s.backend.set_envmap(sun_sky(512) if scene == "sky" else flat_sky())
        s.backend.set_sky_sampling(sampler)
        p = sptamd.make_params(size, size, SPP, DEPTH, rr_start_depth=2, pipeline="fused")
    s.backend.set_mis(mis)
    return s, s.accumulator(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9, help="timed repetitions per leg (at least 9)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "mis"))
    ap.add_argument("--size", type=int, default=W, help="image side (the recorded figures use 1024)")
    a = ap.parse_args()
    assert a.calls >= 9, "medians of at least 9"
    assert torch.cuda.is_available(), "mis_bench needs a GPU"
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "mis_bench.jsonl"), "a") as f:
        for scene in ("nee", "sky", "flat_sky"):
            legs = {}
            for name, sampler, mis in (("off", False, False), ("sampler", True, False), ("sampler_mis", True, True)):
                s, acc = make(scene, sampler, mis, a.size)
                legs[name] = dict(scene=s, acc=acc, ms=[], st=None)

            def run(leg):
                leg["acc"].reset()
                t0 = time.perf_counter()
                leg["st"] = leg["acc"].add(SPP)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            for leg in legs.values():
                run(leg)                               # warm-up: working sets, jump tables
            for _ in range(a.calls):
                for leg in legs.values():
                    leg["ms"].append(run(leg))
            recs = {}
            for name, leg in legs.items():
                st, ms = leg["st"], leg["ms"]
                var = float(leg["acc"].variance.cpu().numpy().astype(np.float64).mean())
                rec = {"what": "mis_bench", "scene": scene, "leg": name, "size": [a.size, a.size], "spp": SPP, "depth": DEPTH,
                       "mis": leg["scene"].backend.mis(), "fused": st["fused"],
                       "ms": round(med(ms), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
                       "mpaths": round(a.size * a.size * SPP / (med(ms) * 1e3), 1),
                       "ray_casts": st["ray_casts"], "shadow_casts": st["shadow_casts"],
                       "shadow_per_cast": round(st["shadow_casts"] / st["ray_casts"], 4),
                       "mean_variance": var, "mean_film": float(leg["acc"].film.mean()),
                       "build_id": _lib.lib.spt_build_id().decode()}
                recs[name] = rec
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
            sa, mi, off = recs["sampler"], recs["sampler_mis"], recs["off"]
            rec = {"what": "mis_summary", "scene": scene,
                   "time_ratio_mis_over_sampler": round(mi["ms"] / sa["ms"], 4),
                   "variance_ratio_sampler_over_mis": round(sa["mean_variance"] / mi["mean_variance"], 3),
                   "variance_ratio_off_over_sampler": round(off["mean_variance"] / sa["mean_variance"], 3),
                   "variance_ratio_off_over_mis": round(off["mean_variance"] / mi["mean_variance"], 3),
                   "same_ray_casts": off["ray_casts"] == sa["ray_casts"] == mi["ray_casts"],
                   "shadow_casts_mis_minus_sampler": mi["shadow_casts"] - sa["shadow_casts"], "build_id": mi["build_id"]}
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
            del legs


if __name__ == "__main__":
    main()
