"""Sky sampling on the GPU (spt_scene_set_sky_sampling): what the
shadow rays cost and what they buy, in one process.

    python tools/sky_bench.py [--calls 9] [--n 512] [--out bench_out/sky]

Scene: config 1's frame — mitsuba_synth at detail 1.0, 1024^2 x 64 spp, 8 casts
— with every albedo 0.8, under an N^2 octahedral sky: a dim blue gradient and
a sun of 2.5 degrees angular radius and radiance 4e3 high in the sky.  Three legs,
alternated call by call after one warm-up each: the wavefront and the fused
pipeline with the switch off, the fused pipeline with it on (the only pipeline
it has).  One JSON line per leg (also appended to OUT/sky_bench.jsonl): the
median frame time of --calls spt_render_accum passes with min-max, shadow_casts
/ ray_casts, the image means of the variance plane and of the film; then a
summary line with the efficiency 1 / (variance x time) of the switch on against
the better leg with it off.
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


def sun_sky(n, sun_dir=(0.35, 0.8, 0.45), radius_deg=2.5, radiance=4.0e3):
    """(n, n, 3) octahedral texels (map frame = world frame, +z the image centre):
    a gradient that is brighter toward +y, and a disc of `radiance` about sun_dir."""
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b = (i + 0.5) / n * 2.0 - 1.0, (j + 0.5) / n * 2.0 - 1.0
    z = 1.0 - np.abs(a) - np.abs(b)
    x = np.where(z < 0, (1.0 - np.abs(b)) * np.where(a < 0, -1.0, 1.0), a)
    y = np.where(z < 0, (1.0 - np.abs(a)) * np.where(b < 0, -1.0, 1.0), b)
    d = np.stack([x, y, z], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    up = 0.5 + 0.5 * d[..., 1]
    tex = np.stack([0.10 + 0.25 * up, 0.15 + 0.35 * up, 0.25 + 0.55 * up], axis=-1)
    s = np.asarray(sun_dir, np.float64)
    s /= np.linalg.norm(s)
    tex[d @ s >= np.cos(np.deg2rad(radius_deg))] = (radiance, 0.9 * radiance, 0.75 * radiance)
    return tex.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9, help="timed repetitions per leg (at least 9)")
    ap.add_argument("--n", type=int, default=512, help="the map's side")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "sky"))
    ap.add_argument("--size", type=int, default=W, help="image side (the recorded figures use 1024)")
    a = ap.parse_args()
    assert a.calls >= 9, "medians of at least 9"
    assert torch.cuda.is_available(), "sky_bench needs a GPU"
    os.makedirs(a.out, exist_ok=True)
    mesh = scenes.mitsuba_synth(detail=1.0)
    albedo = np.full((max(1, len(mesh.get("kd", [0]))), 3), 0.8, np.float32)
    tex = sun_sky(a.n)
    legs = {}
    for name, pipeline, on in (("wavefront_off", "wavefront", False), ("fused_off", "fused", False),
                               ("fused_on", None, True)):
        s = sptamd.Scene()
        s.add_arrays(mesh)
        s.commit(0)
        s.backend.set_albedo(albedo)
        s.backend.set_envmap(tex)
        s.backend.set_sky_sampling(on)
        p = sptamd.make_params(a.size, a.size, SPP, DEPTH, rr_start_depth=2, pipeline=pipeline)
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
    with open(os.path.join(a.out, "sky_bench.jsonl"), "a") as f:
        for name, leg in legs.items():
            st, ms = leg["st"], leg["ms"]
            var = float(leg["acc"].variance.cpu().numpy().astype(np.float64).mean())
            rec = {"what": "sky_bench", "leg": name, "size": [a.size, a.size], "spp": SPP, "depth": DEPTH, "map": a.n,
                   "sun_texels": int((tex[..., 0] > 100).sum()), "cells": leg["scene"].backend.sky_sampling()[2],
                   "fused": st["fused"], "ms": round(med(ms), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
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
        rec = {"what": "sky_summary", "better_off_leg": off,
               "time_ratio_vs_fused_off": round(on["ms"] / recs["fused_off"]["ms"], 3),
               "time_ratio_vs_better_off": round(on["ms"] / recs[off]["ms"], 3),
               "variance_ratio_off_over_on": round(recs[off]["mean_variance"] / on["mean_variance"], 2),
               "efficiency_on_over_off": round(eff, 2), "same_ray_casts": on["ray_casts"] == recs["fused_off"]["ray_casts"],
               "build_id": on["build_id"]}
        print(json.dumps(rec), flush=True)
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
