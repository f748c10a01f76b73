"""Temporal accumulation on the GPU: what carrying the history across a camera
orbit buys per frame, and what spt_temporal_accumulate costs — in one process.

    python tools/temporal_bench.py [--frames 8] [--calls 7] [--out bench_out/temporal]

One JSON line per measurement (also appended to OUT/temporal_bench.jsonl):
  orbit      config 1's stand-in (mitsuba_synth, 8 casts) at 512^2, 4 spp per
             frame, the camera turned 1 degree per frame about its up axis: per
             frame the rmse to a 1024-spp render of that frame's view of the
             frame's own 4 spp, of the temporal film (default parameters) and
             of spt_denoise_var of the temporal film with the temporal
             variance; the mean history length; denoise_var of the 4 spp alone
             beside them
  kernel     spt_temporal_accumulate at 1024^2 with a moved camera and every
             guide plane (HIP events around --reps back-to-back calls, median
             over --calls windows after a warm-up), the bytes its planes hold
             (36 planes: 23 read, 13 written) over that time, and one
             spt_denoise_var iteration at the same size as the yardstick
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smallpt-enoki-optix_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sptamd  # noqa: E402
from sptamd import _lib, scenes  # noqa: E402

DEPTH, SPP, REF_SPP = 8, 4, 1024
med = statistics.median


def emit(f, rec):
    rec["build_id"] = _lib.lib.spt_build_id().decode()
    print(json.dumps(rec), flush=True)
    f.write(json.dumps(rec) + "\n")
    f.flush()


def orbit(camera, degrees):
    f, a, u = (np.array(camera[k], np.float64) for k in ("look_from", "look_at", "up"))
    u = u / np.linalg.norm(u)
    v, t = f - a, math.radians(degrees)
    v = v * math.cos(t) + np.cross(u, v) * math.sin(t) + u * np.dot(u, v) * (1 - math.cos(t))
    return dict(camera, look_from=tuple(float(x) for x in v + a))


def rmse(a, b):
    return float(torch.sqrt(torch.mean((a.double() - b.double()) ** 2)))


def bench_orbit(f, s, frames, size):
    base = sptamd.reference_camera()
    t = sptamd.TemporalAccumulator(s, sptamd.make_params(size, size, SPP, DEPTH))
    for k in range(frames):
        cam = orbit(base, 1.0 * k)
        t.frame(SPP, camera=cam)
        ref, _ = s.render(sptamd.make_params(size, size, REF_SPP, DEPTH, camera=cam))
        own = t.sum / float(SPP)
        n = float(SPP)
        own_var = torch.clamp(t.sum_sq / n - own * own, min=0.0) / (n - 1.0)
        clean = sptamd.denoise_var(t.film, t.variance, t.aov)
        own_clean = sptamd.denoise_var(own.contiguous(), own_var.contiguous(), t.aov)
        torch.cuda.synchronize()
        emit(f, {"what": "orbit", "frame": k, "size": [size, size], "spp_per_frame": SPP, "ref_spp": REF_SPP,
                 "degrees_per_frame": 1.0, "rmse_own": round(rmse(own, ref), 5), "rmse_temporal": round(rmse(t.film, ref), 5),
                 "rmse_temporal_denoise_var": round(rmse(clean, ref), 5),
                 "rmse_own_denoise_var": round(rmse(own_clean, ref), 5),
                 "mean_history": round(float(t.length.mean()), 3),
                 "restarted_share": round(float((t.length <= SPP).float().mean()), 5) if k else 1.0})


def events(fn, calls, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return ms


def bench_kernel(f, s, calls, reps, size):
    base = sptamd.reference_camera()
    cams = [base, orbit(base, 1.0)]
    p = sptamd.make_params(size, size, SPP, DEPTH)
    t = sptamd.TemporalAccumulator(s, p)
    t.frame(SPP, camera=cams[0])
    prev = {k: getattr(t, k).clone() for k in ("color", "moment2", "length")}
    prev_aov = {k: v.clone() for k, v in t.aov.items()}
    t.frame(SPP, camera=cams[1])
    out = {k: torch.empty_like(v) for k, v in prev.items()}
    out["film"], out["variance"] = torch.empty_like(t.film), torch.empty_like(t.variance)
    torch.cuda.synchronize()

    def temporal():
        sptamd.temporal_accumulate(t.sum, t.sum_sq, t.aov, cams[1], prev=prev, prev_aov=prev_aov, prev_camera=cams[0],
                                   samples=SPP, out=out)

    dout = torch.empty_like(t.film)
    ms_t = events(temporal, calls, reps)
    ms_d = events(lambda: sptamd.denoise_var(t.film, t.variance, t.aov, iterations=1, out=dout), calls, reps)
    planes = 36 * size * size * 4
    emit(f, {"what": "kernel", "size": [size, size], "reps_per_window": reps, "windows": calls,
             "temporal_ms": round(med(ms_t), 5), "temporal_ms_min_max": [round(min(ms_t), 5), round(max(ms_t), 5)],
             "plane_bytes": planes, "plane_gb_per_s": round(planes / (med(ms_t) * 1e6), 1),
             "denoise_var_1_iteration_ms": round(med(ms_d), 5),
             "denoise_var_ms_min_max": [round(min(ms_d), 5), round(max(ms_d), 5)],
             "ratio": round(med(ms_t) / med(ms_d), 3),
             "note": "both include the Python call and launch overhead of each call; denoise_var with iterations = 1 "
                     "is its variance-init launch, one a-trous launch and a scratch allocation from torch's cache"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--calls", type=int, default=7, help="timed windows (at least 7)")
    ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
    ap.add_argument("--orbit-size", type=int, default=512)
    ap.add_argument("--kernel-size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "temporal"))
    a = ap.parse_args()
    assert a.calls >= 7, "medians of at least 7"
    assert torch.cuda.is_available(), "temporal_bench needs a GPU"
    os.makedirs(a.out, exist_ok=True)
    s = sptamd.Scene()
    s.add_arrays(scenes.mitsuba_synth(detail=1.0))
    s.commit(0)
    with open(os.path.join(a.out, "temporal_bench.jsonl"), "a") as f:
        bench_kernel(f, s, a.calls, a.reps, a.kernel_size)
        bench_orbit(f, s, a.frames, a.orbit_size)


if __name__ == "__main__":
    main()
