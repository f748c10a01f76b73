"""Progressive rendering on the GPU: what splitting a render into passes costs,
what the moments resolve costs beside the plain one, and spt_denoise_var beside
spt_denoise — in one process.

    python tools/progressive_bench.py [--calls 7] [--out bench_out/progressive]

One JSON line per measurement (also appended to OUT/progressive_bench.jsonl),
medians over --calls timed repetitions after a warm-up:
  passes     config 1 (mitsuba_synth, 1024^2 x 64 spp, 8 casts) as 1, 4, 16 and 64
             spt_render_accum passes queued back to back on one stream (wall time
             to the last pass's end, with and without the second moments),
             against one spt_render of 64 spp; equal: the films match bit for bit
  resolve    resolve_ms (SPT_FLAG_TIMING_ALL) of one 64-spp pass with and without
             the moments, against spt_render's resolve
  denoise    spt_denoise_var against spt_denoise at 1024^2, 5 iterations (HIP events)
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


def timed(fn, calls):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def emit(f, rec):
    rec["build_id"] = _lib.lib.spt_build_id().decode()
    print(json.dumps(rec), flush=True)
    f.write(json.dumps(rec) + "\n")
    f.flush()


def bench_passes(f, s, calls):
    q = sptamd.queue_stream()
    p = sptamd.make_params(W, H, SPP, DEPTH)
    film = torch.empty((3, H, W), dtype=torch.float32, device="cuda")

    def whole():
        s.render(p, film=film, stream=q)

    base = timed(whole, calls)
    ref = film.cpu().numpy()
    emit(f, {"what": "passes", "passes": 0, "api": "spt_render", "ms": round(med(base), 3),
             "ms_min_max": [round(min(base), 3), round(max(base), 3)], "mpaths": round(W * H * SPP / (med(base) * 1e3), 1)})
    for moments in (False, True):
        acc = s.accumulator(p, moments=moments)
        for n in (1, 4, 16, 64):
            def run():
                acc.reset()
                tickets = [acc.add_async(SPP // n, stream=q) for _ in range(n)]
                for t in tickets:
                    acc.wait(t)

            ms = timed(run, calls)
            emit(f, {"what": "passes", "passes": n, "moments": moments, "api": "spt_render_accum",
                     "ms": round(med(ms), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)],
                     "mpaths": round(W * H * SPP / (med(ms) * 1e3), 1), "vs_render": round(med(ms) / med(base), 4),
                     "equal": bool(np.array_equal(acc.film.cpu().numpy(), ref))})


def bench_resolve(f, s, calls):
    p = sptamd.make_params(W, H, SPP, DEPTH, timing="all")
    film = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    for name, unit in (("unit (flag bytes)", True), ("albedo (float film)", False)):
        if not unit:
            alb = np.full((max(1, len(s.mesh.get("kd", [0]))), 3), 0.8, np.float32)
            s.backend.set_albedo(alb)
        plain = []
        for k in range(calls + 1):
            _, st = s.render(p, film=film)
            if k:
                plain.append(st["resolve_ms"])
        rec = {"what": "resolve", "mode": name, "plain_ms": round(med(plain), 4)}
        for moments in (False, True):
            acc = s.accumulator(p, moments=moments)
            ms = []
            for k in range(calls + 1):
                acc.reset()
                st = acc.add(SPP)
                if k:
                    ms.append(st["resolve_ms"])
            rec["accum_moments_ms" if moments else "accum_sum_ms"] = round(med(ms), 4)
        emit(f, rec)


def bench_denoise(f, s, calls):
    p = sptamd.make_params(W, H, 8, DEPTH)
    acc = s.accumulator(p)
    acc.add(8)
    aov = s.render_aov(p)
    torch.cuda.synchronize()
    out = torch.empty_like(acc.film)

    def events(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    plain = events(lambda: sptamd.denoise(acc.film, aov, out=out))
    var = events(lambda: sptamd.denoise_var(acc.film, acc.variance, aov, out=out))
    emit(f, {"what": "denoise", "size": [W, H], "iterations": 5, "denoise_ms": round(med(plain), 4),
             "denoise_var_ms": round(med(var), 4), "ratio": round(med(var) / med(plain), 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7, help="timed repetitions (at least 7)")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "progressive"))
    a = ap.parse_args()
    assert a.calls >= 7, "medians of at least 7"
    assert torch.cuda.is_available(), "progressive_bench needs a GPU"
    os.makedirs(a.out, exist_ok=True)
    s = sptamd.Scene()
    s.add_arrays(scenes.mitsuba_synth(detail=1.0))
    s.commit(0)
    with open(os.path.join(a.out, "progressive_bench.jsonl"), "a") as f:
        bench_passes(f, s, a.calls)
        bench_denoise(f, s, a.calls)
        bench_resolve(f, s, a.calls)


if __name__ == "__main__":
    main()
