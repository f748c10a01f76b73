"""Adaptive sampling on the GPU: what a tolerance costs with uniform passes and
with passes over the unconverged pixels only, and what a sparse pass costs
whatever it holds — in one process.

    python tools/adaptive_bench.py [--calls 7] [--max-spp 256] [--out bench_out/adaptive]

One JSON line per measurement (also appended to OUT/adaptive_bench.jsonl),
medians over --calls timed repetitions after a warm-up, on config 1's frame
(mitsuba_synth, 1024^2, 8 casts) in unit mode and with every albedo 0.8:
  schedule   passes of 8, 16, 32, ... samples (doubling, cut at --max-spp) with
             spt_default_adapt_params' tolerance and floor: "uniform" adds every
             pass to every pixel until spt_adapt_select finds none active,
             "adaptive" runs select + spt_render_accum_list.  Total paths, wall
             ms of the whole loop (selection included), passes, the active
             fraction per pass, and the RMSE of each film against one spt_render
             of --ref-spp samples of the same build
  fixed      a sparse pass of one pixel at 8 and at 128 samples (wall ms: the
             launches, the tile-sized film chunk's clear and the resolve, with no
             tracing to speak of), its resolve_ms (SPT_FLAG_TIMING_ALL), the
             resolve_ms of a sparse pass over 1 %, 10 % and all pixels beside the
             plain pass's, and spt_adapt_select alone (HIP events)
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
DEPTH, FIRST = 8, 8
med = statistics.median


def emit(f, rec):
    rec["build_id"] = _lib.lib.spt_build_id().decode()
    print(json.dumps(rec), flush=True)
    f.write(json.dumps(rec) + "\n")
    f.flush()


def pass_sizes(max_spp):
    out, size, base = [], FIRST, 0
    while base < max_spp:
        n = min(size, max_spp - base)
        out.append(n)
        base += n
        size *= 2
    return out


def run_uniform(acc, rule, sizes):
    acc.reset()
    active, paths = [], 0
    npix = acc.count.numel()
    for n in sizes:
        k = npix if acc.samples == 0 else len(sptamd.adapt_select(acc.sum, acc.sum_sq, acc.count, acc.samples, **rule))
        if k == 0:
            break
        active.append(k)
        paths += acc.add(n)["paths"]
    return active, paths


def run_adaptive(acc, rule, sizes):
    acc.reset()
    active, paths = [], 0
    for n in sizes:
        st = acc.add_adaptive(n, **rule)
        if st["active"] == 0:
            break
        active.append(st["active"])
        paths += st["paths"]
    return active, paths


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def bench_schedule(f, s, mode, calls, max_spp, ref_spp):
    d = _lib.default_adapt_params()
    rule = dict(tolerance=d.tolerance, floor=d.floor, min_spp=d.min_spp, max_spp=max_spp)
    sizes = pass_sizes(max_spp)
    ref, _ = s.render(sptamd.make_params(W, H, ref_spp, DEPTH))
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    acc = s.accumulator(sptamd.make_params(W, H, FIRST, DEPTH))
    for name, run in (("uniform", run_uniform), ("adaptive", run_adaptive)):
        run(acc, rule, sizes)                      # warm-up: every pass shape once
        torch.cuda.synchronize()
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            active, paths = run(acc, rule, sizes)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        count = acc.count.cpu().numpy()
        emit(f, {"what": "schedule", "mode": mode, "loop": name, "rule": rule, "pass_sizes": sizes[: len(active)],
                 "passes": len(active), "total_paths": paths, "mean_spp": round(float(count.mean()), 3),
                 "max_count": int(count.max()), "ms": round(med(ms), 3),
                 "ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "mpaths": round(paths / (med(ms) * 1e3), 1),
                 "active_fraction": [round(k / (W * H), 5) for k in active],
                 "rmse_vs_ref": round(rmse(acc.film.cpu().numpy(), ref), 6), "ref_spp": ref_spp})


def bench_fixed(f, s, mode, calls):
    npix = W * H
    p = sptamd.make_params(W, H, FIRST, DEPTH, timing="all")
    acc = s.accumulator(p)
    acc.add(FIRST)
    torch.cuda.synchronize()
    base = acc.samples

    def sparse(pixels, spp):
        """(wall ms, resolve ms) medians of a pass of spp samples over `pixels`, each from the same state."""
        wall, res = [], []
        for k in range(calls + 1):
            acc.samples = base                      # the same pass again: sums of listed pixels drift, timing does not
            t0 = time.perf_counter()
            st = acc.add_list(spp, pixels)
            torch.cuda.synchronize()
            if k:
                wall.append((time.perf_counter() - t0) * 1e3)
                res.append(st["resolve_ms"])
        return med(wall), med(res)

    one = torch.tensor([npix // 2 + W // 2], dtype=torch.int32, device="cuda")
    rec = {"what": "fixed", "mode": mode}
    for spp in (8, 128):
        w, r = sparse(one, spp)
        rec[f"one_pixel_{spp}spp_ms"] = round(w, 4)
        rec[f"one_pixel_{spp}spp_resolve_ms"] = round(r, 4)
    rng = np.random.default_rng(1)
    for frac in (0.01, 0.1, 1.0):
        n = int(npix * frac)
        px = np.arange(npix) if frac == 1.0 else np.sort(rng.choice(npix, size=n, replace=False))
        w, r = sparse(torch.from_numpy(px.astype(np.int32)).cuda(), 8)
        rec[f"list_{frac:g}_8spp_ms"] = round(w, 4)
        rec[f"list_{frac:g}_8spp_resolve_ms"] = round(r, 4)
    plain_w, plain_r = [], []
    for k in range(calls + 1):
        acc.reset()
        t0 = time.perf_counter()
        st = acc.add(8)
        torch.cuda.synchronize()
        if k:
            plain_w.append((time.perf_counter() - t0) * 1e3)
            plain_r.append(st["resolve_ms"])
    rec["plain_8spp_ms"] = round(med(plain_w), 4)
    rec["plain_8spp_resolve_ms"] = round(med(plain_r), 4)
    # the selection alone, on the sums of an 8-sample pass
    lst = torch.empty(npix, dtype=torch.int32, device="cuda")
    scratch = torch.empty(_lib.lib.spt_adapt_select_scratch_bytes(npix), dtype=torch.uint8, device="cuda")
    rule = dict(min_spp=2, max_spp=1024)
    sel, n = [], 0
    for k in range(calls + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        n = sptamd.adapt_select(acc.sum, acc.sum_sq, acc.count, acc.samples, out=lst, scratch=scratch, **rule)
        e1.record()
        torch.cuda.synchronize()
        if k:
            sel.append(e0.elapsed_time(e1))
    rec["select_ms"] = round(med(sel), 4)
    rec["select_active"] = n
    emit(f, rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7, help="timed repetitions (at least 7)")
    ap.add_argument("--max-spp", type=int, default=256)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "adaptive"))
    a = ap.parse_args()
    assert a.calls >= 7, "medians of at least 7"
    assert torch.cuda.is_available(), "adaptive_bench needs a GPU"
    os.makedirs(a.out, exist_ok=True)
    mesh = scenes.mitsuba_synth(detail=1.0)
    s = sptamd.Scene()
    s.add_arrays(mesh)
    s.commit(0)
    with open(os.path.join(a.out, "adaptive_bench.jsonl"), "a") as f:
        for mode in ("unit", "albedo 0.8"):
            if mode != "unit":
                s.backend.set_albedo(np.full((max(1, len(mesh.get("kd", [0]))), 3), 0.8, np.float32))
            bench_schedule(f, s, mode, a.calls, a.max_spp, a.ref_spp)
            bench_fixed(f, s, mode, a.calls)


if __name__ == "__main__":
    main()
