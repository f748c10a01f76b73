"""Refit versus rebuild on the GPU: spt_scene_update_geometry against what it
replaces — spt_scene_create_cfg with the GPU builder on the deformed mesh plus
the setters applied again — in one process on the same meshes.

    python tools/refit_bench.py [--scenes mitsuba,city1m,city10m] [--calls 9] [--out bench_out/refit]

Per scene one JSON line (also appended to OUT/refit_bench.jsonl), medians over
--calls calls after a warm-up, each call with a different deformation:
  refit_ms / update_ms / plan_ms     spt_refit_stats (HIP events; host wall time of the call; once)
  update_ms_device                   update_ms with the arrays already on the device
  rebuild_build_ms / rebuild_wall_ms spt_scene_stats.build_ms of the rebuild; wall time of commit + setters
  refit_gbs                          the two passes' algorithmic bytes over refit_ms: per triangle 36 B of
                                     vertices read, 64 + 48 B written, 64 B re-read; per node the node read
                                     and written, 24 B of box scratch written, 24 B per inner child read
  mpaths_refit / mpaths_fresh        render rate on the refitted tree and on a fresh tree of the same mesh
  area_ratio                         area_now / area_built of that deformation
  equal                              the two renders match bit for bit
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

SCENES = {
    # name: (mesh maker, camera, render (W, H, spp, depth))
    "mitsuba": (lambda: scenes.mitsuba_synth(detail=1.0), None, (1024, 1024, 64, 8)),
    "city1m": (lambda: scenes.city_synth(1_000_000), scenes.city_camera, (1920, 1080, 16, 8)),
    "city10m": (lambda: scenes.city_synth(10_000_000), scenes.city_camera, (1920, 1080, 16, 8)),
}


def deform(pos, phase, amp):
    """The tests' smooth field: pos + amp sin(3 pos[:, [1, 2, 0]] + phase)."""
    return (pos + np.float32(amp) * np.sin(3.0 * pos[:, [1, 2, 0]] + np.float32(phase))).astype(np.float32)


def commit(mesh, albedo):
    cfg = sptamd.default_config()
    cfg.build = _lib.SPT_BUILD_GPU_PLOC
    s = sptamd.Scene(config=cfg)
    s.add_arrays(mesh)
    s.commit(0)
    s.backend.set_albedo(albedo)                    # the setters a rebuild has to apply again
    torch.cuda.synchronize()
    return s


def render_rate(s, p, steps=5):
    film = None
    for _ in range(2):
        film, _ = s.render(p, film=film)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        film, st = s.render(p, film=film)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return st["paths"] / (statistics.median(ms) * 1e3), film.cpu().numpy()


def one(name, calls, amp):
    make, cam, (W, H, spp, depth) = SCENES[name]
    mesh = make()
    pos = np.asarray(mesh["pos"], np.float32)
    nrm = mesh.get("nrm")
    albedo = np.ones((max(1, len(mesh.get("kd", [0]))), 3), np.float32)   # the headline config's unit albedo
    phases = [0.3 + 0.37 * k for k in range(calls + 2)]
    s = commit(mesh, albedo)
    ntri, nodes = s.backend.stats["ntri"], s.backend.stats["nodes"]
    upd, refit = [], []
    for k, ph in enumerate(phases):                 # the first two calls: the plan, a warm-up
        s.update_geometry(deform(pos, ph, amp), nrm)
        rs = s.backend.refit_stats()
        if k >= 2:
            upd.append(rs["update_ms"])
            refit.append(rs["refit_ms"])
    plan_ms, plan_bytes, levels = rs["plan_ms"], rs["plan_bytes"], rs["levels"]
    # the same updates from arrays already on the device (a simulation's output)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()  # noqa: E731
    pt_d, nt_d = up(mesh["pos_tri"], np.int32), None if nrm is None else up(mesh["nrm_tri"], np.int32)
    nrm_d = None if nrm is None else up(nrm, np.float32)
    upd_dev = []
    for k, ph in enumerate(phases):
        pos_d = up(deform(pos, ph, amp), np.float32)
        torch.cuda.synchronize()
        s.update_geometry(pos_d, nrm_d, pos_tri=pt_d, nrm_tri=nt_d)
        if k >= 2:
            upd_dev.append(s.backend.refit_stats()["update_ms"])
    rs = s.backend.refit_stats()
    p = sptamd.make_params(W, H, spp, depth, camera=cam() if cam else None)
    rate_refit, film_refit = render_rate(s, p)
    area_ratio = rs["area_now"] / rs["area_built"]
    del s
    bld, wall = [], []
    fresh = None
    for k, ph in enumerate(phases[1:]):             # the first: a warm-up
        m = dict(mesh)
        m["pos"] = deform(pos, ph, amp)
        fresh = None                                # destroy the old scene, as a caller would
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fresh = commit(m, albedo)
        if k >= 1:
            wall.append((time.perf_counter() - t0) * 1e3)
            bld.append(fresh.backend.stats["build_ms"])
    rate_fresh, film_fresh = render_rate(fresh, p)  # the last rebuild holds the last deformation
    node_bytes = 64 if fresh.backend.stats["bvh_width"] == 6 else (80 if fresh.backend.stats["bvh_width"] == 8 else 64)
    algo = ntri * (36 + 64 + 48 + 64) + nodes * (2 * node_bytes + 24) + (nodes - 1) * 24
    med = statistics.median
    rec = {"scene": name, "ntri": ntri, "nodes": nodes, "levels": levels, "calls": len(upd),
           "refit_ms": round(med(refit), 4), "refit_ms_min_max": [round(min(refit), 4), round(max(refit), 4)],
           "update_ms": round(med(upd), 4), "update_ms_min_max": [round(min(upd), 4), round(max(upd), 4)],
           "update_ms_device": round(med(upd_dev), 4), "plan_ms": round(plan_ms, 3), "plan_bytes": plan_bytes,
           "rebuild_build_ms": round(med(bld), 3), "rebuild_wall_ms": round(med(wall), 3),
           "rebuild_build_ms_min_max": [round(min(bld), 3), round(max(bld), 3)],
           "algo_bytes": algo, "refit_gbs": round(algo / (med(refit) * 1e-3) / 1e9, 1),
           "mpaths_refit": round(rate_refit, 1), "mpaths_fresh": round(rate_fresh, 1),
           "area_ratio": round(area_ratio, 4), "equal": bool(np.array_equal(film_refit, film_fresh)),
           "update_below_build": bool(med(upd) < med(bld)), "build_id": _lib.lib.spt_build_id().decode()}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="mitsuba,city1m")
    ap.add_argument("--calls", type=int, default=9, help="timed calls per scene (at least 7)")
    ap.add_argument("--amp", type=float, default=0.25, help="amplitude of the deformation field")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "refit"))
    a = ap.parse_args()
    assert a.calls >= 7, "medians of at least 7 calls"
    assert torch.cuda.is_available(), "refit_bench needs a GPU"
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "refit_bench.jsonl"), "a") as f:
        for name in a.scenes.split(","):
            f.write(json.dumps(one(name, a.calls, a.amp)) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
