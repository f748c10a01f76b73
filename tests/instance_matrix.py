"""The case matrix: every configuration the launch ladders of csrc/kernels.hip
read, as small named cases, each held to the reference its own feature test uses
(tests/test_gpu_instance_matrix.py runs them; DESIGN.md, parity section).

CASES is the cross product the ladders read, pruned to what is reachable:
tree width x path mode (with and without spheres / kinds, with and without a sky
image) x pipeline (fused, wavefront per cast, short-queue drain, lockstep_first
1 / 2 / 3 with the forced and the short-queue drain, the sorted drain, the cull
and the root hand-off switched off) x queue cache x pass (spt_render,
spt_render_accum, spt_render_accum_list), the samplers with and without MIS, the
isect launches, the AOV pass, and one representative call into each other code
object (denoisers, adapt select, refit, GPU build, camera entry table).

run_case(case) builds the scene, renders or calls, and returns the comparisons:
(label, got, want, tol) with tol None for bit equality.  verify() asserts them.

As a program it runs every case in order and writes each case's begin / end
time stamps, so that a rocprofv3 kernel trace of the run can be cut into cases:

    python tests/instance_matrix.py --out cases.json
    python tests/instance_matrix.py --write-ledger     # traced run -> tests/instance_ledger.json
"""
import argparse
import csv
import ctypes
import functools
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "smallpt-enoki-optix_amd"), os.path.join(ROOT, "oracle"), ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import kernel_inventory as K  # noqa: E402

LEDGER = os.path.join(HERE, "instance_ledger.json")

# Instances no call through include/spt.h can select: mangled name -> the file and
# line of the condition that excludes it.  (The goal is an empty dict.)
ALLOW = {}

# The traced child (traced_run) took 5.8 s on an MI355X, profiler and Python start included
# (the cases themselves 3.2 s): 3 x that for a shared machine, rounded up.
TRACE_LIMIT_S = 20

F = np.float32
W, H, SPP, DEPTH = 24, 20, 3, 4          # 1440 paths: eleven 128-lane blocks and a tail of 32
KW = dict(rr_start_depth=2, env=(0.3, 0.7, 1.0))
SW, SH, SDEPTH = 16, 12, 5               # the samplers' slow numpy restatements: a smaller image
PLANES = ("sum", "sum_sq", "film", "variance")
WIDTHS = (2, 6, 8)
MATS_FUSED = ("unit", "albedo", "albedo_sph", "albedo_env", "albedo_sph_env", "emit", "emit_sph", "emit_env",
              "emit_sph_env")
# the wavefront's kernels read spheres / kinds (kSpt) and the sky image (kSpt, kEnv) one at a time
MATS_WAVE = ("unit", "albedo", "albedo_sph", "albedo_env", "emit", "emit_sph", "emit_env")
PIPES_ANY = ("percast", "queued", "lock1", "lock1s")
PIPES_WIDE = ("lock2", "lock3", "lock3s", "lock3sort")    # the camera cast: wide trees only
PIPES_UNIT = ("lock3noroot", "lock3nocull")               # the cull and the hand-off: unit mode only
SAMPLERS = {
    # name: scene of specular_scenes.variant, sky image, light sampling, sky sampling, share, MIS, env
    "lights": dict(name="specular", tex=False, nee=True, sky=False, share=0.5, mis=False, env=(0.0, 0.0, 0.0)),
    "lights_mis": dict(name="specular", tex=False, nee=True, sky=False, share=0.5, mis=True, env=(0.0, 0.0, 0.0)),
    "lights_env": dict(name="specular", tex=True, nee=True, sky=False, share=0.5, mis=False, env=(0.9, 0.8, 0.7)),
    "lights_env_mis": dict(name="specular", tex=True, nee=True, sky=False, share=0.5, mis=True, env=(0.9, 0.8, 0.7)),
    "sky": dict(name="dark", tex=True, nee=False, sky=True, share=0.5, mis=False, env=(1.0, 1.0, 1.0)),
    "sky_mis": dict(name="dark", tex=True, nee=False, sky=True, share=0.5, mis=True, env=(1.0, 1.0, 1.0)),
    "both": dict(name="specular", tex=True, nee=True, sky=True, share=0.25, mis=False, env=(0.9, 0.8, 0.7)),
    "both_mis": dict(name="specular", tex=True, nee=True, sky=True, share=0.25, mis=True, env=(0.9, 0.8, 0.7)),
}


def _cases():
    out = []

    def add(id, kind, **kw):
        out.append(dict(id=id, kind=kind, **kw))

    for w in WIDTHS:
        for mat in MATS_FUSED:
            for pas in ("render", "list"):
                add(f"w{w}-{mat}-fused-{pas}", "render", width=w, mat=mat, pipe="fused", cache=0, pas=pas)
        for mat in ("unit", "emit_sph"):   # the two plus two full-pass resolve kernels
            for pipe in ("fused", "percast"):
                add(f"w{w}-{mat}-{pipe}-accum", "render", width=w, mat=mat, pipe=pipe, cache=int(pipe != "fused"), pas="accum")
        for mat in ("unit", "albedo_sph", "emit"):
            add(f"w{w}-{mat}-stats-render", "render", width=w, mat=mat, pipe="stats", cache=0, pas="render")
        pipes = PIPES_ANY + (PIPES_WIDE if w != 2 else ())
        for mat in MATS_WAVE:
            for pipe in pipes + (PIPES_UNIT if w != 2 and mat == "unit" else ()):
                for cache, cname in ((1, "c"), (2, "nt")):
                    for pas in ("render", "list"):
                        add(f"w{w}-{mat}-{pipe}-{cname}-{pas}", "render", width=w, mat=mat, pipe=pipe, cache=cache,
                            pas=pas)
        for name in SAMPLERS:
            for pas in ("accum", "list"):
                add(f"w{w}-{name}-{pas}", "sampler", width=w, sampler=name, pas=pas)
        for sph in (False, True):
            add(f"w{w}-aov{'-sph' if sph else ''}", "aov", width=w, spheres=sph)
        add(f"w{w}-isect-lane", "isect", width=w, persistent=0)
        if w != 2:
            add(f"w{w}-isect-persistent", "isect", width=w, persistent=1)
        for entry in ("host", "device"):
            add(f"w{w}-refit-{entry}", "refit", width=w, entry=entry)
    add("hit-info", "hit_info")
    for w, radius in ((6, 16), (8, 8), (6, 32), (8, 64)):   # the PLOC search radius is a template argument
        add(f"w{w}-gpu-build-r{radius}", "gpu_build", width=w, radius=radius)
    add("w6-camera-entry", "camera_entry")
    add("denoise", "denoise")
    add("denoise-var", "denoise_var")
    add("adapt-select", "adapt", base=4)
    add("adapt-select-base0", "adapt", base=0)
    return out


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


# ---------------------------------------------------------------- scenes and references

@functools.lru_cache(maxsize=None)
def mesh():
    from sptamd import scenes
    return scenes.mitsuba_synth(detail=0.25)     # tests/test_gpu_parity.py's `small`


@functools.lru_cache(maxsize=None)
def sky_image():
    import envmap_ref as E
    return E.random_map(8, seed=21), E.rotation((0.4, 1.0, -0.3), 63.0)


@functools.lru_cache(maxsize=None)
def materials(mat):
    """tests/test_gpu_drain.py's materials, one switch at a time."""
    nm = len(mesh()["kd"])
    rng = np.random.default_rng(4)
    out = {}
    if mat == "unit":
        return out
    out["albedo"] = rng.uniform(0.3, 0.95, size=(nm, 3)).astype(F)
    if mat.startswith("emit"):
        emi = np.zeros((nm, 3), F)
        emi[4] = (2.0, 1.5, 1.0)
        out["emission"] = emi
    if "_sph" in mat:
        kinds = np.zeros(nm, np.uint32)
        kinds[2], kinds[3] = 1, 2  # mirror, glass
        out.update(kinds=kinds, spheres=np.array([[0.0, 0.6, 0.0, 0.35], [0.7, 0.3, 0.4, 0.2]], F),
                   sphere_mat=np.array([2, 3], np.int32))
    if mat.endswith("_env"):
        out["envmap"] = sky_image()
    return out


def oracle_scene(mat, emission=True, m=None):
    import oracle as O
    mt = materials(mat)
    return O.OracleScene(mesh() if m is None else m, albedo=mt.get("albedo"),
                         emission=mt.get("emission") if emission else None, spheres=mt.get("spheres"),
                         sphere_mat=mt.get("sphere_mat"), kinds=mt.get("kinds"))


def oparams():
    import oracle as O
    return O.reference_params(W, H, SPP, DEPTH, **KW)


@functools.lru_cache(maxsize=None)
def reference(mat):
    """(planes of accum_ref.moments over the per-sample contributions, film, ray casts or None)."""
    import accum_ref as A
    import envmap_ref as E
    mt = materials(mat)
    p = oparams()
    if "envmap" in mt:
        tex, rot = mt["envmap"]
        x = E.contributions(oracle_scene(mat, emission=False), p, tex, rot,
                            osc_emit=oracle_scene(mat) if "emission" in mt else None)
        planes = dict(zip(PLANES, A.moments(x)))
        return planes, planes["film"], None
    osc = oracle_scene(mat)
    planes = dict(zip(PLANES, A.moments(A.contributions(osc, p))))
    film, casts = osc.render(p)        # the oracle's own film, bit for bit
    np.testing.assert_array_equal(planes["film"], film)
    return planes, film, casts


_scenes = {}


def config(width, **knobs):
    import sptamd
    cfg = sptamd.default_config()
    cfg.bvh_width = width
    cfg.sub_queues = 0      # plain streams: the cached scenes below would each keep hardware queues of their own
    for k, v in knobs.items():
        setattr(cfg, k, v)
    return cfg


def gpu_scene(width, mat):
    """One scene per (width, materials), reconfigured per case (a host build launches no kernel)."""
    import sptamd
    key = (width, mat)
    if key not in _scenes:
        s = sptamd.Scene(config=config(width))
        s.add_arrays(mesh())
        s.commit(0)
        assert s.backend.stats["bvh_width"] == width
        mt = materials(mat)
        if "albedo" in mt:
            s.backend.set_albedo(mt["albedo"])
        if "emission" in mt:
            s.backend.set_emission(mt["emission"])
        if "spheres" in mt:
            s.backend.set_spheres(mt["spheres"], mt["sphere_mat"])
            s.backend.set_material_kinds(mt["kinds"])
        if "envmap" in mt:
            s.backend.set_envmap(*mt["envmap"])
        _scenes[key] = s
    return _scenes[key]


def pipeline(pipe, width, cache):
    """(config, make_params keywords, flags) of a pipeline name."""
    from sptamd import _lib
    knobs, kw, flags = dict(queue_cache=cache), dict(pipeline="wavefront"), 0
    if pipe == "fused":
        kw = dict(pipeline="fused")
    elif pipe in ("percast", "stats"):     # isect / shade / refill per cast over two sub-wavefronts, no drain
        knobs.update(drain_q8=0, streams=2)
        kw["wavefront_paths"] = 500
        if pipe == "stats":
            flags = _lib.SPT_FLAG_TRAVERSAL_STATS
    elif pipe == "queued":                 # ... with the drain taking every short queue
        knobs.update(streams=2)
        kw["wavefront_paths"] = 500
    else:
        # a job that fits in flight; the small persistent grid and drain_q8 = 1 put the drain's
        # threshold below this job's paths, so the first cast runs (render.cpp first_refill)
        knobs.update(lockstep_first=int(pipe[4]), drain_q8=1, isect_grid_q8=16,
                     drain_casts=0 if pipe.endswith("s") else 1, drain_sort=1 if pipe.endswith("sort") else 0)
        if pipe == "lock3noroot":
            flags = _lib.SPT_FLAG_NO_ROOT_HANDOFF
        elif pipe == "lock3nocull":
            flags = _lib.SPT_FLAG_NO_BOUNCE_CULL
    return config(width, **knobs), kw, flags


def listed_pixels(npix):
    return np.flatnonzero(np.arange(npix) % 3 != 1).astype(np.int32)   # 320 of 480: 960 paths, 7.5 blocks


def nan_pattern(n):
    """n float32 quiet NaNs with distinct payloads (compared as bits)."""
    return (0x7FC00000 | (np.arange(n, dtype=np.int64) % 0x3FFFFF + 1)).astype(np.uint32).view(F)


def list_pass(scene, params, npix):
    """One spt_render_accum_list pass at sample_base 0 over listed_pixels into pre-filled planes:
    ({plane: bits (3, npix)}, count, the pre-fill's bits, the pre-filled count, listed mask, stats)."""
    import torch
    from sptamd import _lib
    px = listed_pixels(npix)
    init = nan_pattern(3 * npix)
    count0 = (np.arange(npix) % 5 + 100).astype(np.int32)
    t = {k: torch.from_numpy(init.copy()).cuda() for k in PLANES}
    count = torch.from_numpy(count0.copy()).cuda()
    dev = torch.from_numpy(px).cuda()
    acc = _lib.Accum()
    acc.sample_base = 0
    for k in PLANES:
        setattr(acc, k, t[k].data_ptr())
    pl = _lib.PixelList()
    pl.pixels, pl.n, pl.count = dev.data_ptr(), len(px), count.data_ptr()
    st = _lib.RenderStats()
    scene.backend.sync_config()
    _lib.check(_lib.lib.spt_render_accum_list(scene.backend.handle, ctypes.byref(params), ctypes.byref(acc),
                                              ctypes.byref(pl), ctypes.byref(st), None), "spt_render_accum_list")
    torch.cuda.synchronize()
    listed = np.zeros(npix, bool)
    listed[px] = True
    bits = {k: t[k].cpu().numpy().view(np.uint32).reshape(3, npix) for k in PLANES}
    return bits, count.cpu().numpy(), init.view(np.uint32).reshape(3, npix), count0, listed, scene.backend._stats(st)


def list_checks(scene, params, planes, npix, spp):
    """The listed pixels hold the full pass's planes, the others are untouched."""
    bits, count, init, count0, listed, st = list_pass(scene, params, npix)
    out = []
    for k in PLANES:
        want = np.where(listed[None], np.ascontiguousarray(planes[k]).reshape(3, npix).view(np.uint32), init)
        out.append((f"list {k}", bits[k], want, None))
    out.append(("list count", count, np.where(listed, spp, count0).astype(np.int32), None))
    n = int(listed.sum()) * spp
    out.append(("list paths", np.array([st["paths"], st["paths_started"], st["paths_terminated"],
                                        st["film_slots_unwritten"]]), np.array([n, n, n, 0]), None))
    return out, st


def accum_checks(scene, params, planes, spp):
    import torch
    acc = scene.accumulator(params)
    st = acc.add(spp)
    torch.cuda.synchronize()
    return [(f"accum {k}", getattr(acc, k).cpu().numpy(), planes[k], None) for k in PLANES], st


# ---------------------------------------------------------------- the cases

def run_render(c):
    import sptamd
    import torch
    cfg, kw, flags = pipeline(c["pipe"], c["width"], c["cache"])
    s = gpu_scene(c["width"], c["mat"])
    s.backend.base_config = cfg
    p = sptamd.make_params(W, H, SPP, DEPTH, **KW, **kw)
    p.flags |= flags
    planes, film, casts = reference(c["mat"])
    paths = W * H * SPP
    if c["pas"] == "render":
        got, st = s.render(p)
        torch.cuda.synchronize()
        checks = [("film", got.cpu().numpy(), film, None)]
        if casts is not None:
            checks.append(("ray_casts", np.array(st["ray_casts"]), np.array(casts), None))
        checks.append(("paths", np.array([st["paths_started"], st["paths_terminated"], st["film_slots_unwritten"]]),
                       np.array([paths, paths, 0]), None))
    elif c["pas"] == "accum":
        checks, st = accum_checks(s, p, planes, SPP)
    else:
        checks, st = list_checks(s, p, planes, W * H, SPP)
        paths = int(len(listed_pixels(W * H))) * SPP
    # the pipeline the case names is the one that ran
    pipe = c["pipe"]
    assert st["fused"] == (pipe == "fused"), (pipe, st["fused"])
    if pipe != "fused":
        assert st["queue_cache"] == c["cache"] or pipe == "stats", st["queue_cache"]
    if pipe in ("percast", "stats"):
        assert st["drained_paths"] == 0 and st["drain_launches"] == 0
    if pipe == "stats":
        assert st["isect_nodes"] > 0 or c["width"] == 2 and st["isect_tris"] > 0
    if pipe == "queued":
        assert st["drained_paths"] > 0 and st["lockstep_casts"] == 0
    if pipe.startswith("lock"):
        assert st["lockstep_casts"] == paths, (st["lockstep_casts"], paths)   # the first cast ran in lockstep
        assert st["drain_launches"] > 0
        culls = pipe in ("lock3", "lock3s", "lock3sort", "lock3noroot") and c["mat"] == "unit"
        assert (st["culled_paths"] > 0) == culls, (pipe, st["culled_paths"])
    return checks


@functools.lru_cache(maxsize=None)
def sampler_reference(name):
    """(planes, shadow casts) of the sampler's restatement: nee_ref, sky_ref or mis_ref."""
    import accum_ref as A
    import mis_ref as M
    import nee_ref as R
    import oracle as O
    import sky_ref as S
    import specular_scenes as SS
    c = SAMPLERS[name]
    m, kd, ke, _ = SS.variant(c["name"])
    sky = sky_of(c)
    p = O.reference_params(SW, SH, SPP, SDEPTH, camera=SS.CAM, env=c["env"], rr_start_depth=2)
    count = {}
    if c["mis"]:
        x = M.contributions(m, p, kd, ke, sky=sky, nee=c["nee"], sky_on=c["sky"], share=c["share"], mis=True,
                            count=count)
    elif c["sky"]:
        x = S.contributions(m, p, kd, ke, sky, on=True, nee=c["nee"], share=c["share"], count=count)
    else:
        x = R.contributions(m, p, kd, ke, sky=sky, count=count)
    assert np.isfinite(x).all() and count["shadow_casts"] > 0
    return dict(zip(PLANES, A.moments(x))), count["shadow_casts"]


def sky_of(c):
    if not c["tex"]:
        return None
    from test_gpu_mis import ROT, TEX
    return TEX["sun"], ROT


def run_sampler(c):
    import specular_scenes as SS
    import sptamd
    sm = SAMPLERS[c["sampler"]]
    m, kd, ke, _ = SS.variant(sm["name"])
    s = sptamd.Scene(config=config(c["width"]))
    s.add_arrays(m)
    s.commit(0)
    s.backend.set_albedo(kd)
    s.backend.set_emission(ke)
    if sm["tex"]:
        s.backend.set_envmap(*sky_of(sm))
    if sm["nee"]:
        s.backend.set_light_sampling(True)
    if sm["sky"]:
        s.backend.set_sky_sampling(True, sm["share"])
    if sm["mis"]:
        s.backend.set_mis(True)
    p = sptamd.make_params(SW, SH, SPP, SDEPTH, camera=SS.CAM, env=sm["env"], rr_start_depth=2)
    planes, shadow = sampler_reference(c["sampler"])
    if c["pas"] == "accum":
        checks, st = accum_checks(s, p, planes, SPP)
        checks.append(("shadow_casts", np.array(st["shadow_casts"]), np.array(shadow), None))
    else:
        checks, st = list_checks(s, p, planes, SW * SH, SPP)
        assert st["shadow_casts"] > 0
    assert st["fused"] == 1
    return checks


def run_aov(c):
    import aov_ref
    import oracle as O
    import sptamd
    mat = "albedo_sph" if c["spheres"] else "albedo"
    mt = materials(mat)
    m = dict(mesh(), **{k: mt[k] for k in ("spheres", "sphere_mat", "kinds") if k in mt})
    s = gpu_scene(c["width"], mat)
    s.backend.base_config = config(c["width"])
    hits = aov_ref.first_hits(oracle_scene(mat), O.reference_params(W, H, SPP, DEPTH), range(H))
    assert (hits["id"] != -1).any() and (hits["id"] == -1).any() and (not c["spheres"] or (hits["id"] < -1).any())
    ref = aov_ref.reference_planes(s, m, hits, albedo=mt["albedo"])
    got = aov_ref.gpu_planes(s, sptamd.make_params(W, H, SPP, DEPTH))
    return [(f"aov {k}", got[k], ref[k], None) for k in ("albedo", "normal", "depth", "coverage")]


def random_rays(n, seed):
    """tests/test_gpu_isect.py's rays: random origins in the scene's box, un-normalised directions,
    a block of camera rays."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-2.5, 2.5, size=(3, n)).astype(F)
    o[1] = rng.uniform(-0.9, 3.0, size=n)
    d = rng.normal(size=(3, n)).astype(F)
    d *= rng.uniform(0.2, 3.0, size=n).astype(F)
    o[:, : n // 8] = np.array([[0.0], [3.03], [5.0]], F)
    return o, d


def isect_checks(s, osc, n, seed):
    import sptamd
    import torch
    o, d = random_rays(n, seed)
    rays = sptamd.Ray3.make(o, d)
    got = [a.cpu().numpy() for a in s.backend.intersect_raw(rays)]
    anyh = s.backend.intersect_raw(rays, do_closest=False)[0].cpu().numpy()
    torch.cuda.synchronize()
    rt, rtt, ru, rv = osc.intersect(o, d)
    h = rt >= 0
    assert h.sum() > n // 10
    return [("tri_id", got[0], rt, None), ("t", got[1][h], rtt[h], None), ("u", got[2][h], ru[h], None),
            ("v", got[3][h], rv[h], None), ("any-hit occlusion", anyh >= 0, h, None)]


def run_isect(c):
    s = gpu_scene(c["width"], "unit")
    s.backend.base_config = config(c["width"], public_persistent=c["persistent"], public_refill_idle=8)
    return isect_checks(s, oracle_scene("unit"), 3001, 7)   # 23 blocks and a tail of 57


def run_hit_info(c):
    """tests/test_gpu_isect.py test_hit_info."""
    import sptamd
    import torch
    m = mesh()
    s = gpu_scene(6, "unit")
    s.backend.base_config = config(6)
    o, d = random_rays(3001, 8)
    hit, active = s.backend.intersect(sptamd.Ray3.make(o, d))
    torch.cuda.synchronize()
    tri = hit.tri_id.cpu().numpy()
    h = tri >= 0
    t, u, v = hit.t.cpu().numpy(), hit.barycentric[0].cpu().numpy(), hit.barycentric[1].cpu().numpy()
    pt, nt, nrm, pos = (np.asarray(m[k]) for k in ("pos_tri", "nrm_tri", "nrm", "pos"))
    pt, nt = pt.reshape(-1, 3), nt.reshape(-1, 3)
    ids = tri[h]
    w = (F(1.0) - u[h]) - v[h]
    n0, n1, n2 = (nrm[nt[ids, k]].T for k in range(3))
    p0, p1, p2 = (pos[pt[ids, k]].T for k in range(3))
    gn = np.cross((p1 - p0).T, (p2 - p0).T).T
    gn = gn / np.linalg.norm(gn, axis=0)
    return [("active", active.cpu().numpy(), h, None),
            ("position", hit.position.cpu().numpy()[:, h], (o + t * d)[:, h], None),
            ("shading normal", hit.shading_normal.cpu().numpy()[:, h], (w * n0 + u[h] * n1) + v[h] * n2, None),
            ("geometric normal", hit.geometry_normal.cpu().numpy()[:, h], gn, 2e-5),   # its own test's bound
            ("material", hit.material_id.cpu().numpy()[h], np.asarray(m["mat_id"])[ids], None)]


def run_gpu_build(c):
    import sptamd
    import torch
    from sptamd import _lib
    s = sptamd.Scene(config=config(c["width"], ploc_radius=c["radius"]))
    s.add_arrays(mesh())
    s.commit(0, build=_lib.SPT_BUILD_GPU_PLOC)
    assert s.backend.stats["builder"] == _lib.SPT_BUILD_GPU_PLOC and s.backend.stats["bvh_width"] == c["width"]
    _, film, casts = reference("unit")
    got, st = s.render(sptamd.make_params(W, H, SPP, DEPTH, pipeline="fused", **KW))
    torch.cuda.synchronize()
    return [("film", got.cpu().numpy(), film, None), ("ray_casts", np.array(st["ray_casts"]), np.array(casts), None)] + \
        isect_checks(s, oracle_scene("unit"), 3001, 9)


@functools.lru_cache(maxsize=None)
def moved_mesh():
    """A denser mesh than the renders': the BVH8 refit takes its per-level kernel only for a level of
    more than 1024 nodes (refit.hip kTopLevelNodes)."""
    from sptamd import scenes
    m = dict(scenes.mitsuba_synth(detail=0.5))
    pos = np.asarray(m["pos"], F)
    m["pos"] = (pos + 0.25 * np.sin(3.0 * pos[:, [1, 2, 0]] + F(0.7))).astype(F)
    return m


@functools.lru_cache(maxsize=None)
def moved_reference():
    return oracle_scene("albedo", m=moved_mesh()).render(oparams())


def run_refit(c):
    """tests/test_gpu_refit.py: after the update the film is the oracle's on the new mesh."""
    import sptamd
    import torch
    from sptamd import scenes
    s = sptamd.Scene(config=config(c["width"]))
    s.add_arrays(scenes.mitsuba_synth(detail=0.5))
    s.commit(0)
    s.backend.set_albedo(materials("albedo")["albedo"])
    new = moved_mesh()
    if c["entry"] == "device":
        s.update_geometry(torch.from_numpy(new["pos"]).cuda(), nrm=torch.from_numpy(np.asarray(new["nrm"], F)).cuda())
    else:
        s.update_geometry(new["pos"], nrm=new["nrm"])
    assert s.backend.refit_stats()["updates"] == 1
    film, casts = moved_reference()
    got, st = s.render(sptamd.make_params(W, H, SPP, DEPTH, pipeline="fused", **KW))
    torch.cuda.synchronize()
    return [("film", got.cpu().numpy(), film, None), ("ray_casts", np.array(st["ray_casts"]), np.array(casts), None)] + \
        isect_checks(s, oracle_scene("unit", m=new), 1001, 10)


def run_camera_entry(c):
    """tests/test_gpu_camera_entry.py: with the table and without it, the oracle's film; one table built."""
    import sptamd
    import torch
    from sptamd import _lib
    s = sptamd.Scene(config=pipeline("lock3", 6, 1)[0])
    s.add_arrays(mesh())
    s.commit(0)
    _, film, casts = reference("unit")
    out = []
    for flags, built in ((0, 1), (_lib.SPT_FLAG_NO_CAMERA_ENTRY, 0)):
        p = sptamd.make_params(W, H, SPP, DEPTH, pipeline="wavefront", **KW)
        p.flags |= flags
        before = int(_lib.lib.spt_debug_entry_builds())
        got, st = s.render(p)
        torch.cuda.synchronize()
        assert st["lockstep_casts"] == W * H * SPP
        out += [(f"film flags {flags}", got.cpu().numpy(), film, None),
                (f"ray_casts flags {flags}", np.array(st["ray_casts"]), np.array(casts), None),
                (f"tables built flags {flags}", np.array(int(_lib.lib.spt_debug_entry_builds()) - before),
                 np.array(built), None)]
    return out


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F)).cuda()


def run_denoise(c):
    """tests/test_gpu_denoise.py: |gpu - f64 restatement| <= 8 x max|f32 - f64 restatement|."""
    import denoise_ref as R
    import sptamd
    import torch
    from sptamd import _lib
    d = R.synthetic(seed=9, w=W, h=H)
    p = _lib.default_denoise_params()
    kw = dict(color=d["color"], iterations=3, sigma_color=p.sigma_color, sigma_normal=p.sigma_normal,
              sigma_albedo=p.sigma_albedo, sigma_depth=p.sigma_depth, **{k: d[k] for k in ("normal", "albedo", "depth")})
    tol, r64 = R.tolerance(kw)
    assert tol <= 1e-3 * float(np.abs(d["color"]).max())
    out = sptamd.denoise(_dev(d["color"]), {k: _dev(d[k]) for k in ("normal", "albedo", "depth")}, iterations=3)
    torch.cuda.synchronize()
    return [("denoise", out.cpu().numpy(), r64, tol)]


def run_denoise_var(c):
    """tests/test_gpu_denoise_var.py, the same bound for the colour and the variance plane."""
    import denoise_var_ref as V
    import sptamd
    import torch
    from sptamd import _lib
    d = V.synthetic(seed=9, w=W, h=H)
    p = _lib.default_denoise_var_params()
    kw = dict(color=d["color"], variance=d["variance"], iterations=3, sigma_variance=p.sigma_variance,
              sigma_normal=p.sigma_normal, sigma_albedo=p.sigma_albedo, sigma_depth=p.sigma_depth,
              **{k: d[k] for k in ("normal", "albedo", "depth")})
    (tol_c, tol_v), (c64, v64) = V.tolerance(kw)
    assert tol_c <= 1e-3 * float(np.abs(d["color"]).max())
    out, vout = sptamd.denoise_var(_dev(d["color"]), _dev(d["variance"]),
                                   {k: _dev(d[k]) for k in ("normal", "albedo", "depth")}, iterations=3,
                                   return_variance=True)
    torch.cuda.synchronize()
    return [("denoise_var colour", out.cpu().numpy(), c64, tol_c), ("denoise_var variance", vout.cpu().numpy(), v64, tol_v)]


def run_adapt(c):
    """tests/test_gpu_adaptive.py: spt_adapt_select's ordered list is adaptive_ref.active's."""
    import accum_ref as A
    import adaptive_ref as R
    import sptamd
    import torch
    rule = dict(min_spp=2, max_spp=16, tolerance=0.1, floor=0.03)
    npix, n = 703, c["base"]
    rng = np.random.default_rng(npix)
    x = np.empty((4, 3, 1, npix), F)
    amp = rng.choice(np.array([0.0, 0.05, 0.3, 1.0], F), size=npix)
    x[:] = 0.5 + amp * (rng.random((4, 3, 1, npix), dtype=F) - 0.5)
    s, q, _, _ = A.moments(x)
    s, q = s.reshape(3, npix).copy(), q.reshape(3, npix).copy()
    count = np.full(npix, 4, np.int32)
    count[rng.random(npix) < 0.1] = 2
    s[1, rng.random(npix) < 0.03] = np.nan
    want = np.flatnonzero(R.active(s, q, count, n, **rule)) if n else np.arange(npix)
    assert n == 0 or 0 < len(want) < npix
    lst = sptamd.adapt_select(torch.from_numpy(s).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(count).cuda(), n,
                              **rule)
    torch.cuda.synchronize()
    return [("active list", lst.cpu().numpy(), want.astype(np.int32), None)]


RUNNERS = dict(render=run_render, sampler=run_sampler, aov=run_aov, isect=run_isect, hit_info=run_hit_info,
               gpu_build=run_gpu_build, refit=run_refit, camera_entry=run_camera_entry, denoise=run_denoise,
               denoise_var=run_denoise_var, adapt=run_adapt)


def run_case(case):
    """The case's comparisons: [(label, GPU result, reference result, tol or None for bit equality)]."""
    return RUNNERS[case["kind"]](case)


def verify(case, checks):
    assert checks, case["id"]
    for label, got, want, tol in checks:
        got, want = np.asarray(got), np.asarray(want)
        if tol is None:
            np.testing.assert_array_equal(got, want, err_msg=f"{case['id']}: {label}")
        else:
            assert got.shape == want.shape, (case["id"], label)
            err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
            assert err <= tol, f"{case['id']}: {label}: max error {err:.3e} > {tol:.3e}"


def config_variables():
    """The SPT_* variables that override spt_config (sptamd._lib.config_from_env); the cases set every
    knob they need themselves."""
    from sptamd import _lib
    return [k for k in _lib._ENV_CONFIG if k in os.environ]


def clear_env():
    for k in config_variables():
        del os.environ[k]


# ---------------------------------------------------------------- the traced run and the ledger

def _clocks():
    return {"boot": time.clock_gettime_ns(time.CLOCK_BOOTTIME), "mono": time.clock_gettime_ns(time.CLOCK_MONOTONIC),
            "real": time.time_ns()}


def run_all(out, only=None):
    """Every case in CASES' order, each between two device synchronisations; the time stamps go to
    `out`.  A failed comparison is recorded and the run goes on; any other error ends it at once."""
    import torch
    clear_env()
    torch.cuda.init()
    records, failed, fatal = [], [], None
    t_start = time.time()
    for case in CASES:
        if only and case["id"] not in only:
            continue
        torch.cuda.synchronize()
        rec = {"id": case["id"], "begin": _clocks()}
        try:
            verify(case, run_case(case))
            torch.cuda.synchronize()
        except AssertionError as e:
            rec["error"] = str(e)[:600]
            failed.append(case["id"])
            print(f"FAILED {case['id']}: {rec['error']}", flush=True)
            torch.cuda.synchronize()
        except BaseException as e:  # a HIP error, a fault: nothing more is started on the GPU
            rec["error"] = fatal = f"{type(e).__name__}: {e}"[:600]
            rec["end"] = _clocks()
            records.append(rec)
            print(f"FATAL {case['id']}: {fatal}", flush=True)
            break
        rec["end"] = _clocks()
        records.append(rec)
    doc = {"cases": records, "failed": failed, "fatal": fatal, "seconds": time.time() - t_start}
    with open(out, "w") as f:
        json.dump(doc, f)
    print(f"{len(records)} cases in {doc['seconds']:.1f} s, {len(failed)} failed" + (", ended by an error" if fatal else ""),
          flush=True)
    return 2 if fatal else 1 if failed else 0


def trace_command(tmp, extra=()):
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    return ["timeout", "-k", "10", str(TRACE_LIMIT_S), "rocprofv3", "--kernel-trace", "--mangled-kernels",
            "--output-format", "csv", "-d", tmp, "-o", "run", "--"] + py + \
           [os.path.abspath(__file__), "--out", os.path.join(tmp, "cases.json")] + list(extra)


def traced_run(tmp, extra=()):
    """Start the traced child once (a fresh process, the environment passed on unchanged):
    (exit status or None when rocprofv3 is missing, the end of its output, wall seconds)."""
    t0 = time.time()
    try:
        r = subprocess.run(trace_command(tmp, extra), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except FileNotFoundError as e:
        return None, str(e), time.time() - t0
    return r.returncode, r.stdout[-4000:], time.time() - t0


def read_trace(tmp):
    """(kernel name, start time stamp) of every dispatch in the kernel trace under tmp."""
    files = sorted(glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no kernel trace under {tmp}"
    rows = []
    for path in files:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"]
                rows.append((name[:-3] if name.endswith(".kd") else name, int(r["Start_Timestamp"])))
    return rows


def ledger_from_trace(tmp):
    """({project kernel: sorted case ids that launched it}, [project kernels launched outside every case])
    from the trace and the cases' time stamps.  The profiler's clock is whichever of the host clocks
    brackets the dispatches."""
    with open(os.path.join(tmp, "cases.json")) as f:
        cases = json.load(f)["cases"]
    rows = [(n, t) for n, t in read_trace(tmp) if K.is_project_kernel(n)]
    assert rows and cases, "an empty trace or an empty run"
    lo, hi = min(t for _, t in rows), max(t for _, t in rows)
    clock = [k for k in ("boot", "mono", "real") if cases[0]["begin"][k] <= lo and hi <= cases[-1]["end"][k]]
    assert clock, f"no host clock brackets the trace's time stamps [{lo}, {hi}]: {cases[0]['begin']} .. {cases[-1]['end']}"
    clock = clock[0]
    begins = np.array([c["begin"][clock] for c in cases], np.int64)
    ends = np.array([c["end"][clock] for c in cases], np.int64)
    ledger, outside = {}, []
    for name, t in rows:
        i = int(np.searchsorted(begins, t, side="right")) - 1
        if i < 0 or t > ends[i]:
            outside.append(name)
            continue
        ledger.setdefault(name, set()).add(cases[i]["id"])
    return {k: sorted(v) for k, v in sorted(ledger.items())}, sorted(set(outside))


def load_ledger():
    with open(LEDGER) as f:
        return json.load(f)


def write_ledger(trace_dir=None):
    with tempfile.TemporaryDirectory() as tmp:
        if trace_dir is None:
            status, tail, seconds = traced_run(tmp)
            print(tail)
            print(f"traced run: exit {status}, {seconds:.1f} s")
            if status != 0:
                return 1
            trace_dir = tmp
        ledger, outside = ledger_from_trace(trace_dir)
    assert not outside, f"project kernels launched outside every case: {outside}"
    with open(LEDGER, "w") as f:
        json.dump(ledger, f, indent=0, sort_keys=True)
        f.write("\n")
    missing = sorted(set(K.project_kernels()) - set(ledger) - set(ALLOW))
    print(f"{LEDGER}: {len(ledger)} kernels over {len(CASES)} cases; never launched: {len(missing)}")
    for n in missing:
        print("  " + n)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="run every case and write the cases' time stamps to this file")
    ap.add_argument("--cases", help="comma-separated case ids (default: all)")
    ap.add_argument("--write-ledger", action="store_true", help="trace a run and write tests/instance_ledger.json")
    ap.add_argument("--trace", help="with --write-ledger: a finished traced run's directory instead of a new run")
    ap.add_argument("--list", action="store_true", help="print the case ids")
    a = ap.parse_args()
    if a.list:
        print("\n".join(CASE_IDS))
        return 0
    if a.write_ledger:
        return write_ledger(a.trace)
    if a.out:
        return run_all(a.out, set(a.cases.split(",")) if a.cases else None)
    ap.error("one of --out, --write-ledger, --list")


if __name__ == "__main__":
    sys.exit(main())
