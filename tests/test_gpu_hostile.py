"""The trace kernels on the hostile families of tests/hostile.py: trees that
are deep, span dozens of binades, sit far from the origin or are made of
coincident triangles, for every tree width, builder and child-group packing
of test_gpu_refit.CONFIGS.  The closest hit does not depend on the tree
(DESIGN.md §2), so every record equals the brute-force oracle's bit for bit
(tests/test_hostile_ref.py checks that reference on its own); an any-hit
record is held to be a real point of its triangle in float64; the
traversal-statistics variant confirms that the LDS stack never holds more
entries than the depth of the tree grants it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bvh_audit
import hostile
import oracle as O
import sptamd
import test_gpu_refit as R
import test_hostile_ref as H
import test_scene_cache as C
from sptamd import _lib

pytestmark = pytest.mark.gpu

ALBEDO = np.float32([[0.7, 0.6, 0.5]])
KW = dict(rr_start_depth=3, env=(1.0, 0.9, 0.8))
W, HGT, D = 32, 24, 4
FINITE = tuple(f for f in hostile.FAMILIES if f != "nonfinite")
IDS = [f"w{w}-{'host' if b == R.HOST else 'ploc'}-p{p}" for w, b, p in R.CONFIGS]


@functools.lru_cache(maxsize=None)
def scene(name, cfg):
    """The committed scene of a family for a (width, builder, pack_groups) of R.CONFIGS, built once."""
    s = R.scene(R.config(*cfg), hostile.family(name), with_albedo=False)
    s.backend.set_albedo(ALBEDO)
    return s


@functools.lru_cache(maxsize=None)
def oracle_film(name, spp):
    osc = O.OracleScene(hostile.family(name), albedo=ALBEDO)
    return osc.render(O.reference_params(W, HGT, spp, D, camera=hostile.camera(name), **KW))


def params(name, spp, pipeline=None, flags=0):
    p = sptamd.make_params(W, HGT, spp, D, camera=hostile.camera(name), pipeline=pipeline, **KW)
    p.flags |= flags
    return p


def cast(s, rays, closest=True, n=None):
    o, d, tmin, tmax = (a[..., :n] for a in rays)
    r = sptamd.Ray3.make(np.ascontiguousarray(o), np.ascontiguousarray(d))
    r.tmin.copy_(torch.as_tensor(np.ascontiguousarray(tmin)))
    r.tmax.copy_(torch.as_tensor(np.ascontiguousarray(tmax)))
    out = s.backend.intersect_raw(r, do_closest=closest)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def assert_closest(got, ref, what=""):
    np.testing.assert_array_equal(got[0], ref[0], err_msg=what)
    h = ref[0] >= 0
    for k in (1, 2, 3):
        np.testing.assert_array_equal(got[k][h], ref[k][h], err_msg=f"{what} record {k}")


def assert_any_hit(name, anyh, ref, rays, spans, what=""):
    """Occupancy: a hit exactly where the closest query has one, inside the
    interval and no nearer than the closest.  Genuineness: the record is a real
    intersection of the reported triangle.  That triangle may be any the ray
    crosses, so the closest-hit reference does not hold the record; two checks
    do.  It equals, bit for bit, the watertight test of that ray against that
    triangle alone (hostile.woop_records, a numpy float32 restatement that
    reproduces every closest and any-hit record of the oracle on every family).
    And its float64 residual is within 4 x REF_RESIDUAL, the reference's own
    largest residual over every crossing along the family's rays.  (Measured
    over the closest hits alone that figure does not cover an any-hit's
    choice: on nonfinite, BVH2, a through ray stops at a small triangle far
    down the ray with residual 0.0149 against 0.0013 for the worst closest hit
    of that set; the record passes the bit-for-bit check, and the reference's
    crossings of that set reach 1.06.)"""
    o, d, tmin, tmax = rays
    n = len(anyh[0])
    np.testing.assert_array_equal(anyh[0] >= 0, ref[0][:n] >= 0, err_msg=what)
    h = anyh[0] >= 0
    assert (anyh[1][h] >= tmin[:n][h]).all() and (anyh[1][h] <= tmax[:n][h]).all(), what
    assert (anyh[1][h] >= ref[1][:n][h]).all(), what
    assert anyh[0].max() < len(hostile.family(name)["pos_tri"])
    # the record is the watertight test of that ray and that triangle alone, bit for bit
    inside, t, u, v = hostile.woop_records(hostile.family(name), o[:, :n], d[:, :n], anyh[0])
    assert inside[h].all(), what
    for got, want in zip(anyh[1:], (t, u, v)):
        np.testing.assert_array_equal(got[h], want[h], err_msg=what)
    res = hostile.residual(hostile.family(name), o[:, :n], d[:, :n], *anyh)
    for st, sl in spans.items():
        r = res[sl][h[sl]]
        if len(r):
            print(f"{what} any-hit residual {st}: {r.max():.3g} (reference {H.ref_residual(name, st):.3g})")
            assert np.isfinite(r).all() and r.max() <= 4.0 * H.ref_residual(name, st), (what, st, r.max())


def check_hits(name, cfg):
    rays, spans = hostile.all_rays(name)
    ref = H.brute(name)
    s = scene(name, cfg)
    assert (ref[0] >= 0).sum() > 10000
    assert_closest(cast(s, rays), ref, f"{name} {cfg}")
    assert_any_hit(name, cast(s, rays, closest=False), ref, rays, spans, f"{name} {cfg}")
    return ref


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", R.CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", FINITE)
def test_closest_and_any_hit(name, cfg):
    check_hits(name, cfg)


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=IDS)
def test_nonfinite_family(cfg):
    """NaN, +inf and -inf coordinates in 5 % of the triangles, at creation.
    Read before this ran on a GPU:

    host builder (bvh_build.cpp build_bvh): a triangle's box is fmin / fmax of
    its vertices, so a NaN coordinate drops out unless all three are NaN; an
    all-NaN axis is parked at 0.  Infinite coordinates stay: the centroid is
    +-inf or NaN (inf - inf), the centroid extent inf or NaN.  An extent that
    is not > 0 skips the axis; an infinite one gives scale 0 and f = 0 or NaN,
    and sah_bin sends NaN to bin 0 (the float clamp comes before the
    conversion).  NaN areas lose every `cost < best` comparison, which ends in
    the object-median split.  bvh8_build.cpp gives a non-finite extent the
    widest exponent (127) and clamps every quantised byte NaN-safely.

    GPU builder (gpu_build.hip): tri_box_kernel uses fminf / fmaxf the same
    way (an all-NaN axis stays NaN: no parking).  The centroid bounds go
    through the order-preserving uint map, where a NaN sorts beyond +-inf, so
    morton_kernel's cube may be inf or NaN; t = (c - lo) / cube is then 0 or
    NaN, and fminf(fmaxf(t, 0), 1) brings both to [0, 1] before the
    conversion: the key is in range (most keys are equal, a poor but valid
    order).  No index is out of range.  nn_kernel compared the merged area
    with `a < best` from best = inf, so a cluster with an infinite or NaN area
    never merged and the build ended with hipErrorUnknown once only such
    clusters were left; it now orders those areas as FLT_MAX, after every
    finite one.  dp_kernel and collapse_emit_kernel take inf / NaN costs and
    extents as the host code does.

    The finite triangles answer as the brute-force oracle on the same mesh;
    no ray reports a non-finite triangle."""
    ref = check_hits("nonfinite", cfg)
    bad = np.flatnonzero(~hostile.finite_tris(hostile.family("nonfinite")))
    assert len(bad) == 150
    rays, _ = hostile.all_rays("nonfinite")
    for closest in (True, False):
        assert not np.isin(cast(scene("nonfinite", cfg), rays, closest=closest)[0], bad).any()
    assert not np.isin(ref[0], bad).any()


# 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refill", ["1", "64"])
@pytest.mark.parametrize("cfg", R.CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", ["mixed_scale", "corner_chain", "coincident"])
def test_persistent_lane_refill_kernel(name, cfg, refill, monkeypatch):
    monkeypatch.setenv("SPT_PUBLIC_PERSISTENT", "1")
    monkeypatch.setenv("SPT_PUBLIC_REFILL_IDLE", refill)
    rays, spans = hostile.all_rays(name)
    n = rays[0].shape[1] - 1                                # ragged: not a multiple of the wave
    assert n % 64 != 0
    ref = tuple(a[:n] for a in H.brute(name))
    s = scene(name, cfg)
    assert_closest(cast(s, rays, n=n), ref, f"{name} {cfg} refill {refill}")
    spans = {k: slice(sl.start, min(sl.stop, n)) for k, sl in spans.items()}
    assert_any_hit(name, cast(s, rays, closest=False, n=n), ref, rays, spans, f"{name} {cfg} refill {refill}")


# 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", R.CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", hostile.FAMILIES)
def test_render(name, cfg):
    ref, casts = oracle_film(name, 3)
    s = scene(name, cfg)
    for pipeline in ("fused", "wavefront"):
        f, st = s.render(params(name, 3, pipeline))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(f.cpu().numpy(), ref, err_msg=f"{name} {cfg} {pipeline}")
        assert st["ray_casts"] == casts, (name, cfg, pipeline)
    assert casts > W * HGT * 3                               # the camera sees geometry: paths bounce


# 4 ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def perturbed(name):
    """The family with every vertex moved by a relative 1e-3, and the brute-force hits on it."""
    m = hostile.family(name)
    rng = np.random.default_rng(77)
    pos = np.asarray(m["pos"], np.float32)
    new = (pos * (1.0 + 1e-3 * rng.uniform(-1.0, 1.0, size=pos.shape))).astype(np.float32)
    new.setflags(write=False)
    mesh = dict(m, pos=new)
    o, d, tmin, tmax = hostile.all_rays(name)[0]
    return mesh, O.OracleScene(mesh, use_bvh=False).intersect(o, d, tmin, tmax)


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", ["mixed_scale", "corner_chain"])
def test_refit(name, cfg, tmp_path):
    mesh, ref = perturbed(name)
    s = R.scene(R.config(*cfg), hostile.family(name), with_albedo=False)
    s.update_geometry(mesh["pos"])
    rays, _ = hostile.all_rays(name)
    assert (ref[0] >= 0).sum() > 5000
    assert_closest(cast(s, rays), ref, f"refit {name} {cfg}")
    path = tmp_path / "refit.sptc"
    s.save(str(path))
    bvh_audit.assert_sound(bvh_audit.parse(path), mesh, f"refit {name} {cfg}")


# 5 ------------------------------------------------------------------------------------------
def stack_entries(width, max_depth):
    """capi.cpp: bvh8_stack_entries (depth - 1, at least 1) for the wide trees, max_depth + 1 for the BVH2."""
    return max(1, max_depth + 1) if width == 2 else max(1, max_depth - 1)


@functools.lru_cache(maxsize=None)
def host_depth(name, width):
    cfg = sptamd.default_config()
    cfg.bvh_width = width
    st = _lib.SceneStats()
    tv = hostile.tri_soup(hostile.family(name))
    assert _lib.lib.spt_bvh_build_stats(tv.ctypes.data, tv.shape[0], ctypes.byref(cfg), ctypes.byref(st)) == 0
    return st.max_depth


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", hostile.FAMILIES)
def test_stack_bound_and_statistics_variant(name, cfg):
    """isect_queue_kernel<..., kStats = true>: the same film, and the deepest
    stack entry any lane used is within the entries the tree's depth grants.

    Measured on an MI355X, max_depth / isect_max_stack / entries, the configs
    in R.CONFIGS' order (w8 host p0, w8 host p1, w8 ploc p2, w6 host p2,
    w6 ploc p1, w6 ploc p0, w2 host p1):

    mixed_scale   27/12/26   27/12/26   52/20/51   31/12/30   61/25/60   61/25/60   41/15/42
    corner_chain  17/1/16    17/1/16    17/0/16    23/0/22    24/0/23    24/0/23    25/12/26
    far_small     6/5/5      6/5/5      6/4/5      7/4/6      7/5/6      7/5/6      16/6/17
    coincident    6/4/5      6/4/5      86/1/85    8/6/7      120/2/119  120/2/119  9/9/10
    slivers       8/5/7      8/5/7      8/6/7      9/7/8      10/7/9     10/7/9     19/14/20
    flat_axes     5/2/4      5/2/4      5/3/4      7/2/6      6/3/5      6/3/5      14/2/15
    nonfinite     11/9/10    11/9/10    115/9/114  13/9/12    118/10/117 118/10/117 18/11/19

    (The render's camera sits above corner_chain's plane, where the wide
    tracers reach the leaves from the top levels; the 20 000 rays of
    test_closest_and_any_hit go through the same trees without counters.)"""
    width, build, _ = cfg
    s = scene(name, cfg)
    ref, casts = oracle_film(name, 2)
    plain, _ = s.render(params(name, 2, "wavefront"))
    film, st = s.render(params(name, 2, flags=_lib.SPT_FLAG_TRAVERSAL_STATS))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(film.cpu().numpy(), plain.cpu().numpy())
    np.testing.assert_array_equal(film.cpu().numpy(), ref)
    assert st["ray_casts"] == casts
    depth = s.backend.stats["max_depth"]
    entries = stack_entries(width, depth)
    print(f"stack {name} {IDS[R.CONFIGS.index(cfg)]}: max_depth {depth} isect_max_stack {st['isect_max_stack']} "
          f"entries {entries}")
    assert st["isect_max_stack"] <= entries
    assert st["isect_nodes"] > 0 and st["isect_tris"] > 0
    assert st["isect_lane_steps"] >= st["isect_wave_steps"] > 0
    if build == R.HOST:
        assert depth == host_depth(name, width)             # the same builder, on the CPU
    elif name == "corner_chain":
        # every box holds the smaller ones: PLOC's tree should be a caterpillar too
        assert depth >= host_depth(name, width) / 3.0, (depth, host_depth(name, width))


# 6 ------------------------------------------------------------------------------------------
def test_lds_guard_refuses_a_cache_with_an_impossible_stack(tmp_path):
    """A hand-built cache header (tests/test_scene_cache.py) whose stack_depth
    needs 512 MiB of LDS: spt_scene_load answers SPT_ERR_LIMIT, names the
    depth and leaves no scene.  No tree of that depth is built or traced."""
    secs = C.sections()
    ok = C.write(tmp_path / "ok.sptc", C.header(secs), secs)
    out = ctypes.c_void_p()
    assert _lib.lib.spt_scene_load(ok.encode(), ctypes.byref(out), None, 0, None) == _lib.SPT_OK
    _lib.lib.spt_scene_destroy(out)
    depth = 1 << 20
    p = C.write(tmp_path / "deep.sptc", C.header(secs, stack_depth=depth), secs)
    assert C.info_status(p)[0] == _lib.SPT_OK                # the file itself is well formed
    out = ctypes.c_void_p(0x1234)
    code = _lib.lib.spt_scene_load(p.encode(), ctypes.byref(out), None, 0, None)
    assert code == _lib.SPT_ERR_LIMIT, _lib.lib.spt_last_error()
    assert not out.value
    msg = _lib.lib.spt_last_error().decode()
    assert f"depth {depth}" in msg and "LDS" in msg, msg
