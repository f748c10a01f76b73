"""Every kernel that tests the analytic spheres after the BVH (trace_spheres,
csrc/kernels.hip) on the hostile sphere families of tests/hostile_spheres.py:
256 overlapping spheres, wall spheres of radius 1e2 to 1e5, spheres seen from
1e2 to 3e3 radii away, spheres wholly outside the triangle mesh's bounds,
spheres and no triangles, exact ties.  The public intersect kernel and its
persistent lane-refill variant (closest and any-hit, per-ray intervals), hit
info, the camera cast and the drain / fused lane loop through whole renders,
the AOV kernel, the light and sky shadow rays, and a refitted tree: all equal
the CPU oracle bit for bit (tests/test_hostile_spheres_ref.py checks that
reference against float64 on its own).  Spheres do not depend on the tree, so
one six-wide and one eight-wide entry of test_gpu_refit.CONFIGS stand for all."""
import functools

import numpy as np
import pytest
import torch

import accum_ref as A
import aov_ref
import envmap_ref as E
import hostile
import hostile_spheres as S
import mis_ref
import nee_ref
import oracle as O
import sky_ref
import sptamd
import test_gpu_refit as R
import test_hostile_spheres_ref as H
from sptamd import scenes

pytestmark = pytest.mark.gpu

F = np.float32
CONFIGS = [(8, R.HOST, 0), (6, R.GPU, 1)]
assert all(c in R.CONFIGS for c in CONFIGS)
IDS = [f"w{w}-{'host' if b == R.HOST else 'ploc'}-p{p}" for w, b, p in CONFIGS]
W, HGT, SPP, D = 32, 24, 3, 4
KW = dict(rr_start_depth=3, env=(0.9, 0.7, 0.5))
RENDERED = ("unit256", "walls_1e3", "outside", "alone")


def make_scene(cfg, mesh, **knobs):
    c = R.config(*cfg)
    for k, v in knobs.items():
        setattr(c, k, v)
    s = sptamd.Scene(config=c)
    s.add_arrays(mesh)
    s.commit(0)
    if len(mesh["pos_tri"]):
        assert s.backend.stats["bvh_width"] == cfg[0] and s.backend.stats["builder"] == cfg[1]
    if mesh.get("spheres") is not None:
        s.backend.set_albedo(S.ALBEDO)
        s.backend.set_emission(S.EMISSION)
    else:
        s.backend.set_albedo(S.ALBEDO[:1])
    return s


@functools.lru_cache(maxsize=None)
def scene(name, cfg):
    return make_scene(cfg, S.family(name))


@functools.lru_cache(maxsize=None)
def triangles_alone(name):
    """The closest hits of the family's triangles without its spheres (brute force)."""
    (o, d, tmin, tmax), _ = S.all_rays(name)
    return O.OracleScene(S.without_spheres(S.family(name)), use_bvh=False).intersect(o, d, tmin, tmax)


def cast(s, rays, closest=True, n=None):
    o, d, tmin, tmax = (np.array(a[..., :n]) for a in rays)          # (the families' arrays are read-only)
    r = sptamd.Ray3.make(o, d)
    r.tmin.copy_(torch.as_tensor(tmin))
    r.tmax.copy_(torch.as_tensor(tmax))
    out = s.backend.intersect_raw(r, do_closest=closest)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def assert_closest(got, ref, what):
    np.testing.assert_array_equal(got[0], ref[0], err_msg=what)
    h = ref[0] != -1
    for k in (1, 2, 3):
        np.testing.assert_array_equal(got[k][h], ref[k][h], err_msg=f"{what} record {k}")


def assert_any_hit(name, anyh, rays, what):
    """Where the triangles alone are not hit the any-hit record is the oracle's
    bit for bit: the first sphere in index order that the ray meets in its
    interval.  Where they are, the query stops in the triangle pass, at any
    triangle the ray crosses: a hit inside the interval, no nearer than the
    closest triangle, and its record the watertight test of that ray and that
    triangle alone (hostile.woop_records), bit for bit."""
    o, d, tmin, tmax = rays
    n = len(anyh[0])
    tri = triangles_alone(name)
    ref = tuple(a[:n] for a in H.oracle_hits(name, False, False))
    free = tri[0][:n] == -1
    np.testing.assert_array_equal(anyh[0] != -1, ref[0] != -1, err_msg=what)
    np.testing.assert_array_equal(anyh[0][free], ref[0][free], err_msg=what)
    h = free & (ref[0] != -1)
    for k in (1, 2, 3):
        np.testing.assert_array_equal(anyh[k][h], ref[k][h], err_msg=f"{what} record {k}")
    held = ~free
    assert (anyh[0][held] >= 0).all() and (anyh[0][held] < len(S.family(name)["pos_tri"])).all(), what
    assert (anyh[1][held] >= tmin[:n][held]).all() and (anyh[1][held] <= tmax[:n][held]).all(), what
    assert (anyh[1][held] >= tri[1][:n][held]).all(), what
    if held.any():
        inside, t, u, v = hostile.woop_records(S.family(name), o[:, :n], d[:, :n], np.where(held, anyh[0], -1))
        assert inside[held].all(), what
        for got, want in zip(anyh[1:], (t, u, v)):
            np.testing.assert_array_equal(got[held], want[held], err_msg=what)


def check_hits(name, cfg, n=None, what=""):
    rays, _ = S.all_rays(name)
    ref = H.reference(name)
    assert ((ref[0] < -1).sum() > 4000) and (name in ("alone", "small_far_3e-4") or (ref[0] >= 0).sum() > 20)
    ref = tuple(a[:n] for a in ref)
    s = scene(name, cfg)
    assert_closest(cast(s, rays, n=n), ref, f"{name} {cfg} {what}")
    assert_any_hit(name, cast(s, rays, closest=False, n=n), rays, f"{name} {cfg} {what} any-hit")


# 1 ------------------------------------------------------------------------------------------ public intersect
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", S.FAMILIES + S.BEYOND)
def test_closest_and_any_hit(name, cfg):
    check_hits(name, cfg)
    if name == "tie":
        got = cast(scene(name, cfg), S.all_rays(name)[0], n=5)
        for i, (want_id, want_t) in enumerate(S.TIE_EXPECT):
            assert got[0][i] == want_id and got[1][i] == F(want_t)


@pytest.mark.parametrize("refill", ["1", "64"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", S.FAMILIES + S.BEYOND)
def test_persistent_lane_refill_kernel(name, cfg, refill, monkeypatch):
    """isect_public_persistent_kernel; `alone` reaches its spheres-only branch."""
    monkeypatch.setenv("SPT_PUBLIC_PERSISTENT", "1")
    monkeypatch.setenv("SPT_PUBLIC_REFILL_IDLE", refill)
    n = S.all_rays(name)[0][0].shape[1] - 1                     # ragged: not a multiple of the wave
    assert n % 64 != 0
    check_hits(name, cfg, n=n, what=f"refill {refill}")


# 2 ------------------------------------------------------------------------------------------ hit info
@pytest.mark.parametrize("name", ["unit256", "walls_1e4"])
def test_hit_info_on_sphere_hits(name):
    """Position o + t d, the sphere's material, the normal normalize((o + t d) - c) (include/spt.h)."""
    mesh = S.family(name)
    o, d, tmin, tmax = (np.array(a) for a in S.all_rays(name)[0])
    ref = H.reference(name)
    r = sptamd.Ray3.make(o, d)
    r.tmin.copy_(torch.as_tensor(tmin))
    r.tmax.copy_(torch.as_tensor(tmax))
    hit, active = scene(name, CONFIGS[0]).backend.intersect(r)
    torch.cuda.synchronize()
    ids = hit.tri_id.cpu().numpy()
    np.testing.assert_array_equal(ids, ref[0])
    np.testing.assert_array_equal(active.cpu().numpy(), ref[0] != -1)
    sel = ids < -1
    assert sel.sum() > 10000
    k = -2 - ids[sel]
    if name == "walls_1e4":
        assert (k < 6).sum() > 3000 and (k >= 6).sum() > 1000      # the walls and the spheres in the room
    tt = ref[1][sel]
    p = np.stack([o[i][sel] + tt * d[i][sel] for i in range(3)]).astype(F)
    np.testing.assert_array_equal(hit.position.cpu().numpy()[:, sel], p)
    q = (p - mesh["spheres"][k, :3].T).astype(F)
    with np.errstate(all="ignore"):
        nn = q * (F(1.0) / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]).astype(F)))
    ok = np.isfinite(nn).all(axis=0)
    assert ok.mean() > 0.999
    np.testing.assert_allclose(hit.shading_normal.cpu().numpy()[:, sel][:, ok], nn[:, ok], rtol=0, atol=2e-7)
    np.testing.assert_allclose(hit.geometry_normal.cpu().numpy()[:, sel][:, ok], nn[:, ok], rtol=0, atol=2e-7)
    np.testing.assert_array_equal(hit.material_id.cpu().numpy()[sel], mesh["sphere_mat"][k])
    np.testing.assert_array_equal(hit.texcoord.cpu().numpy()[:, sel], 0)


# 3 ------------------------------------------------------------------------------------------ render
@functools.lru_cache(maxsize=None)
def oracle_film(name, spheres=True, w=W, h=HGT):
    mesh = S.family(name) if spheres else S.without_spheres(S.family(name))
    osc = O.OracleScene(mesh, albedo=S.ALBEDO if spheres else S.ALBEDO[:1], emission=S.EMISSION if spheres else None)
    return osc.render(O.reference_params(w, h, SPP, D, camera=S.camera(name), **KW))


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", RENDERED)
def test_render(name, cfg):
    """The fused lane loop, the wavefront's drain (an image this small goes to it
    whole) and, with the drain off, the shade kernel at every cast: diffuse,
    mirror and glass spheres and an emitting one, the camera inside the room of
    walls_1e3."""
    ref, casts = oracle_film(name)
    kinds = S.KINDS[S.family(name)["sphere_mat"]]
    assert all((kinds == k).any() for k in (0, 1, 2)) and (S.family(name)["sphere_mat"] == S.EMITTER).sum() == 1
    s = scene(name, cfg)
    for kw in (dict(pipeline="fused"), dict(pipeline="wavefront"), dict(pipeline="wavefront", wavefront_paths=500)):
        assert kw.get("wavefront_paths", W * HGT) <= W * HGT
        f, st = s.render(sptamd.make_params(W, HGT, SPP, D, camera=S.camera(name), **KW, **kw))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(f.cpu().numpy(), ref, err_msg=f"{name} {cfg} {kw}")
        assert st["ray_casts"] == casts, (name, cfg, kw)
        assert st["fused"] == (kw["pipeline"] == "fused") and (st["fused"] or st["drained_paths"] > 0)
    f, st = make_scene(cfg, S.family(name), drain_q8=0).render(
        sptamd.make_params(W, HGT, SPP, D, camera=S.camera(name), pipeline="wavefront", **KW))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(f.cpu().numpy(), ref, err_msg=f"{name} {cfg} no drain")
    assert st["ray_casts"] == casts and st["drained_paths"] == 0 and st["fused"] == 0
    assert casts > W * HGT * SPP                                  # paths bounce
    if name == "outside":
        assert not np.array_equal(ref, oracle_film(name, spheres=False)[0])
    if name == "alone":                                           # not the sky alone
        sky = np.broadcast_to(np.array(KW["env"], F)[:, None, None], ref.shape)
        assert (np.abs(ref - sky).max(axis=0) > 1e-3).mean() > 0.2


CW, CH = 50, 37


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", RENDERED)
def test_camera_cast(name, cfg):
    """camera_cast_kernel tests the spheres for the first cast of a job that
    fits in flight and is longer than the drain's threshold: drain_q8 = 1 and
    the 50 x 37 image of tests/test_gpu_bounce_cull.py, the smallest known to
    take it.  (Wide trees only: without triangles there is no camera cast.)"""
    ref, casts = oracle_film(name, w=CW, h=CH)
    s = make_scene(cfg, S.family(name), drain_q8=1, drain_casts=1)
    f, st = s.render(sptamd.make_params(CW, CH, SPP, D, camera=S.camera(name), pipeline="wavefront", **KW))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(f.cpu().numpy(), ref, err_msg=f"{name} {cfg}")
    assert st["ray_casts"] == casts
    if name != "alone":
        assert st["lockstep_casts"] == CW * CH * SPP, st       # the camera cast ran


# 4 ------------------------------------------------------------------------------------------ AOV
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("name", ["outside", "alone"])
def test_aov(name, cfg):
    mesh = S.family(name)
    osc = O.OracleScene(mesh, albedo=S.ALBEDO, emission=S.EMISSION)
    hits = aov_ref.first_hits(osc, O.reference_params(W, HGT, SPP, D, camera=S.camera(name), **KW), range(HGT))
    assert (hits["id"] < -1).sum() > 200 and (hits["id"] == -1).any()
    if name == "outside":
        lo = np.abs(hits["o"] + hits["t"][..., None] * hits["d"]) - S.OUTSIDE_HALF
        assert ((hits["id"] < -1) & (lo.max(axis=-1) > 0)).sum() > 200      # first hits beyond the mesh's bounds
    s = scene(name, cfg)
    ref = aov_ref.reference_planes(s, mesh, hits, albedo=S.ALBEDO)
    got = aov_ref.gpu_planes(s, sptamd.make_params(W, HGT, SPP, D, camera=S.camera(name), **KW))
    for k in ("albedo", "normal", "depth", "coverage"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{name} {cfg} {k}")


# 5 ------------------------------------------------------------------------------------------ shadow rays
# The Cornell box of tests/test_gpu_nee.py seen from further back, and three spheres in front of its open side,
# all wholly outside the mesh's bounding box (z <= 2.9): a diffuse receiver, a sphere between the receiver and the
# ceiling light, and a sphere between the box's floor and the sky's bright texel.
SW, SH, SSPP, SDEPTH = 37, 19, 8, 5
SKW = dict(rr_start_depth=2)
SCAM = dict(scenes.cornell_camera(), look_from=(0.5, 0.52, 4.5), look_at=(0.5, 0.477, 3.5))
ROT = E.rotation((0.4, 1.0, -0.3), 63.0)
PLANES = ("sum", "sum_sq", "film", "variance")
RECEIVER, LIGHT_BLOCK, SKY_BLOCK = (0.5, 0.3, 3.3, 0.15), (0.5, 0.44, 3.0, 0.08), (0.975, 0.865, 3.4, 0.3)
SPHERE_MAT = {RECEIVER: 6, LIGHT_BLOCK: 3, SKY_BLOCK: 1}
SHADOW_CASES = {"lights": dict(nee=True, sky=False, mis=False, env=(0.0, 0.0, 0.0), block=(LIGHT_BLOCK,)),
                "sky": dict(nee=False, sky=True, mis=False, env=(1.0, 1.0, 1.0), block=(SKY_BLOCK,)),
                "both_mis": dict(nee=True, sky=True, mis=True, env=(1.0, 1.0, 1.0), block=(LIGHT_BLOCK, SKY_BLOCK))}


def sun_map():
    """tests/test_gpu_sky.py's map: one texel near 1e3 toward (0.25, 0.35, 1), through the open front."""
    tex = E.random_map(8, 21, bright=0)
    _, fx, fy = E.coords(8, ROT, np.array((0.25, 0.35, 1.0), F))
    tex[int(np.clip(np.rint(fy), 0, 7)), int(np.clip(np.rint(fx), 0, 7))] = (1000.0, 800.0, 600.0)
    return tex


@functools.lru_cache(maxsize=None)
def shadow_scene(case, blocked=True):
    """(mesh, albedo, emission) of a case; blocked=False: without the occluders the case is about."""
    c = SHADOW_CASES[case]
    m = dict(scenes.cornell_spheres(0.05))
    kd, ke = scenes.smallpt_materials(m)
    lo, hi = m["pos"].min(axis=0), m["pos"].max(axis=0)
    sph = [s for s in (RECEIVER, LIGHT_BLOCK, SKY_BLOCK) if blocked or s not in c["block"]]
    for s in sph:                                                 # wholly outside the mesh's bounding box
        assert s[2] - s[3] > hi[2]
    kd = np.concatenate([kd, np.array([[0.6, 0.6, 0.2]], F)])
    ke = np.concatenate([ke if c["nee"] else np.zeros_like(ke), np.zeros((1, 3), F)])
    m["spheres"], m["sphere_mat"] = np.array(sph, F), np.array([SPHERE_MAT[s] for s in sph], np.int32)
    return m, kd, ke


@functools.lru_cache(maxsize=None)
def shadow_expected(case, blocked=True):
    c = SHADOW_CASES[case]
    m, kd, ke = shadow_scene(case, blocked)
    p = O.reference_params(SW, SH, SSPP, SDEPTH, camera=SCAM, env=c["env"], **SKW)
    count = {}
    if case == "lights":
        x = nee_ref.contributions(m, p, kd, ke, count=count)
    elif case == "sky":
        x = sky_ref.contributions(m, p, kd, ke, (sun_map(), ROT), count=count)
    else:
        x = mis_ref.contributions(m, p, kd, ke, sky=(sun_map(), ROT), nee=True, sky_on=True, mis=True, count=count)
    assert np.isfinite(x).all()
    return dict(zip(PLANES, A.moments(x))), count["shadow_casts"]


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("case", list(SHADOW_CASES))
def test_shadow_rays_meet_a_sphere_outside_the_bounds(case, cfg):
    c = SHADOW_CASES[case]
    want, nshadow = shadow_expected(case)
    assert nshadow > 1000
    assert not np.array_equal(want["film"], shadow_expected(case, blocked=False)[0]["film"])   # the spheres do occlude
    m, kd, ke = shadow_scene(case)
    s = sptamd.Scene(config=R.config(*cfg))
    s.add_arrays(m)
    s.commit(0)
    s.backend.set_albedo(kd)
    s.backend.set_emission(ke)
    if c["sky"]:
        s.backend.set_envmap(sun_map(), ROT)
        s.backend.set_sky_sampling(True, 0.5)
    if c["nee"]:
        s.backend.set_light_sampling(True)
    if c["mis"]:
        s.backend.set_mis(True)
    acc = s.accumulator(sptamd.make_params(SW, SH, SSPP, SDEPTH, camera=SCAM, env=c["env"], **SKW))
    st = acc.add(SSPP)
    torch.cuda.synchronize()
    assert st["fused"] == 1 and st["shadow_casts"] == nshadow
    for k in PLANES:
        np.testing.assert_array_equal(getattr(acc, k).cpu().numpy(), want[k], err_msg=f"{case} {cfg} {k}")


# 6 ------------------------------------------------------------------------------------------ refit
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_refit_leaves_the_spheres_outside_the_bounds(cfg):
    """Built five times the size, the mesh's bounds hold every sphere of
    `outside`; update_geometry shrinks it to the family's mesh."""
    mesh = S.family("outside")
    big = dict(mesh, pos=(mesh["pos"] * F(5.0)).astype(F))
    half = np.abs(big["pos"]).max(axis=0)
    sph = mesh["spheres"]
    assert ((np.abs(sph[:, :3]) + sph[:, 3:4]) < half).all(axis=1).sum() >= 20    # inside the bounds as built
    rays, _ = S.all_rays("outside")
    s = make_scene(cfg, big)
    before = cast(s, rays)
    assert_closest(before, O.OracleScene(big, use_bvh=False).intersect(*rays), f"as built {cfg}")
    s.update_geometry(mesh["pos"])
    ref = H.reference("outside")
    assert not np.array_equal(before[0], ref[0])
    assert_closest(cast(s, rays), ref, f"refitted {cfg}")
    assert_any_hit("outside", cast(s, rays, closest=False), rays, f"refitted {cfg} any-hit")
