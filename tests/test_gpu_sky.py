"""Sky sampling on the GPU (spt_scene_set_sky_sampling): the planes
of a render with the switch on are the CPU restatement's (tests/sky_ref.py over
the oracle's paths) bit for bit — the Cornell scene lit by the sky alone and
with its cap emitting beside light sampling (the share), in every tree width
and builder, both work orders, with a mirror material, with analytic spheres,
under a thin lens and a tint, and a scene without any emission table; an empty
table, no map or the switch off is the parent's path; the accumulator's splits,
pixel lists, tiles and queued renders; set_envmap afterwards; the counters; the
refusals; the LDS guard; the command-line host; and, statistically, the same
expectation with less variance."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import accum_ref as A
import envmap_ref as E
import hostile
import oracle as O
import sky_ref as S
import sptamd
from sptamd import _lib, scenes
from test_accum_ref import mode_scene

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, DEPTH = 37, 19, 8, 5
DETAIL = 0.05
CAM = scenes.cornell_camera()
KW = dict(rr_start_depth=2)
PLANES = ("sum", "sum_sq", "film", "variance")
ROT = E.rotation((0.4, 1.0, -0.3), 63.0)
ONE = (1.0, 1.0, 1.0)
CLI = os.path.join(os.path.dirname(_lib.LIB_PATH), "spt_render_cli")
# test_sky_sampling_lowers_the_variance: measured once on an MI355X, see there
MEASURED_VARIANCE_RATIO = 8.80


def sun_map(seed, toward):
    """random_map(8) without its own bright texels, and one texel near 1e3: the one whose
    centre is nearest the world direction `toward` under ROT."""
    tex = E.random_map(8, seed, bright=0)
    _, fx, fy = E.coords(8, ROT, np.array(toward, F))
    i, j = int(np.clip(np.rint(fx), 0, 7)), int(np.clip(np.rint(fy), 0, 7))
    tex[j, i] = (1000.0, 800.0, 600.0)
    return tex


TEX = sun_map(21, (0.25, 0.35, 1.0))     # through the Cornell box's open front, up and to the right
TEX2 = sun_map(22, (-0.3, 0.2, 1.0))
TEX_M = sun_map(23, (0.3, 1.0, 0.4))     # above the mitsuba stand-in


@functools.lru_cache(maxsize=None)
def cornell():
    m = scenes.cornell_spheres(DETAIL)
    kd, ke = scenes.smallpt_materials(m)
    return m, kd, ke


def variant(name):
    """(mesh, albedo, emission) of the named scene."""
    m, kd, ke = cornell()
    m = dict(m)
    if name == "skyonly":                        # the cap dark: the sky is the only light
        ke = np.zeros_like(ke)
    elif name == "mirror":
        kinds = np.zeros(len(kd), np.uint32)
        kinds[4] = _lib.SPT_MAT_MIRROR
        m["kinds"] = kinds
    elif name == "spheres":                      # an occluder in the opening, a receiver on the floor
        kd = np.concatenate([kd, np.array([[0.6, 0.6, 0.2]], F)])
        ke = np.concatenate([np.zeros_like(ke), np.zeros((1, 3), F)])
        m["spheres"] = np.array([[0.6, 0.55, 2.2, 0.25], [0.75, 0.2, 1.6, 0.15]], F)
        m["sphere_mat"] = np.array([3, 6], np.int32)
    else:
        assert name == "base"
    return m, kd, ke


def make_scene(name="skyonly", cfg=None, sky=True, nee=False, share=0.5, tex=TEX):
    m, kd, ke = variant(name)
    s = sptamd.Scene(config=cfg)
    s.add_arrays(m)
    s.commit(0)
    s.backend.set_albedo(kd)
    s.backend.set_emission(ke)
    if tex is not None:
        s.backend.set_envmap(tex, ROT)
    if nee:
        s.backend.set_light_sampling(True)
    if sky:
        s.backend.set_sky_sampling(True, share)
    return s


def camera(lens=0.0):
    cam = dict(CAM)
    if lens:
        cam["lens_radius"], cam["focal_dist"] = lens, 2.0
    return cam


def oparams(env=ONE, lens=0.0):
    return O.reference_params(W, H, SPP, DEPTH, camera=camera(lens), env=env, **KW)


def gparams(env=ONE, lens=0.0, w=W, h=H, **kw):
    return sptamd.make_params(w, h, SPP, DEPTH, camera=camera(lens), env=env, **KW, **kw)


@functools.lru_cache(maxsize=None)
def expected(name="skyonly", on=True, nee=False, share=0.5, env=ONE, lens=0.0, tex="TEX"):
    """The planes, the contributions and the shadow-ray counts of the restatement."""
    m, kd, ke = variant(name)
    count = {}
    x = S.contributions(m, oparams(env, lens), kd, ke, (globals()[tex], ROT), on=on, nee=nee, share=share, count=count)
    assert np.isfinite(x).all()
    return dict(zip(PLANES, A.moments(x))), x, count


def planes_of(s, p, split=(SPP,)):
    acc = s.accumulator(p)
    st = [acc.add(n) for n in split]
    torch.cuda.synchronize()
    return {k: getattr(acc, k).cpu().numpy() for k in PLANES}, st


def render(s, p):
    film, st = s.render(p)
    torch.cuda.synchronize()
    return film.cpu().numpy(), st


def assert_planes(got, want, msg):
    for k in PLANES:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{msg} {k}")


# ---- 1. the planes are the restatement's

def test_the_restatement_differs_from_the_plain_estimator():
    for kw in (dict(), dict(name="base", nee=True)):
        on, x, n = expected(**kw)
        off = expected(on=False, **kw)[0]
        assert not np.array_equal(on["film"], off["film"]), kw
        # shadow rays toward the sky both left through the opening and ended on a wall
        assert n["sky_visible"] > 500 and n["sky_occluded"] > 500 and n["shadow_casts"] >= n["sky_visible"] + n["sky_occluded"]
    # the sun is in the film, and the sampled estimator finds it from far more paths
    assert expected()[1].max() > 50
    assert (expected()[1] > 1).mean() > 3 * (expected(on=False)[1] > 1).mean()
    # the share matters, and so does light sampling beside it
    assert not np.array_equal(expected("base", nee=True)[0]["film"], expected("base", nee=True, share=0.25)[0]["film"])
    assert not np.array_equal(expected("base", nee=True)[0]["film"], expected("base")[0]["film"])


@pytest.mark.parametrize("build", [_lib.SPT_BUILD_HOST_SAH, _lib.SPT_BUILD_GPU_PLOC])
@pytest.mark.parametrize("width", [2, 6, 8])
def test_planes_equal_the_restatement(width, build):
    want, _, n = expected()
    for order in (_lib.SPT_WORK_SAMPLE_MAJOR, _lib.SPT_WORK_PIXEL_MAJOR):
        cfg = sptamd.default_config()
        cfg.bvh_width, cfg.build, cfg.work_order = width, build, order
        s = make_scene(cfg=cfg)
        assert s.backend.stats["bvh_width"] == width and s.backend.sky_sampling() == (True, 0.5, 64)
        assert s.backend.light_sampling() == (False, 0)
        got, st = planes_of(s, gparams())
        assert st[0]["fused"] == 1 and st[0]["work_order"] == order and st[0]["film_slots_unwritten"] == 0
        assert st[0]["shadow_casts"] == n["shadow_casts"]
        assert_planes(got, want, f"width {width} build {build} order {order}")
        film, _ = render(s, gparams())
        np.testing.assert_array_equal(film, want["film"])


@pytest.mark.parametrize("share", [0.5, 0.25])
def test_with_light_sampling_the_share_chooses(share):
    want, _, n = expected("base", nee=True, share=share)
    for width in (2, 6, 8):
        cfg = sptamd.default_config()
        cfg.bvh_width = width
        s = make_scene("base", cfg=cfg, nee=True, share=share)
        assert s.backend.sky_sampling() == (True, share, 64) and s.backend.light_sampling() == (True, 28)
        got, st = planes_of(s, gparams())
        assert st[0]["shadow_casts"] == n["shadow_casts"]
        assert_planes(got, want, f"share {share} width {width}")
    # the cap emitting, light sampling off: the sky sampled with weight 1, emission counted at hits
    want, _, n = expected("base", share=share)
    got, st = planes_of(make_scene("base", share=share), gparams())
    assert st[0]["shadow_casts"] == n["shadow_casts"]
    assert_planes(got, want, "sky sampling alone on the emitting scene")


def test_sky_off_with_light_sampling_is_the_parent():
    """(tests/test_gpu_nee.py::test_sky_constant_and_sky_image holds the same scene to nee_ref.)"""
    want = expected("base", on=False, nee=True)[0]
    s = make_scene("base", sky=False, nee=True)
    got, _ = planes_of(s, gparams())
    assert_planes(got, want, "light sampling and a sky image, the sky switch off")
    s.backend.set_sky_sampling(True)
    s.backend.set_sky_sampling(False)
    got, _ = planes_of(s, gparams())
    assert_planes(got, want, "on and off again")


def test_mirror_material_clears_both_bits():
    want, _, n = expected("mirror", nee=True)
    assert not np.array_equal(want["film"], expected("base", nee=True)[0]["film"])
    assert 0 < n["shadow_casts"] < expected("base", nee=True)[2]["shadow_casts"]
    got, st = planes_of(make_scene("mirror", nee=True), gparams())
    assert st[0]["shadow_casts"] == n["shadow_casts"]
    assert_planes(got, want, "mirror")


def test_analytic_spheres_occlude_and_receive():
    want, _, n = expected("spheres")
    assert not np.array_equal(want["film"], expected()[0]["film"])
    for width in (2, 6):
        cfg = sptamd.default_config()
        cfg.bvh_width = width
        got, st = planes_of(make_scene("spheres", cfg=cfg), gparams())
        assert st[0]["shadow_casts"] == n["shadow_casts"]
        assert_planes(got, want, f"spheres width {width}")


def test_thin_lens_and_tint():
    want, _, n = expected(lens=0.04)
    assert not np.array_equal(want["film"], expected()[0]["film"])
    got, st = planes_of(make_scene(), gparams(lens=0.04))
    assert st[0]["shadow_casts"] == n["shadow_casts"]
    assert_planes(got, want, "thin lens")
    env = (0.3, 0.7, 1.0)
    want, _, n = expected("base", nee=True, env=env)
    got, st = planes_of(make_scene("base", nee=True), gparams(env=env))
    assert st[0]["shadow_casts"] == n["shadow_casts"]
    assert_planes(got, want, "tint")
    # a black tint: every contribution is 0 and no shadow ray is traced
    got, st = planes_of(make_scene(), gparams(env=(0.0, 0.0, 0.0)))
    assert st[0]["shadow_casts"] == 0 and got["film"].max() == 0


@pytest.mark.parametrize("mode", ["unit", "albedo"])
def test_a_scene_without_an_emission_table(mode):
    """mitsuba_synth under the open sky, no spt_scene_set_emission at all: the scene still
    takes the emitter-mode instances (the only ones with the lane loop)."""
    m, albedo, _ = mode_scene(mode, scenes.mitsuba_synth(detail=0.1))
    alb = np.ones((len(m["kd"]), 3), F) if albedo is None else albedo
    p = O.reference_params(W, H, SPP, DEPTH, env=ONE, **KW)
    count = {}
    x = S.contributions(m, p, alb, None, (TEX_M, ROT), count=count)
    off = S.contributions(m, p, alb, None, (TEX_M, ROT), on=False)
    want = dict(zip(PLANES, A.moments(x)))
    assert not np.array_equal(want["film"], A.moments(off)[2]) and count["sky_visible"] > 500 and count["sky_occluded"] > 100
    s = sptamd.Scene()
    s.add_arrays(m)
    s.commit(0)
    if albedo is not None:
        s.backend.set_albedo(albedo)
    s.backend.set_envmap(TEX_M, ROT)
    gp = sptamd.make_params(W, H, SPP, DEPTH, env=ONE, **KW)
    plain, _ = planes_of(s, gp)
    assert_planes(plain, dict(zip(PLANES, A.moments(off))), f"{mode} off")
    s.backend.set_sky_sampling(True)
    got, st = planes_of(s, gp)
    assert st[0]["fused"] == 1 and st[0]["shadow_casts"] == count["shadow_casts"]
    assert_planes(got, want, mode)


# ---- 2. inert cases

def test_empty_table_no_map_and_switch_off_are_the_parent():
    p = gparams()
    off, so = planes_of(make_scene(sky=False), p)
    assert_planes(off, expected(on=False)[0], "off")
    # the switch off again
    s = make_scene()
    s.backend.set_sky_sampling(False, 0.3)
    assert s.backend.sky_sampling() == (False, pytest.approx(0.3), 0)
    got, st = planes_of(s, p)
    assert_planes(got, off, "switched off")
    assert st[0]["shadow_casts"] == 0
    film, st = render(s, gparams(pipeline="wavefront"))          # inert: the wavefront still runs
    assert st["fused"] == 0
    np.testing.assert_array_equal(film, off["film"])
    # an all-zero map: an empty table
    z = make_scene(tex=np.zeros((4, 4, 3), F))
    assert z.backend.sky_sampling() == (True, 0.5, 0)
    zoff, _ = planes_of(make_scene(sky=False, tex=np.zeros((4, 4, 3), F)), p)
    got, st = planes_of(z, p)
    assert_planes(got, zoff, "zero map")
    assert st[0]["shadow_casts"] == 0 and render(z, gparams(pipeline="wavefront"))[1]["fused"] == 0
    # no map at all: accepted and inert, with and without light sampling
    for nee in (False, True):
        n = make_scene("base", tex=None, nee=nee)
        assert n.backend.sky_sampling() == (True, 0.5, 0)
        ref, sr = planes_of(make_scene("base", tex=None, nee=nee, sky=False), p)
        got, st = planes_of(n, p)
        assert_planes(got, ref, f"no map nee {nee}")
        assert st[0]["shadow_casts"] == sr[0]["shadow_casts"] and st[0]["ray_casts"] == sr[0]["ray_casts"]


# ---- 3. accumulator splits, lists, tiles, queued renders, set_envmap afterwards

def test_splits_lists_tiles_and_the_setter_between_queued_renders():
    want, x, _ = expected()
    s = make_scene()
    p = gparams()
    for split in ([4, 4], [3, 5], [1] * 8):
        got, _ = planes_of(s, p, split)
        assert_planes(got, want, f"split {split}")
    rng = np.random.default_rng(31)
    listed = np.sort(rng.choice(W * H, size=200, replace=False)).astype(np.int32)
    acc = s.accumulator(p)
    acc.add(3)
    st = acc.add_list(5, torch.as_tensor(listed, device="cuda"))
    torch.cuda.synchronize()
    assert st["paths"] == 5 * listed.size and st["shadow_casts"] > 0
    first = dict(zip(PLANES, A.moments(x[:3])))
    mask = np.zeros(W * H, bool)
    mask[listed] = True
    mask = mask.reshape(H, W)
    for k in PLANES:
        np.testing.assert_array_equal(getattr(acc, k).cpu().numpy(), np.where(mask[None], want[k], first[k]), err_msg=k)
    for t in range(2):
        film, _ = render(s, gparams(tile_index=t, tile_count=2, rows_per_group=3))
        np.testing.assert_array_equal(film, want["film"][:, sptamd.tile_rows(H, t, 2, 3)])
    # a render queued before the switch goes off keeps its estimator
    q = sptamd.queue_stream()
    film1, ticket = s.render_async(p, stream=q)
    s.backend.set_sky_sampling(False)
    film2, _ = s.render(p)
    s.render_wait(ticket)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(film1.cpu().numpy(), want["film"])
    np.testing.assert_array_equal(film2.cpu().numpy(), expected(on=False)[0]["film"])


def test_set_envmap_afterwards_rebuilds_or_empties_the_table():
    s = make_scene()
    s.backend.set_envmap(TEX2, ROT)
    assert s.backend.sky_sampling() == (True, 0.5, 64)
    want, _, n = expected(tex="TEX2")
    assert not np.array_equal(want["film"], expected()[0]["film"])
    got, st = planes_of(s, gparams())
    assert st[0]["shadow_casts"] == n["shadow_casts"]
    assert_planes(got, want, "a new map")
    s.backend.set_envmap(None)                                   # the table empties, the switch stays
    assert s.backend.sky_sampling() == (True, 0.5, 0)
    ref, _ = planes_of(make_scene(tex=None, sky=False), gparams())
    got, st = planes_of(s, gparams())
    assert st[0]["shadow_casts"] == 0
    assert_planes(got, ref, "the map removed")
    s.backend.set_envmap(TEX, ROT)                                # and a map again: sampled again
    got, _ = planes_of(s, gparams())
    assert_planes(got, expected()[0], "the map back")
    # a rotation that is not orthonormal: the map is set, the switch goes off, the error is returned
    bad = (ROT * F(1.5)).astype(F)
    with pytest.raises(sptamd.SptError) as e:
        s.backend.set_envmap(TEX, bad)
    assert e.value.code == _lib.SPT_ERR_INVALID and "orthonormal" in str(e.value)
    assert s.backend.sky_sampling() == (False, 0.5, 0)
    got, _ = planes_of(s, gparams())
    u = make_scene(sky=False, tex=None)
    u.backend.set_envmap(TEX, bad)
    assert_planes(got, planes_of(u, gparams())[0], "the scaled rotation, unsampled")
    with pytest.raises(sptamd.SptError) as e:
        u.backend.set_sky_sampling(True)
    assert e.value.code == _lib.SPT_ERR_INVALID and u.backend.sky_sampling() == (False, 0.5, 0)


# ---- 4. counters and refusals

def test_shadow_casts_and_ray_casts():
    n = expected()[2]
    on, off = make_scene(), make_scene(sky=False)
    _, a = render(on, gparams())
    _, b = render(off, gparams(pipeline="fused"))
    assert a["shadow_casts"] == n["shadow_casts"] and b["shadow_casts"] == 0
    for k in ("ray_casts", "continuations", "paths", "paths_started", "paths_terminated"):
        assert a[k] == b[k], k
    assert a["paths"] == W * H * SPP and a["film_slots_unwritten"] == 0


def test_refusals(tmp_path):
    s = make_scene()
    film0, _ = render(s, gparams())
    with pytest.raises(sptamd.SptError) as e:
        s.render(gparams(pipeline="wavefront"))
    assert e.value.code == _lib.SPT_ERR_INVALID and "sky sampling" in str(e.value)
    p = gparams()
    p.flags |= _lib.SPT_FLAG_TRAVERSAL_STATS
    with pytest.raises(sptamd.SptError) as e:
        s.render(p)
    assert e.value.code == _lib.SPT_ERR_INVALID and "sky sampling" in str(e.value)
    h = s.backend.handle
    for on, share in ((7, 0.5), (1, 0.0), (1, 1.0), (0, float("nan")), (1, -1.0)):
        assert _lib.lib.spt_scene_set_sky_sampling(h, on, share) == _lib.SPT_ERR_INVALID
    assert s.backend.sky_sampling() == (True, 0.5, 64)
    again, _ = render(s, gparams())
    np.testing.assert_array_equal(again, film0)
    cfg = sptamd.default_config()
    cfg.pipeline = _lib.SPT_PIPELINE_WAVEFRONT                   # the config's pipeline choice does not matter
    film, st = render(make_scene(cfg=cfg), gparams())
    assert st["fused"] == 1
    np.testing.assert_array_equal(film, film0)
    # the cache does not store the switch: refused with it on, map or no map
    t = make_scene(tex=None)
    path = str(tmp_path / "scene.sptc")
    with pytest.raises(sptamd.SptError) as e:
        t.save(path)
    assert e.value.code == _lib.SPT_ERR_INVALID and "sky sampling" in str(e.value) and not os.path.exists(path)
    t.backend.set_sky_sampling(False)
    t.save(path)
    assert os.path.exists(path)


def test_lds_guard_counts_the_larger_park():
    """test_gpu_nee.py's guard with the sky switch: a stack that fits beside 32 B per lane
    and not beside 64 B is refused with SPT_ERR_LIMIT; eight entries fewer, it renders."""
    cap = torch.cuda.get_device_properties(0).shared_memory_per_block
    block, wide = 128, 2 * 128 * 16
    entries = (cap - wide - block * 32) // (block * 4)
    assert entries * block * 4 + wide + block * 64 > cap
    base = hostile.tri_soup(hostile.family("coincident"))[:1]

    def deep(n, slack):
        cfg = sptamd.default_config()
        cfg.bvh_width, cfg.build, cfg.stack_slack = 6, _lib.SPT_BUILD_GPU_PLOC, slack
        s = sptamd.Scene(config=cfg)
        s.add_arrays(hostile.soup(np.repeat(base, n, axis=0)))
        s.commit(0)
        return s

    lo, hi, chosen = 256, 1 << 16, None
    for _ in range(16):
        n = (lo + hi) // 2
        try:
            have = deep(n, 0).backend.stats["max_depth"] - 1
        except sptamd.SptError as e:
            assert e.code == _lib.SPT_ERR_LIMIT
            have = entries + 1
        if entries - 64 <= have <= entries - 8:
            chosen = (n, entries - have)
            break
        lo, hi = (n, hi) if have < entries - 64 else (lo, n)
    assert chosen, f"no stack of copies reaches {entries} stack entries with 8 <= stack_slack <= 64 (LDS {cap} B)"
    n, slack = chosen
    p = sptamd.make_params(16, 8, 2, 3, camera=hostile.camera("coincident"), env=ONE, **KW)

    def lit(s):
        s.backend.set_albedo(np.array([[0.7, 0.7, 0.7]], F))
        s.backend.set_envmap(TEX, ROT)
        return s

    s = lit(deep(n, slack))
    film0, _ = render(s, p)
    with pytest.raises(sptamd.SptError) as e:
        s.backend.set_sky_sampling(True)
    assert e.value.code == _lib.SPT_ERR_LIMIT and "LDS" in str(e.value)
    assert s.backend.sky_sampling() == (False, 0.5, 0)
    np.testing.assert_array_equal(render(s, p)[0], film0)
    t = lit(deep(n, slack - 8))
    t.backend.set_sky_sampling(True)
    assert t.backend.sky_sampling() == (True, 0.5, 64)
    film, st = render(t, p)
    assert st["fused"] == 1 and st["film_slots_unwritten"] == 0 and np.isfinite(film).all()


# ---- 5. the same expectation, with less variance

@pytest.mark.parametrize("name,nee", [("skyonly", False), ("base", True)])
def test_same_expectation(name, nee):
    """32 x 24: every switch off at 2^16 spp against sky sampling (and, for the emitting
    scene, light sampling at share 1/2) at 2^12 spp, means and variances of the mean from
    two accumulators; every pixel and channel within z <= 5 (tests/independent.py's
    bound), the image mean likewise; no pixel skipped.

    Measured on an MI355X: the sky alone, image means 4.49545 (off) 4.50773 (on), image z
    2.39, worst of the 2304 values z 4.24; with the cap and light sampling 4.57286 / 4.59569,
    3.39, 4.15 (the two scenes share their paths, so these are one observation, not two).
    No value had an off variance of 0.  At 2^20 / 2^17 spp the image means stand at 4.495778 /
    4.497844 (z +1.97) and 4.573197 / 4.574260 (z +0.82), and at 48 x 36 and the same counts at
    4.497823 / 4.496332 (z -2.13) and 4.575174 / 4.572694 (z -2.87): the sign turns, and the mean
    of z^2 over the single values is 0.94 - 0.98 in all four."""
    w, h = 32, 24
    res = {}
    for on, spp in ((False, 1 << 16), (True, 1 << 12)):
        acc = make_scene(name, sky=on, nee=nee and on).accumulator(gparams(w=w, h=h))
        acc.add(spp)
        torch.cuda.synchronize()
        res[on] = (acc.film.cpu().numpy().astype(np.float64), acc.variance.cpu().numpy().astype(np.float64))
    (m0, v0), (m1, v1) = res[False], res[True]
    both0 = (v0 == 0) & (v1 == 0)
    np.testing.assert_array_equal(m1[both0], m0[both0])
    z = np.abs(m1 - m0) / np.sqrt(np.where(both0, 1.0, v0 + v1))
    zi = abs(m1.mean() - m0.mean()) / np.sqrt((v0.sum() + v1.sum()) / m0.size ** 2)
    print(f"same expectation {name}: worst pixel z {z[~both0].max():.2f}, image z {zi:.2f}, means {m0.mean():.5f} "
          f"{m1.mean():.5f}, {int(both0.sum())} values with both variances 0, {int((v0 == 0).sum())} with the off variance 0")
    assert m0.mean() > 0.05
    # the off render has a variance of its own wherever the sampled one sees light
    assert not np.any((v0 == 0) & (m1 > 0))
    assert z[~both0].max() <= 5.0
    assert zi <= 5.0


def test_sky_sampling_lowers_the_variance():
    """64 spp, the sky the only light: the image mean of the variance plane with the switch
    on against off (off: the parent's estimator, bit for bit —
    test_empty_table_no_map_and_switch_off_are_the_parent).  Measured once on an MI355X: off
    20.6334, on 2.34495, ratio 8.80 (MEASURED_VARIANCE_RATIO, DESIGN.md §15,
    profiles/sky/variance_ratio.txt); half of it is asserted, the off estimate being
    firefly-dominated at 64 spp."""
    v = {}
    for on in (False, True):
        acc = make_scene(sky=on).accumulator(gparams())
        acc.add(64)
        torch.cuda.synchronize()
        v[on] = float(acc.variance.cpu().numpy().astype(np.float64).mean())
    ratio = v[False] / v[True]
    print(f"variance off {v[False]:.6g} on {v[True]:.6g} ratio {ratio:.2f}")
    assert v[True] < v[False]
    assert MEASURED_VARIANCE_RATIO is not None, "the ratio has not been measured"
    assert ratio >= MEASURED_VARIANCE_RATIO / 2


# ---- 6. the command-line host

def test_cli_sky_nee_equals_the_python_api(tmp_path):
    w, h, d, spp = 40, 24, 4, 4
    s = sptamd.Scene()
    s.add_triangle_mesh(scenes.scene_pbrt("cornell_spheres", DETAIL))
    s.commit(0)
    kd, ke = scenes.smallpt_materials(s.mesh)
    s.backend.set_albedo(kd)
    s.backend.set_emission(ke)
    path, oct_pfm = str(tmp_path / "cornell.sptc"), str(tmp_path / "oct.pfm")
    s.save(path)
    sptamd.write_pfm(oct_pfm, np.ascontiguousarray(TEX.transpose(2, 0, 1)))
    deg = 30.0
    t = np.deg2rad(deg)
    rot = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]]).astype(F)
    sky = ["--envmap-oct", oct_pfm, "--env-rotate-y", str(deg)]

    def cli(out, *flags, ok=True):
        r = subprocess.run([CLI, "-w", str(w), "-h", str(h), "-d", str(d), "-s", str(spp), "--rr", "2", path, "-o", out]
                           + list(flags), capture_output=True, text=True, timeout=180)
        if not ok:
            return r
        assert r.returncode == 0, r.stdout + r.stderr
        return sptamd.read_pfm(out).transpose(2, 0, 1)

    p = sptamd.make_params(w, h, spp, d, camera=s.pbrt_info["camera"], rr_start_depth=2)
    s.backend.set_envmap(TEX, rot)
    plain, _ = render(s, p)
    np.testing.assert_array_equal(cli(str(tmp_path / "off.pfm"), *sky), plain)
    s.backend.set_sky_sampling(True)
    want, st = render(s, p)
    assert st["shadow_casts"] > 0 and not np.array_equal(want, plain)
    np.testing.assert_array_equal(cli(str(tmp_path / "on.pfm"), *sky, "--sky-nee"), want)
    np.testing.assert_array_equal(cli(str(tmp_path / "acc.pfm"), *sky, "--sky-nee", "-s", "2", "--passes", "2"), want)
    s.backend.set_light_sampling(True)
    s.backend.set_sky_sampling(True, 0.25)
    both, _ = render(s, p)
    assert not np.array_equal(both, want)
    np.testing.assert_array_equal(cli(str(tmp_path / "both.pfm"), *sky, "--sky-nee", "--nee", "--sky-share", "0.25"), both)
    # refused with a message: no map, a share outside (0, 1), a share without the switch
    for flags in (["--sky-nee"], sky + ["--sky-nee", "--sky-share", "1"], sky + ["--sky-share", "0.3"]):
        r = cli(str(tmp_path / "no.pfm"), *flags, ok=False)
        assert r.returncode == 2 and "--sky-" in r.stderr and not os.path.exists(str(tmp_path / "no.pfm")), flags
