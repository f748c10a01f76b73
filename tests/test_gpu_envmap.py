"""Environment-map lighting on the GPU (spt_scene_set_envmap): the
film of a scene under an octahedral sky image is the CPU restatement's
(tests/envmap_ref.py over the oracle's rays and throughputs) bit for bit, in
every pipeline, work order and tree width, with spheres and glass, through the
accumulator and its pixel lists; a unit map leaves the parent's images as they
were; the lookup's edge rule is exercised at the -z pole; the setter orders
itself against queued renders; spt_render_aov and spt_intersect do not see the
map; spt_render_cli's flags give the Python API's image."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import accum_ref as A
import envmap_ref as E
import oracle as O
import sptamd
from sptamd import _lib, scenes
from test_accum_ref import ALBEDO, mode_scene

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, DEPTH = 37, 19, 8, 4
KW = dict(rr_start_depth=2, env=(0.3, 0.7, 1.0))
PLANES = ("sum", "sum_sq", "film", "variance")
N = 8
TEX = E.random_map(N, seed=21)
ROT = E.rotation((0.4, 1.0, -0.3), 63.0)
TEX2 = E.random_map(N, seed=22)
CLI = os.path.join(os.path.dirname(_lib.LIB_PATH), "spt_render_cli")


def make_scene(mode, cfg=None, envmap=True):
    m, albedo, emi = mode_scene(mode)
    s = sptamd.Scene(config=cfg)
    s.add_arrays(m)
    s.commit(0)
    if albedo is not None:
        s.backend.set_albedo(albedo)
    if emi is not None:
        s.backend.set_emission(emi)
    if envmap:
        s.backend.set_envmap(TEX, ROT)
    return s


@functools.lru_cache(maxsize=None)
def expected(mode):
    """(sum, sum_sq, film, variance) and the per-sample contributions of the mode's scene under TEX / ROT."""
    m, albedo, emi = mode_scene(mode)
    osc = O.OracleScene(m, albedo=albedo)
    osc_e = O.OracleScene(m, albedo=albedo, emission=emi) if emi is not None else None
    x = E.contributions(osc, O.reference_params(W, H, SPP, DEPTH, **KW), TEX, ROT, osc_emit=osc_e)
    assert x.max() > 50.0     # a bright texel is in view
    return dict(zip(PLANES, A.moments(x))), x


def pipeline_params(pipeline, cfg, **kw):
    """wavefront: a job that fits in flight (camera cast, drain); queued: the
    per-cast wavefront over short queues with the drain; percast: without it."""
    if pipeline == "percast":
        cfg.drain_q8 = 0
    flag = "fused" if pipeline == "fused" else "wavefront"
    wp = 0 if pipeline in ("wavefront", "fused") else 1500
    return sptamd.make_params(W, H, SPP, DEPTH, pipeline=flag, wavefront_paths=wp, **KW, **kw)


def render(s, p):
    film, st = s.render(p)
    torch.cuda.synchronize()
    return film.cpu().numpy(), st


# ---- 1. the film is the restatement's

@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("pipeline", ["wavefront", "queued", "fused", "percast"])
def test_film_equals_the_restatement(pipeline, order):
    for mode in ("unit", "albedo", "emit"):
        cfg = sptamd.default_config()
        cfg.work_order = order
        p = pipeline_params(pipeline, cfg)
        film, st = render(make_scene(mode, cfg), p)
        assert st["work_order"] == order and st["fused"] == (pipeline == "fused")
        assert st["film_slots_unwritten"] == 0
        np.testing.assert_array_equal(film, expected(mode)[0]["film"], err_msg=f"{mode} {pipeline} order {order}")


@pytest.mark.parametrize("width", [2, 6, 8])
def test_film_equals_the_restatement_in_every_tree_width(width):
    for mode in ("unit", "albedo", "emit"):
        cfg = sptamd.default_config()
        cfg.bvh_width = width
        s = make_scene(mode, cfg)
        assert s.backend.stats["bvh_width"] == width
        for pipeline in ("wavefront", "fused"):
            film, _ = render(s, pipeline_params(pipeline, cfg))
            np.testing.assert_array_equal(film, expected(mode)[0]["film"], err_msg=f"{mode} width {width} {pipeline}")


# ---- 2. spheres, mirror and glass

def test_spheres_and_glass_equal_the_restatement():
    m, albedo, _ = mode_scene("albedo")
    spheres = np.array([[0.0, 0.9, 0.3, 0.55], [1.3, 0.5, 0.9, 0.4], [-1.2, 0.45, 1.0, 0.35]], F)
    sph_mat = np.array([1, 2, 3], np.int32)
    kinds = np.array([0, _lib.SPT_MAT_GLASS, _lib.SPT_MAT_MIRROR, 0, 0, 0], np.uint32)[: len(albedo)]
    p = O.reference_params(W, H, SPP, 6, **KW)
    osc = O.OracleScene(m, albedo=albedo, spheres=spheres, sphere_mat=sph_mat, kinds=kinds)
    x = E.contributions(osc, p, TEX, ROT)
    want = A.moments(x)[2]
    # the spheres are in view and the glass one passes sky through
    plain = A.moments(E.contributions(O.OracleScene(m, albedo=albedo), p, TEX, ROT))[2]
    assert not np.array_equal(want, plain) and want.max() > 1.0
    for pipeline in ("wavefront", "fused"):
        cfg = sptamd.default_config()
        s = sptamd.Scene(config=cfg)
        s.add_arrays(m)
        s.commit(0)
        s.backend.set_albedo(albedo)
        s.backend.set_spheres(spheres, sph_mat)
        s.backend.set_material_kinds(kinds)
        s.backend.set_envmap(TEX, ROT)
        film, _ = render(s, sptamd.make_params(W, H, SPP, 6, pipeline=pipeline, **KW))
        np.testing.assert_array_equal(film, want, err_msg=pipeline)


# ---- 3. a unit map is no map

def planes_of(s, p, split=(SPP,)):
    acc = s.accumulator(p)
    for n in split:
        acc.add(n)
    torch.cuda.synchronize()
    return {k: getattr(acc, k).cpu().numpy() for k in PLANES}


@pytest.mark.parametrize("mode", ["unit", "albedo", "emit"])
def test_unit_map_gives_the_images_of_no_map(mode):
    p = sptamd.make_params(W, H, SPP, DEPTH, **KW)
    s = make_scene(mode, envmap=False)
    base = planes_of(s, p)
    film0, _ = render(s, p)
    s.backend.set_envmap(np.ones((1, 1, 3), F))
    got = planes_of(s, p)
    film1, _ = render(s, p)
    for k in PLANES:
        np.testing.assert_array_equal(got[k], base[k], err_msg=f"{mode} {k}")
    np.testing.assert_array_equal(film1, film0)
    np.testing.assert_array_equal(film0, base["film"])
    assert film0.max() > 0


# ---- 4. the lookup at the -z pole: every edge and a corner

def pole_camera(lens_radius):
    cam = dict(sptamd.reference_camera())
    cam["lens_radius"] = lens_radius
    cam["focal_dist"] = 4.0
    return cam


def pole_rotation(cam):
    """World -> map with the view direction on the map's -z axis, then a turn about it (no axis lines up)."""
    v = np.array(cam["look_at"], np.float64) - np.array(cam["look_from"], np.float64)
    z = -v / np.linalg.norm(v)
    x = np.cross([0.3, 1.0, 0.2], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z]).astype(F)


@functools.lru_cache(maxsize=None)
def pole_expected(lens_radius):
    cam = pole_camera(lens_radius)
    p = O.reference_params(W, H, SPP, 1, camera=cam, **KW)
    d = np.zeros((SPP, H, W, 3), F)
    for y in range(H):
        for px in range(W):
            xi = O.pcg32_floats(p.rng_initstate, y * W + px, 6 * SPP)     # 4 + 2 x 1 draws a sample
            for s in range(SPP):
                # rng_order 0: each pair of draws is (y, x) (the reference's argument evaluation order)
                d[s, y, px] = O.camera_ray(p, px, y, xi[6 * s: 6 * s + 4][[1, 0, 3, 2]])[1]
    touched = {}
    m = E.lookup(TEX, pole_rotation(cam), d, touched=touched)
    x = (np.array(KW["env"], F) * m).astype(F)       # T = 1: 0 + 1 (env M)
    return A.moments(np.ascontiguousarray(np.moveaxis(x, -1, 1)))[2], touched, d


@pytest.mark.parametrize("lens_radius", [0.0, 0.05])
def test_empty_scene_sees_the_map_across_every_edge_and_a_corner(lens_radius):
    want, touched, d = pole_expected(lens_radius)
    # the test counts only if the restatement's fetches left the image on all four edges and at a corner
    assert all(touched.get(k, 0) > 0 for k in E.EDGES), touched
    cam = pole_camera(lens_radius)
    # the camera directions are the oracle's own first rays
    osc = O.OracleScene({"pos": np.zeros((0, 3), F), "pos_tri": np.zeros((0, 3), np.int32)})
    esc, d2, T = E.escapes(osc, O.reference_params(W, H, SPP, 1, camera=cam, **KW))
    assert esc.all() and (T == 1).all()
    np.testing.assert_array_equal(d2, d)
    for pipeline in ("wavefront", "fused"):
        s = sptamd.Scene()
        s.add_arrays({"pos": np.zeros((0, 3), F), "pos_tri": np.zeros((0, 3), np.int32)})
        s.commit(0)
        s.backend.set_envmap(TEX, pole_rotation(cam))
        film, st = render(s, sptamd.make_params(W, H, SPP, 1, camera=cam, pipeline=pipeline, **KW))
        assert st["ray_casts"] == W * H * SPP
        np.testing.assert_array_equal(film, want, err_msg=f"{pipeline} lens {lens_radius}")


# ---- 5. the accumulator and its pixel lists

@pytest.mark.parametrize("pipeline", ["wavefront", "fused"])
def test_accumulator_splits_and_lists(pipeline):
    ref, x = expected("emit")
    s = make_scene("emit")
    p = sptamd.make_params(W, H, SPP, DEPTH, pipeline=pipeline, **KW)
    for split in ([8], [3, 5], [1] * 8):
        got = planes_of(s, p, split)
        for k in PLANES:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{pipeline} split {split} {k}")
    assert (ref["variance"] > 0).any()
    # 3 samples everywhere, then 5 more on a random ascending list
    rng = np.random.default_rng(31)
    listed = np.sort(rng.choice(W * H, size=200, replace=False)).astype(np.int32)
    acc = s.accumulator(p)
    acc.add(3)
    st = acc.add_list(5, torch.as_tensor(listed, device="cuda"))
    torch.cuda.synchronize()
    assert st["paths"] == 5 * listed.size
    first = dict(zip(PLANES, A.moments(x[:3])))
    mask = np.zeros(W * H, bool)
    mask[listed] = True
    mask = mask.reshape(H, W)
    for k in PLANES:
        want = np.where(mask[None], ref[k], first[k])
        np.testing.assert_array_equal(getattr(acc, k).cpu().numpy(), want, err_msg=f"{pipeline} list {k}")
    np.testing.assert_array_equal(acc.count.cpu().numpy(), np.where(mask, 8, 3))


# ---- 6. the setter among queued renders, and the scene cache

def test_setter_waits_for_queued_renders_and_save_refuses_a_map(tmp_path):
    s = make_scene("albedo")
    p = sptamd.make_params(W, H, SPP, DEPTH, **KW)
    want1 = expected("albedo")[0]["film"]
    q = sptamd.queue_stream()
    film1, ticket = s.render_async(p, stream=q)
    s.backend.set_envmap(TEX2, ROT)                 # while the first render may still be queued
    film2, _ = s.render(p)
    s.render_wait(ticket)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(film1.cpu().numpy(), want1)
    assert not np.array_equal(film2.cpu().numpy(), want1)
    # with a map the cache refuses, and the scene still renders
    path = str(tmp_path / "scene.sptc")
    with pytest.raises(sptamd.SptError) as e:
        s.save(path)
    assert e.value.code == _lib.SPT_ERR_INVALID and "environment map" in str(e.value) and not os.path.exists(path)
    again, _ = render(s, p)
    np.testing.assert_array_equal(again, film2.cpu().numpy())
    # a refused setter leaves the map as it was
    bad = TEX.copy()
    bad[3, 3, 1] = np.inf
    with pytest.raises(sptamd.SptError):
        s.backend.set_envmap(bad)
    assert _lib.lib.spt_scene_set_envmap(s.backend.handle, TEX.ctypes.data, 4097, None) == _lib.SPT_ERR_LIMIT
    again, _ = render(s, p)
    np.testing.assert_array_equal(again, film2.cpu().numpy())
    # without the map: the plain render, and the cache works again
    s.backend.set_envmap(None)
    plain, _ = render(make_scene("albedo", envmap=False), p)
    none, _ = render(s, p)
    np.testing.assert_array_equal(none, plain)
    s.save(path)
    # a loaded scene takes a map
    t = sptamd.Scene.load(path)
    loaded, _ = render(t, p)
    np.testing.assert_array_equal(loaded, plain)
    t.backend.set_envmap(TEX, ROT)
    loaded, _ = render(t, p)
    np.testing.assert_array_equal(loaded, want1)


# ---- 7. what does not read the map

def test_aov_and_intersect_are_unchanged_by_a_map():
    s = make_scene("albedo", envmap=False)
    p = sptamd.make_params(W, H, SPP, DEPTH, **KW)
    rng = np.random.default_rng(41)
    n = 2048
    o = np.repeat(np.array([[0.0], [3.03], [5.0]], F), n, 1)
    d = rng.normal(size=(3, n)).astype(F)
    d[1] = -np.abs(d[1])
    rays = sptamd.Ray3.make(o, d)

    def snapshot():
        aov = s.render_aov(p)
        hit = s.backend.intersect_raw(rays)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in aov.items()}, [h.cpu().numpy() for h in hit]

    aov0, hit0 = snapshot()
    s.backend.set_envmap(TEX, ROT)
    aov1, hit1 = snapshot()
    assert aov0.keys() == aov1.keys() and (hit0[0] >= 0).any()
    for k in aov0:
        np.testing.assert_array_equal(aov1[k], aov0[k], err_msg=k)
    for a, b in zip(hit0, hit1):
        np.testing.assert_array_equal(b, a)


# ---- 8. the command-line host

def test_cli_envmap_flags_equal_the_python_api(tmp_path):
    w, h, d, spp = 40, 24, 4, 4
    obj = scenes.scene_obj("mitsuba_synth", 0.1)
    oct_pfm, ll_pfm = str(tmp_path / "oct.pfm"), str(tmp_path / "latlong.pfm")
    sptamd.write_pfm(oct_pfm, np.ascontiguousarray(TEX.transpose(2, 0, 1)))
    latlong = E.random_map(16, seed=51)[:8]                      # 8 rows x 16 columns
    sptamd.write_pfm(ll_pfm, np.ascontiguousarray(latlong.transpose(2, 0, 1)))

    def cli(out, *flags):
        r = subprocess.run([CLI, "-w", str(w), "-h", str(h), "-d", str(d), "-s", str(spp), obj, "-o", out] + list(flags),
                           capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stdout + r.stderr
        return sptamd.read_pfm(out).transpose(2, 0, 1)

    s = sptamd.Scene()
    s.add_triangle_mesh(obj)
    s.commit(0)
    p = sptamd.make_params(w, h, spp, d)
    plain, _ = render(s, p)
    deg = 30.0
    t = np.deg2rad(deg)
    rot = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]]).astype(F)
    s.backend.set_envmap(TEX, rot)
    want, _ = render(s, p)
    assert not np.array_equal(want, plain)
    got = cli(str(tmp_path / "a.pfm"), "--envmap-oct", oct_pfm, "--env-rotate-y", str(deg))
    np.testing.assert_array_equal(got, want)
    s.backend.set_envmap(sptamd.envmap_from_latlong(latlong, 16))
    want, _ = render(s, p)
    got = cli(str(tmp_path / "b.pfm"), "--envmap", ll_pfm, "--env-res", "16")
    np.testing.assert_array_equal(got, want)
    # and through the accumulating path
    got = cli(str(tmp_path / "c.pfm"), "--envmap", ll_pfm, "--env-res", "16", "-s", "2", "--passes", "2")
    np.testing.assert_array_equal(got, want)
