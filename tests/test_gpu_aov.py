"""spt_render_aov (include/spt.h): the first-hit albedo / normal / depth /
coverage planes of a tile, bit-equal to a reference built from the CPU
oracle's first casts (tests/aov_ref.py) — textured materials behind a thin
lens in both rng orders and every tree width, smallpt's analytic spheres with
mirror and glass materials, a mesh without normals, a camera that mostly sees
sky — and the call's other promises: tiles, NULL planes, argument checks, no
effect on renders, and alignment with the beauty pass."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import aov_ref
import oracle as O
import sptamd
from sptamd import _lib, scenes

pytestmark = pytest.mark.gpu

DEPTH = 3   # sets the draws per sample (4 + 2 x casts), like the render's
SHAPES = [(37, 19, 5), (64, 3, 1), (37, 19, 1), (64, 3, 5)]
PLANES = ("albedo", "normal", "depth", "coverage")

LENS_CAM = dict(look_from=(0.0, 3.03, 5.0), look_at=(0.0, 1.2, 0.0), up=(0.0, 1.0, 0.0), lens_radius=0.05,
                focal_dist=5.0, fov_y=0.9, film_size_y=0.035)
SKY_CAM = dict(look_from=(0.0, 3.03, 5.0), look_at=(0.0, 2.6, 0.0), up=(0.0, 1.0, 0.0), lens_radius=0.0,
               focal_dist=1.0, fov_y=0.9, film_size_y=0.035)


def smallpt_cam(h):
    # into the box's open front, the two balls on the centre rows; the narrow
    # 64 x 3 strip gets a narrow field so the box still spans many pixels
    return dict(look_from=(0.8, 0.3, 6.0), look_at=(0.5, 0.2, 0.6), up=(0.0, 1.0, 0.0), lens_radius=0.0,
                focal_dist=1.0, fov_y=0.5 if h == 19 else 0.05, film_size_y=0.035)


def textures():  # the set of test_gpu_textures.py
    rng = np.random.default_rng(3)
    return {1: scenes.checker(8, 8, cell=1),
            2: rng.uniform(0.1, 0.95, size=(5, 3, 3)).astype(np.float32),
            3: scenes.checker(16, 4, cell=2),
            5: np.full((1, 1, 3), 0.7, np.float32)}


@functools.lru_cache(maxsize=None)
def mitsuba():
    m = scenes.with_planar_uv(scenes.mitsuba_synth(detail=0.15))
    rng = np.random.default_rng(11)
    albedo = rng.uniform(0.2, 0.9, size=(len(m["kd"]), 3)).astype(np.float32)
    return m, albedo


@functools.lru_cache(maxsize=None)
def mitsuba_scene(width):
    m, albedo = mitsuba()
    cfg = sptamd.default_config()
    cfg.bvh_width = width
    s = sptamd.Scene(config=cfg)
    s.add_arrays(m)
    s.commit(0)
    s.backend.set_albedo(albedo)
    for mat, img in textures().items():
        s.backend.set_texture(mat, img)
    assert s.backend.stats["bvh_width"] == width
    return s


@functools.lru_cache(maxsize=None)
def mitsuba_hits(w, h, spp, order):
    m, albedo = mitsuba()
    osc = O.OracleScene(m, albedo=albedo, textures=textures())
    return aov_ref.first_hits(osc, O.reference_params(w, h, spp, DEPTH, camera=LENS_CAM, rng_order=order), range(h))


def assert_hits_and_misses(h):
    hit = h["id"] != -1
    assert hit.any() and (~hit).any(), "the case must have both hit and miss samples"


def assert_planes_equal(got, ref):
    for k in PLANES:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


@pytest.mark.parametrize("width", [2, 6, 8])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("w,h,spp", SHAPES)
def test_textured_thin_lens_bitexact(w, h, spp, order, width):
    m, albedo = mitsuba()
    hits = mitsuba_hits(w, h, spp, order)
    assert_hits_and_misses(hits)
    s = mitsuba_scene(width)
    ref = aov_ref.reference_planes(s, m, hits, albedo=albedo, textures=textures())
    got = aov_ref.gpu_planes(s, sptamd.make_params(w, h, spp, DEPTH, camera=LENS_CAM, rng_order=order))
    assert_planes_equal(got, ref)
    if spp > 1 and h > 3:   # silhouettes: some pixels are partly covered
        assert ((ref["coverage"] > 0) & (ref["coverage"] < 1)).any()
    if order == 1 and spp == 5 and h == 19:  # the lens draws matter: the other order gives other planes
        other = mitsuba_hits(w, h, spp, 0)
        assert not np.array_equal(other["o"], hits["o"])


@pytest.mark.parametrize("w,h,spp", SHAPES[:2])
def test_smallpt_spheres_mirror_glass(w, h, spp):
    m = scenes.smallpt_analytic(detail=0.5)
    alb, emi = scenes.smallpt_materials(m)
    cam = smallpt_cam(h)
    osc = O.OracleScene(m, albedo=alb, emission=emi)
    hits = aov_ref.first_hits(osc, O.reference_params(w, h, spp, DEPTH, camera=cam), range(h))
    assert_hits_and_misses(hits)
    assert (hits["id"] == -2).any() and (hits["id"] == -3).any(), "the mirror and the glass ball must be seen"
    assert (hits["id"] >= 0).any()
    s = sptamd.Scene()
    s.add_arrays(m)
    s.commit(0)
    s.backend.set_albedo(alb)
    s.backend.set_emission(emi)
    ref = aov_ref.reference_planes(s, m, hits, albedo=alb)
    got = aov_ref.gpu_planes(s, sptamd.make_params(w, h, spp, DEPTH, camera=cam))
    assert_planes_equal(got, ref)
    # mirror and glass report their albedo-table colour
    ball = (hits["id"][:, :, 0] == -2) | (hits["id"][:, :, 0] == -3)
    if spp == 1:
        assert np.all(got["albedo"][:, ball] == np.float32(0.999))
    else:
        assert ((ref["coverage"] > 0) & (ref["coverage"] < 1)).any()


def test_mesh_without_normals_uses_geometric_normal():
    m = {k: v for k, v in scenes.mitsuba_synth(detail=0.15).items() if k not in ("nrm", "nrm_tri")}
    w, h, spp = 37, 19, 5
    hits = aov_ref.first_hits(O.OracleScene(m), O.reference_params(w, h, spp, DEPTH, camera=LENS_CAM), range(h))
    assert_hits_and_misses(hits)
    s = sptamd.Scene()
    s.add_arrays(m)
    s.commit(0)
    ref = aov_ref.reference_planes(s, m, hits)
    got = aov_ref.gpu_planes(s, sptamd.make_params(w, h, spp, DEPTH, camera=LENS_CAM))
    assert_planes_equal(got, ref)
    # flat shading: a fully covered pixel whose samples hit one triangle has a unit normal
    one = (hits["id"].min(2) == hits["id"].max(2)) & (hits["id"].min(2) >= 0)
    assert one.any()
    np.testing.assert_allclose(np.linalg.norm(got["normal"][:, one], axis=0), 1.0, atol=1e-6)
    assert np.all(got["albedo"][:, ref["coverage"] == 1] == 1.0)   # no albedo table: material 0's 1


def test_pixels_that_miss_entirely_are_zero():
    m, albedo = mitsuba()
    w, h, spp = 37, 19, 5
    osc = O.OracleScene(m, albedo=albedo, textures=textures())
    hits = aov_ref.first_hits(osc, O.reference_params(w, h, spp, DEPTH, camera=SKY_CAM), range(h))
    assert_hits_and_misses(hits)
    sky = (hits["id"] == -1).all(2)
    assert sky.sum() > w and (~sky).any()
    s = mitsuba_scene(8)
    got = aov_ref.gpu_planes(s, sptamd.make_params(w, h, spp, DEPTH, camera=SKY_CAM))
    assert_planes_equal(got, aov_ref.reference_planes(s, m, hits, albedo=albedo, textures=textures()))
    for k in PLANES:
        assert np.all(got[k][..., sky] == 0.0), k


def test_tiles_stitch_to_the_whole_image():
    w, h, spp = 37, 19, 5
    s = mitsuba_scene(8)
    whole = aov_ref.gpu_planes(s, sptamd.make_params(w, h, spp, DEPTH, camera=LENS_CAM))
    stitched = {k: np.full_like(v, np.nan) for k, v in whole.items()}
    for ti in range(3):
        rows = sptamd.tile_rows(h, ti, 3, 2)
        part = aov_ref.gpu_planes(s, sptamd.make_params(w, h, spp, DEPTH, camera=LENS_CAM, tile_index=ti,
                                                        tile_count=3, rows_per_group=2))
        for k in PLANES:
            assert part[k].shape[-2] == len(rows)
            stitched[k][..., rows, :] = part[k]
    assert_planes_equal(stitched, whole)


def test_null_planes_are_skipped():
    w, h, spp = 37, 19, 5
    s = mitsuba_scene(8)
    p = sptamd.make_params(w, h, spp, DEPTH, camera=LENS_CAM)
    whole = aov_ref.gpu_planes(s, p)
    # depth alone, the middle third of one sentinel-filled buffer
    buf = torch.full((3, h, w), -7.0, dtype=torch.float32, device="cuda")
    got = s.render_aov(p, planes=("depth",), out={"depth": buf[1]})
    torch.cuda.synchronize()
    assert set(got) == {"depth"}
    np.testing.assert_array_equal(buf[1].cpu().numpy(), whole["depth"])
    assert torch.all(buf[0] == -7.0) and torch.all(buf[2] == -7.0)
    # a single colour plane through the C ABI
    one = torch.full((2, h, w), -7.0, dtype=torch.float32, device="cuda")
    aov = _lib.Aov()
    aov.normal_y = one[0].data_ptr()
    _lib.check(_lib.lib.spt_render_aov(s.backend.handle, ctypes.byref(p), ctypes.byref(aov), None), "spt_render_aov")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(one[0].cpu().numpy(), whole["normal"][1])
    assert torch.all(one[1] == -7.0)


def test_argument_checks():
    s = mitsuba_scene(8)
    p = sptamd.make_params(37, 19, 2, DEPTH)
    empty = _lib.Aov()
    h = s.backend.handle
    assert _lib.lib.spt_render_aov(h, ctypes.byref(p), ctypes.byref(empty), None) == _lib.SPT_ERR_INVALID
    assert _lib.lib.spt_render_aov(h, ctypes.byref(p), None, None) == _lib.SPT_ERR_INVALID
    one = torch.zeros((19, 37), dtype=torch.float32, device="cuda")
    ok = _lib.Aov()
    ok.depth = one.data_ptr()
    for field, value in (("tile_index", 1), ("tile_count", 0), ("rows_per_group", 0), ("width", 0), ("spp", 0),
                         ("rng_order", 2)):
        q = sptamd.make_params(37, 19, 2, DEPTH)
        setattr(q, field, value)
        assert _lib.lib.spt_render_aov(h, ctypes.byref(q), ctypes.byref(ok), None) == _lib.SPT_ERR_INVALID, field
    torch.cuda.synchronize()


def test_renders_around_it_keep_their_bits():
    s = mitsuba_scene(8)
    p = sptamd.make_params(48, 40, 4, 4, camera=LENS_CAM, env=(1.0, 0.9, 0.8))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        before, _ = s.render(p, stream=stream)
        planes = s.render_aov(sptamd.make_params(48, 40, 4, 4, camera=LENS_CAM), stream=stream)
        # another spp / seed in between: another jump table
        s.render_aov(sptamd.make_params(48, 40, 3, 2, camera=LENS_CAM, rng_initstate=5), stream=stream)
        after, _ = s.render(p, stream=stream)
        again = s.render_aov(sptamd.make_params(48, 40, 4, 4, camera=LENS_CAM), stream=stream)
    stream.synchronize()
    m, albedo = mitsuba()
    ref, _ = O.OracleScene(m, albedo=albedo, textures=textures()).render(
        O.reference_params(48, 40, 4, 4, camera=LENS_CAM, env=(1.0, 0.9, 0.8)))
    np.testing.assert_array_equal(before.cpu().numpy(), ref)
    np.testing.assert_array_equal(after.cpu().numpy(), ref)
    for k in PLANES:
        np.testing.assert_array_equal(planes[k].cpu().numpy(), again[k].cpu().numpy())


@pytest.mark.parametrize("width", [2, 8])
def test_lines_up_with_the_beauty_pass(width):
    """One cast, unit sky, no emitters: a sample contributes 1 exactly when its
    camera ray misses, so film == 1 - coverage bit for bit.  (spp = 4: with a
    power-of-two spp, misses / spp, hits / spp and their difference from 1 are
    all exact in f32; for spp = 5 the two sides round differently.)"""
    m = scenes.mitsuba_synth(detail=0.15)
    cfg = sptamd.default_config()
    cfg.bvh_width = width
    s = sptamd.Scene(config=cfg)
    s.add_arrays(m)
    s.commit(0)
    w, h, spp = 37, 19, 4
    film, _ = s.render(sptamd.make_params(w, h, spp, 1, camera=LENS_CAM, env=(1.0, 1.0, 1.0)))
    cov = aov_ref.gpu_planes(s, sptamd.make_params(w, h, spp, 1, camera=LENS_CAM), planes=("coverage",))["coverage"]
    torch.cuda.synchronize()
    film = film.cpu().numpy()
    assert 0 < cov.mean() < 1
    for c in range(3):
        np.testing.assert_array_equal(film[c], np.float32(1.0) - cov)
