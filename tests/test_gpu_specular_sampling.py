"""Glass, mirror spheres, textures and triangles without vertex normals under light sampling,
sky sampling and MIS on the GPU: the planes of a render are the CPU
restatement's (tests/mis_ref.py over the oracle's paths, with nee_ref's scatter weight,
reflectance and substitute normals) bit for bit and the shadow rays are counted alike — the
scenes of tests/specular_scenes.py, in which every path starts inside a glass ball, the left
wall emits, and glass and mirror surfaces stop an eighth of the shadow rays; smallpt's own
scene with an emissive quad; in every tree width and builder, through pixel lists, splits,
tiles and the pixel-major order; the counters; a texture removed and a glass ball moved
afterwards; and, statistically, the same expectation as with every switch off."""
import numpy as np
import pytest
import torch

import accum_ref as A
import specular_scenes as SS
import sptamd
from sptamd import _lib
from specular_scenes import CASES, DEPTH, H, SPP, W, expected
from test_gpu_mis import PLANES, ROT, TEX, assert_planes, planes_of, render

pytestmark = pytest.mark.gpu

BUILDS = [_lib.SPT_BUILD_HOST_SAH, _lib.SPT_BUILD_GPU_PLOC]


def make_scene(case, cfg=None, on=True, textures=True):
    """The case's scene with its samplers (on=False: every switch off)."""
    c = CASES[case]
    m, kd, ke, tex = SS.variant(c["name"])
    s = sptamd.Scene(config=cfg)
    s.add_arrays(m)
    s.commit(0)
    s.backend.set_albedo(kd)
    s.backend.set_emission(ke)
    for mat, img in (tex or {}).items() if textures else ():
        s.backend.set_texture(mat, img)
    if c["tex"] is not None:
        s.backend.set_envmap(TEX[c["tex"]], ROT)
    if on and c["nee"]:
        s.backend.set_light_sampling(True)
    if on and c["sky"]:
        s.backend.set_sky_sampling(True, c["share"])
    if on and c["mis"]:
        s.backend.set_mis(True)
    return s


def gparams(case, w=W, h=H, **kw):
    return sptamd.make_params(w, h, SPP, DEPTH, camera=SS.CAM, env=CASES[case]["env"], **SS.KW, **kw)


def config(width=None, build=None, work_order=None):
    cfg = sptamd.default_config()
    if width is not None:
        cfg.bvh_width = width
    if build is not None:
        cfg.build = build
    if work_order is not None:
        cfg.work_order = work_order
    return cfg


def check_case(case, cfg=None, msg=""):
    want, _, n = expected(case)
    got, st = planes_of(make_scene(case, cfg=cfg), gparams(case))
    assert st[0]["fused"] == 1 and st[0]["film_slots_unwritten"] == 0
    assert st[0]["shadow_casts"] == n["shadow_casts"], f"{case} {msg}"
    assert_planes(got, want, f"{case} {msg}")


# ---- 1. the planes are the restatement's

@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("width", [2, 6, 8])
@pytest.mark.parametrize("case", ["spec_lights_mis", "spec_both_mis"])
def test_glass_and_mirror_under_mis_in_every_tracer(case, width, build):
    check_case(case, config(width, build), f"width {width} build {build}")


@pytest.mark.parametrize("width", [2, 6])
@pytest.mark.parametrize("case", ["spec_lights", "spec_sky", "spec_both", "smallpt_lights", "smallpt_lights_mis",
                                  "textured_lights_mis", "textured_sky_mis", "no_normals", "some_normals"])
def test_planes_equal_the_restatement(case, width):
    check_case(case, config(width), f"width {width}")


def test_every_switch_off_is_the_oracle():
    """The fused pipeline without a sampler on the same scenes: the restatement with every switch
    off, which tests/test_specular_ref.py holds to the oracle's own radiance."""
    for case in ("spec_off", "spec_both_off"):
        want = expected(case)[0]
        got, st = planes_of(make_scene(case), gparams(case, pipeline="fused"))
        assert st[0]["fused"] == 1 and st[0]["shadow_casts"] == 0
        assert_planes(got, want, case)
    got, _ = planes_of(make_scene("spec_both_mis", on=False), gparams("spec_both_mis", pipeline="fused"))
    assert_planes(got, expected("spec_both_off")[0], "spec_both_mis, switches off")


# ---- 2. lists, splits, tiles, the work order

def test_pixel_list_after_a_full_pass():
    case = "spec_both_mis"
    want, x, _ = expected(case)
    s = make_scene(case)
    p = gparams(case)
    listed = np.sort(np.random.default_rng(31).choice(W * H, size=200, replace=False)).astype(np.int32)
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


def test_splits_and_tiles():
    case = "spec_both_mis"
    want = expected(case)[0]
    s = make_scene(case)
    got, st = planes_of(s, gparams(case), [3, 5])
    assert sum(t["shadow_casts"] for t in st) == expected(case)[2]["shadow_casts"]
    assert_planes(got, want, "split [3, 5]")
    for t in range(2):
        film, _ = render(s, gparams(case, tile_index=t, tile_count=2, rows_per_group=3))
        np.testing.assert_array_equal(film, want["film"][:, sptamd.tile_rows(H, t, 2, 3)])


def test_pixel_major_work_order():
    case = "spec_lights_mis"
    s = make_scene(case, cfg=config(work_order=_lib.SPT_WORK_PIXEL_MAJOR))
    film, st = render(s, gparams(case))
    assert st["work_order"] == _lib.SPT_WORK_PIXEL_MAJOR and st["shadow_casts"] == expected(case)[2]["shadow_casts"]
    np.testing.assert_array_equal(film, expected(case)[0]["film"])


# ---- 3. the counters

def test_the_samplers_add_shadow_rays_only():
    case = "spec_both_mis"
    _, a = render(make_scene(case), gparams(case))
    _, b = render(make_scene(case, on=False), gparams(case, pipeline="fused"))
    assert a["shadow_casts"] == expected(case)[2]["shadow_casts"] > 0 and b["shadow_casts"] == 0
    for k in ("ray_casts", "continuations", "paths", "paths_started", "paths_terminated"):
        assert a[k] == b[k], k
    assert a["paths"] == W * H * SPP and a["film_slots_unwritten"] == 0


# ---- 4. a texture removed, a glass ball moved

def test_texture_removed_and_geometry_updated_afterwards():
    s = make_scene("textured_lights_mis")
    for mat in SS.textures():
        s.backend.set_texture(mat, None)
    got, st = planes_of(s, gparams("untextured_lights_mis"))
    assert st[0]["shadow_casts"] == expected("untextured_lights_mis")[2]["shadow_casts"]
    assert_planes(got, expected("untextured_lights_mis")[0], "set_texture(mat, None) afterwards")
    m = SS.variant("moved")[0]
    for width in (2, 6):
        s = make_scene("spec_lights_mis", cfg=config(width))
        s.update_geometry(m["pos"], m["nrm"])
        assert s.backend.mis() and s.backend.light_sampling()[0]
        got, st = planes_of(s, gparams("moved"))
        assert st[0]["shadow_casts"] == expected("moved")[2]["shadow_casts"]
        assert_planes(got, expected("moved")[0], f"update_geometry afterwards, width {width}")
    check_case("moved")                          # and a fresh scene


# ---- 5. the same expectation

@pytest.mark.parametrize("case", ["expect", "expect_outside"])
def test_same_expectation(case):
    """32 x 24 of the specular scene under the broad sky image ("dim"), env 1: every switch off at
    2^16 spp against light sampling + sky sampling (share 1/2) + MIS at 2^12 spp, means and
    variances of the mean from two accumulators (DESIGN.md §14's protocol); every pixel and
    channel within z <= 5, the image mean within z <= 4; no pixel skipped.  expect_outside is
    the same scene without the glass ball around the camera.

    Measured on an MI355X (profiles/mis/variance_ratio.txt).  The null, two off renders that
    differ in rng_initstate: worst of the 2304 values z 3.56, image z 0.18 (outside: 3.30, 0.99)
    — under 4, the scene is fit for the protocol.  The test: image means 7.72563 (off) 7.77217
    (on), image z 3.12, worst value z 4.20; outside 7.62416 / 7.63340, 0.79, 4.79.
    From inside the glass ball a pixel's radiance has a heavy tail (pixel (10, 10): mean 1.23,
    a sample variance of 250, passes of 4096 samples between 0.63 and 2.04), which 2^12 samples
    do not always see: on renders with three other rng_initstate against the same off render
    gave image z -0.63, -0.34, 0.30 and worst values 9.42, 4.43, 3.85 — the 9.42 at pixel
    (10, 10), where that render's 4096 samples average 0.62 and 2^14 samples of the same state
    are back within 4.32.  Outside the ball the same three gave 3.80, 4.01, 3.79."""
    w, h = 32, 24
    res = {}
    for on, spp in ((False, 1 << 16), (True, 1 << 12)):
        acc = make_scene(case, on=on).accumulator(gparams(case, w=w, h=h))
        st = acc.add(spp)
        torch.cuda.synchronize()
        assert (st["shadow_casts"] > 0) == on
        res[on] = (acc.film.cpu().numpy().astype(np.float64), acc.variance.cpu().numpy().astype(np.float64))
    (m0, v0), (m1, v1) = res[False], res[True]
    both0 = (v0 == 0) & (v1 == 0)
    np.testing.assert_array_equal(m1[both0], m0[both0])
    z = np.abs(m1 - m0) / np.sqrt(np.where(both0, 1.0, v0 + v1))
    zi = abs(m1.mean() - m0.mean()) / np.sqrt((v0.sum() + v1.sum()) / m0.size ** 2)
    print(f"same expectation {case}: worst value z {z[~both0].max():.2f}, image z {zi:.2f}, means {m0.mean():.5f} "
          f"{m1.mean():.5f}, {int(both0.sum())} values with both variances 0")
    assert m0.mean() > 0.01
    assert z[~both0].max() <= 5.0
    assert zi <= 4.0
