"""Multiple importance sampling on the GPU (spt_scene_set_mis): the
planes of a render with the switch on are the CPU restatement's (tests/mis_ref.py
over the oracle's paths) bit for bit — the emissive triangles alone under a dark
sky, a sky constant and a sky image, the sky alone, both at share 1/2 and 1/4, in
every tree width and builder, with a mirror material, with analytic spheres as
occluder, emitter and receiver, with a member of weight 0 in the light table;
the switch without a table, or off, is the parent's path; the accumulator's
splits, pixel lists, tiles and queued renders; the order of the setters and the
table rebuilds; the counters; the refusals; the command-line host; and,
statistically, the same expectation, with less variance where the samplers
alone do worse than the bounce ray."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import accum_ref as A
import envmap_ref as E
import mis_ref as M
import nee_ref as R
import oracle as O
import sky_ref as S
import sptamd
from sptamd import _lib, scenes

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, DEPTH = 37, 19, 8, 5
DETAIL = 0.05
CAM = scenes.cornell_camera()
KW = dict(rr_start_depth=2)
PLANES = ("sum", "sum_sq", "film", "variance")
ROT = E.rotation((0.4, 1.0, -0.3), 63.0)
ONE, DARK, TINT = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.3, 0.7, 1.0)
CLI = os.path.join(os.path.dirname(_lib.LIB_PATH), "spt_render_cli")
# test_mis_lowers_the_variance_where_it_should: measured once on an MI355X, see there
MEASURED_RATIO_NEAR_PANEL = 291.52
MEASURED_RATIO_FLAT_SKY = 12.67


def sun_map(seed, toward):
    """test_gpu_sky.py's map: random_map(8) without its bright texels and one texel near 1e3."""
    tex = E.random_map(8, seed, bright=0)
    _, fx, fy = E.coords(8, ROT, np.array(toward, F))
    i, j = int(np.clip(np.rint(fx), 0, 7)), int(np.clip(np.rint(fy), 0, 7))
    tex[j, i] = (1000.0, 800.0, 600.0)
    return tex


TEX = {"sun": sun_map(21, (0.25, 0.35, 1.0)), "sun2": sun_map(22, (-0.3, 0.2, 1.0)), "dim": E.random_map(8, seed=21)}


@functools.lru_cache(maxsize=None)
def cornell():
    m = scenes.cornell_spheres(DETAIL)
    kd, ke = scenes.smallpt_materials(m)
    return m, kd, ke


def variant(name):
    """(mesh, albedo, emission) of the named scene."""
    m, kd, ke = cornell()
    m = dict(m)
    if name == "dark":                           # the cap dark: the sky is the only light
        ke = np.zeros_like(ke)
    elif name == "mirror":
        kinds = np.zeros(len(kd), np.uint32)
        kinds[4] = _lib.SPT_MAT_MIRROR
        m["kinds"] = kinds
    elif name == "spheres":                      # an occluder under the light, an emitting sphere, a diffuse receiver
        kd = np.concatenate([kd, np.array([[0.6, 0.6, 0.2]], F)])
        ke = np.concatenate([ke, np.array([[5.0, 4.0, 1.0]], F)])
        m["spheres"] = np.array([[0.5, 0.62, 0.816, 0.09], [0.2, 0.5, 1.5, 0.08], [0.75, 0.2, 1.6, 0.15]], F)
        m["sphere_mat"] = np.array([3, 6, 1], np.int32)
    elif name == "weightless":
        # the left wall "emits" (0, -0.2, 0): a member of the table (some channel is not 0) whose
        # weight area x max(Le) is 0 — never drawn, pdfA = 0, and hit by bounce rays all the time
        ke = ke.copy()
        ke[1] = (0.0, -0.2, 0.0)
    elif name == "moved":
        pos = m["pos"].copy()
        sel = np.unique(m["pos_tri"][m["mat_id"] == 5])
        pos[sel] += np.array([-0.2, -0.05, 0.1], F)
        m["pos"] = pos
    elif name == "dimmer":
        ke = ke.copy()
        ke[5] = (3.0, 6.0, 1.5)
        ke[1] = (0.0, 0.2, 0.0)
    else:
        assert name == "base"
    return m, kd, ke


# what a test renders: the scene, the sky image (None: the constant env), the two samplers, the share, env
CASES = {
    "lights": dict(name="base", tex=None, nee=True, sky=False, share=0.5, env=DARK),
    "lights_tint": dict(name="base", tex=None, nee=True, sky=False, share=0.5, env=TINT),
    "lights_image": dict(name="base", tex="dim", nee=True, sky=False, share=0.5, env=TINT),
    "sky": dict(name="dark", tex="sun", nee=False, sky=True, share=0.5, env=ONE),
    "sky_cap": dict(name="base", tex="sun", nee=False, sky=True, share=0.5, env=ONE),
    "both": dict(name="base", tex="sun", nee=True, sky=True, share=0.5, env=ONE),
    "both_quarter": dict(name="base", tex="sun", nee=True, sky=True, share=0.25, env=ONE),
    "mirror": dict(name="mirror", tex="sun", nee=True, sky=True, share=0.5, env=ONE),
    "spheres": dict(name="spheres", tex=None, nee=True, sky=False, share=0.5, env=DARK),
    "spheres_both": dict(name="spheres", tex="sun", nee=True, sky=True, share=0.5, env=TINT),
    "weightless": dict(name="weightless", tex=None, nee=True, sky=False, share=0.5, env=DARK),
    "moved": dict(name="moved", tex=None, nee=True, sky=False, share=0.5, env=DARK),
    "dimmer": dict(name="dimmer", tex=None, nee=True, sky=False, share=0.5, env=DARK),
    "sky2": dict(name="dark", tex="sun2", nee=False, sky=True, share=0.5, env=ONE),
}


def make_scene(case, mis=True, cfg=None, nee=None, sky=None, first=False):
    c = CASES[case]
    m, kd, ke = variant(c["name"])
    s = sptamd.Scene(config=cfg)
    s.add_arrays(m)
    s.commit(0)
    if first and mis:                            # the switch before anything it could act on
        s.backend.set_mis(True)
    s.backend.set_albedo(kd)
    s.backend.set_emission(ke)
    if c["tex"] is not None:
        s.backend.set_envmap(TEX[c["tex"]], ROT)
    if c["nee"] if nee is None else nee:
        s.backend.set_light_sampling(True)
    if c["sky"] if sky is None else sky:
        s.backend.set_sky_sampling(True, c["share"])
    if mis and not first:
        s.backend.set_mis(True)
    assert s.backend.mis() == bool(mis)
    return s


def oparams(case, w=W, h=H):
    return O.reference_params(w, h, SPP, DEPTH, camera=CAM, env=CASES[case]["env"], **KW)


def gparams(case, w=W, h=H, **kw):
    return sptamd.make_params(w, h, SPP, DEPTH, camera=CAM, env=CASES[case]["env"], **KW, **kw)


@functools.lru_cache(maxsize=None)
def expected(case, mis=True, nee=None, sky=None):
    """The planes, the contributions and the counts of the restatement."""
    c = CASES[case]
    m, kd, ke = variant(c["name"])
    count = {}
    x = M.contributions(m, oparams(case), kd, ke, sky=None if c["tex"] is None else (TEX[c["tex"]], ROT),
                        nee=c["nee"] if nee is None else nee, sky_on=c["sky"] if sky is None else sky, share=c["share"],
                        mis=mis, count=count)
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


def check_case(case, cfg=None, msg=""):
    want, _, n = expected(case)
    got, st = planes_of(make_scene(case, cfg=cfg), gparams(case))
    assert st[0]["fused"] == 1 and st[0]["film_slots_unwritten"] == 0
    assert st[0]["shadow_casts"] == n["shadow_casts"], f"{case} {msg}"
    assert_planes(got, want, f"{case} {msg}")


# ---- 1. the planes are the restatement's

def test_the_restatement_differs():
    for case in ("lights", "lights_tint", "lights_image", "sky", "sky_cap", "both", "both_quarter", "mirror", "spheres",
                 "spheres_both", "weightless"):
        on, _, n = expected(case)
        off, _, m = expected(case, mis=False)
        assert not np.array_equal(on["film"], off["film"]), case
        c = CASES[case]
        assert (n["weighted_hits"] > 100) == c["nee"] and (n["weighted_escapes"] > 100) == c["sky"], (case, n)
        # no ray more; a factor that underflows where cx / cl did not may trace a few fewer
        assert 0 < n["shadow_casts"] <= m["shadow_casts"] and n["shadow_casts"] > 0.99 * m["shadow_casts"], case
    # the share is inside the weights, the mirror clears the marks, the weightless wall counts in full
    assert not np.array_equal(expected("both")[0]["film"], expected("both_quarter")[0]["film"])
    assert not np.array_equal(expected("mirror")[0]["film"], expected("both")[0]["film"])
    assert expected("mirror")[2]["weighted_hits"] < expected("both")[2]["weighted_hits"]
    g_on, g_off = expected("weightless")[1][:, 1], expected("weightless", mis=False)[1][:, 1]
    assert g_on.min() < 0 and g_on.sum() < g_off.sum()         # the wall's negative green, dropped after a vertex without MIS


@pytest.mark.parametrize("build", [_lib.SPT_BUILD_HOST_SAH, _lib.SPT_BUILD_GPU_PLOC])
@pytest.mark.parametrize("width", [2, 6, 8])
def test_planes_equal_the_restatement(width, build):
    for case in ("lights", "sky", "both", "both_quarter"):
        cfg = sptamd.default_config()
        cfg.bvh_width, cfg.build = width, build
        check_case(case, cfg, f"width {width} build {build}")
    cfg = sptamd.default_config()
    cfg.bvh_width, cfg.build, cfg.work_order = width, build, _lib.SPT_WORK_PIXEL_MAJOR
    s = make_scene("both", cfg=cfg)
    film, st = render(s, gparams("both"))
    assert st["work_order"] == _lib.SPT_WORK_PIXEL_MAJOR
    np.testing.assert_array_equal(film, expected("both")[0]["film"])


@pytest.mark.parametrize("case", ["lights_tint", "lights_image", "sky_cap"])
def test_sky_constant_sky_image_and_an_unsampled_cap(case):
    """A sky constant and an unsampled sky image count in full at an escape; with the sky
    sampled and the cap not, the cap's emission counts in full at a hit."""
    for width in (2, 6, 8):
        cfg = sptamd.default_config()
        cfg.bvh_width = width
        check_case(case, cfg, f"width {width}")


def test_mirror_material_clears_the_marks():
    check_case("mirror")


@pytest.mark.parametrize("case", ["spheres", "spheres_both"])
def test_analytic_spheres_occlude_emit_and_receive(case):
    for width in (2, 6):
        cfg = sptamd.default_config()
        cfg.bvh_width = width
        check_case(case, cfg, f"width {width}")


def test_a_member_of_weight_zero_counts_in_full():
    s = make_scene("weightless")
    assert s.backend.light_sampling() == (True, 28 + 32)
    for width in (2, 6, 8):
        cfg = sptamd.default_config()
        cfg.bvh_width = width
        check_case("weightless", cfg, f"width {width}")


# ---- 2. inert cases

def test_without_a_table_or_switched_off_it_is_the_parent():
    # both samplers off: the switch alone changes nothing, and the wavefront still runs
    for case in ("lights", "both"):
        p = gparams(case)
        ref, sr = planes_of(make_scene(case, mis=False, nee=False, sky=False), p)
        s = make_scene(case, nee=False, sky=False)
        got, st = planes_of(s, p)
        assert_planes(got, ref, f"{case}: no sampler")
        assert_planes(got, expected(case, nee=False, sky=False)[0], f"{case}: no sampler, the restatement")
        for k in ("fused", "shadow_casts", "ray_casts", "continuations"):
            assert st[0][k] == sr[0][k], k
        film, st = render(s, gparams(case, pipeline="wavefront"))
        assert st["fused"] == 0
        np.testing.assert_array_equal(film, ref["film"])
    # both samplers on, both tables empty: no emission, no map
    s = make_scene("lights", mis=True)
    s.backend.set_emission(np.zeros((1, 3), F))
    s.backend.set_sky_sampling(True)
    assert s.backend.light_sampling() == (True, 0) and s.backend.sky_sampling() == (True, 0.5, 0) and s.backend.mis()
    t = make_scene("lights", mis=False, nee=False)
    t.backend.set_emission(np.zeros((1, 3), F))
    p = gparams("lights_tint")
    got, st = planes_of(s, p)
    assert_planes(got, planes_of(t, p)[0], "empty tables")
    assert st[0]["shadow_casts"] == 0 and render(s, gparams("lights_tint", pipeline="wavefront"))[1]["fused"] == 0
    # the switch off: today's samplers (nee_ref and sky_ref themselves), before and after a toggle
    m, kd, ke = variant("base")
    for case, want in (("lights", R.contributions(m, oparams("lights"), kd, ke)),
                       ("both_quarter", S.contributions(m, oparams("both_quarter"), kd, ke, (TEX["sun"], ROT), nee=True,
                                                        share=0.25))):
        want = dict(zip(PLANES, A.moments(want)))
        assert_planes(expected(case, mis=False)[0], want, f"{case}: mis_ref off")
        s = make_scene(case, mis=False)
        assert_planes(planes_of(s, gparams(case))[0], want, f"{case}: never on")
        s.backend.set_mis(True)
        s.backend.set_mis(False)
        assert_planes(planes_of(s, gparams(case))[0], want, f"{case}: on and off again")


# ---- 3. accumulator splits, lists, tiles, queued renders

@pytest.mark.parametrize("case", ["lights", "both"])
def test_splits_lists_tiles_and_the_setter_between_queued_renders(case):
    want, x, _ = expected(case)
    s = make_scene(case)
    p = gparams(case)
    for split in ([3, 5], [1] * 8):
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
        film, _ = render(s, gparams(case, tile_index=t, tile_count=2, rows_per_group=3))
        np.testing.assert_array_equal(film, want["film"][:, sptamd.tile_rows(H, t, 2, 3)])
    # a render queued before the switch goes off keeps its estimator
    q = sptamd.queue_stream()
    film1, ticket = s.render_async(p, stream=q)
    s.backend.set_mis(False)
    film2, _ = s.render(p)
    s.render_wait(ticket)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(film1.cpu().numpy(), want["film"])
    np.testing.assert_array_equal(film2.cpu().numpy(), expected(case, mis=False)[0]["film"])


# ---- 4. the order of the setters, and the table rebuilds

def test_setter_order_and_table_rebuilds():
    for case in ("lights", "both_quarter"):
        got, _ = planes_of(make_scene(case, first=True), gparams(case))
        assert_planes(got, expected(case)[0], f"{case}: the switch first")
    s = make_scene("lights")
    s.backend.set_emission(variant("dimmer")[2])
    assert s.backend.light_sampling() == (True, 28 + 32) and s.backend.mis()
    got, st = planes_of(s, gparams("dimmer"))
    assert st[0]["shadow_casts"] == expected("dimmer")[2]["shadow_casts"]
    assert_planes(got, expected("dimmer")[0], "set_emission afterwards")
    s = make_scene("lights")
    m = variant("moved")[0]
    s.update_geometry(m["pos"], m["nrm"])
    assert s.backend.mis()
    assert_planes(planes_of(s, gparams("moved"))[0], expected("moved")[0], "update_geometry afterwards")
    s = make_scene("sky")
    s.backend.set_envmap(TEX["sun2"], ROT)
    assert s.backend.sky_sampling() == (True, 0.5, 64) and s.backend.mis()
    assert not np.array_equal(expected("sky2")[0]["film"], expected("sky")[0]["film"])
    assert_planes(planes_of(s, gparams("sky2"))[0], expected("sky2")[0], "set_envmap afterwards")
    s.backend.set_envmap(None)                                   # the table empties; the switch stays and is inert
    t = make_scene("lights", mis=False, nee=False)
    t.backend.set_emission(np.zeros_like(variant("base")[2]))
    assert s.backend.mis()
    assert_planes(planes_of(s, gparams("sky"))[0], planes_of(t, gparams("sky"))[0], "the map removed")


# ---- 5. counters and refusals

@pytest.mark.parametrize("case", ["lights", "both"])
def test_shadow_casts_and_ray_casts(case):
    n = expected(case)[2]
    _, a = render(make_scene(case), gparams(case))
    _, b = render(make_scene(case, mis=False), gparams(case))
    _, c = render(make_scene(case, mis=False, nee=False, sky=False), gparams(case, pipeline="fused"))
    assert a["shadow_casts"] == n["shadow_casts"] and c["shadow_casts"] == 0
    assert b["shadow_casts"] == expected(case, mis=False)[2]["shadow_casts"] >= a["shadow_casts"]
    for k in ("ray_casts", "continuations", "paths", "paths_started", "paths_terminated"):
        assert a[k] == b[k] == c[k], k
    assert a["paths"] == W * H * SPP and a["film_slots_unwritten"] == 0


def test_refusals(tmp_path):
    s = make_scene("lights")
    film0, _ = render(s, gparams("lights"))
    h = s.backend.handle
    assert _lib.lib.spt_scene_set_mis(h, 2) == _lib.SPT_ERR_INVALID and b"on = 2" in _lib.lib.spt_last_error()
    assert _lib.lib.spt_scene_set_mis(None, 1) == _lib.SPT_ERR_INVALID and b"NULL scene" in _lib.lib.spt_last_error()
    assert _lib.lib.spt_scene_get_mis(None, None) == _lib.SPT_ERR_INVALID
    assert s.backend.mis()
    np.testing.assert_array_equal(render(s, gparams("lights"))[0], film0)
    # as for the samplers alone: the fused pipeline only
    with pytest.raises(sptamd.SptError) as e:
        s.render(gparams("lights", pipeline="wavefront"))
    assert e.value.code == _lib.SPT_ERR_INVALID and "light sampling" in str(e.value)
    # the cache does not store the switch, and is not refused on its account alone
    path = str(tmp_path / "scene.sptc")
    with pytest.raises(sptamd.SptError) as e:
        s.save(path)
    assert "light sampling" in str(e.value) and not os.path.exists(path)
    s.backend.set_light_sampling(False)
    assert s.backend.mis()
    s.save(path)
    t = sptamd.Scene.load(path)
    assert not t.backend.mis()
    t.backend.set_light_sampling(True)
    np.testing.assert_array_equal(render(t, gparams("lights"))[0], expected("lights", mis=False)[0]["film"])


# ---- 6. the command-line host

def test_cli_nee_mis_equals_the_python_api(tmp_path):
    w, h, d, spp = 40, 24, 4, 4
    s = sptamd.Scene()
    s.add_triangle_mesh(scenes.scene_pbrt("cornell_spheres", DETAIL))
    s.commit(0)
    kd, ke = scenes.smallpt_materials(s.mesh)
    s.backend.set_albedo(kd)
    s.backend.set_emission(ke)
    path, oct_pfm = str(tmp_path / "cornell.sptc"), str(tmp_path / "oct.pfm")
    s.save(path)
    sptamd.write_pfm(oct_pfm, np.ascontiguousarray(TEX["sun"].transpose(2, 0, 1)))
    sky = ["--envmap-oct", oct_pfm]

    def cli(out, *flags, ok=True):
        r = subprocess.run([CLI, "-w", str(w), "-h", str(h), "-d", str(d), "-s", str(spp), "--rr", "2", path, "-o", out]
                           + list(flags), capture_output=True, text=True, timeout=180)
        if not ok:
            return r
        assert r.returncode == 0, r.stdout + r.stderr
        return sptamd.read_pfm(out).transpose(2, 0, 1)

    p = sptamd.make_params(w, h, spp, d, camera=s.pbrt_info["camera"], rr_start_depth=2)
    s.backend.set_light_sampling(True)
    plain, _ = render(s, p)
    s.backend.set_mis(True)
    want, st = render(s, p)
    assert st["shadow_casts"] > 0 and not np.array_equal(want, plain)
    np.testing.assert_array_equal(cli(str(tmp_path / "nee.pfm"), "--nee"), plain)
    np.testing.assert_array_equal(cli(str(tmp_path / "on.pfm"), "--nee", "--mis"), want)
    np.testing.assert_array_equal(cli(str(tmp_path / "acc.pfm"), "--mis", "--nee", "-s", "2", "--passes", "2"), want)
    s.backend.set_envmap(TEX["sun"], np.eye(3, dtype=F))
    s.backend.set_sky_sampling(True, 0.25)
    both, _ = render(s, p)
    assert not np.array_equal(both, want)
    np.testing.assert_array_equal(cli(str(tmp_path / "both.pfm"), *sky, "--sky-nee", "--nee", "--sky-share", "0.25", "--mis"), both)
    # --mis alone, and beside a map without a sampler: a usage error, nothing written
    for flags in (["--mis"], sky + ["--mis"]):
        r = cli(str(tmp_path / "no.pfm"), *flags, ok=False)
        assert r.returncode == 2 and "--mis" in r.stderr and not os.path.exists(str(tmp_path / "no.pfm")), flags


# ---- 7. the same expectation

@pytest.mark.parametrize("case", ["lights", "sky", "both"])
def test_same_expectation(case):
    """32 x 24: every switch off at 2^16 spp against the samplers and MIS at 2^12 spp, means and
    variances of the mean from two accumulators (DESIGN.md §14's protocol); every pixel and
    channel within z <= 5, the image mean within z <= 4; no pixel skipped.

    Measured on an MI355X (profiles/mis/variance_ratio.txt): lights, image means 0.07741 (off)
    0.07720 (on), image z 1.49, worst of the 2304 values z 3.97; sky 4.49545 / 4.50375, 1.82, 4.17;
    both 4.57286 / 4.58721, 2.64, 3.73 (the three share their paths and their off renders)."""
    w, h = 32, 24
    res = {}
    for on, spp in ((False, 1 << 16), (True, 1 << 12)):
        s = make_scene(case, mis=on, nee=None if on else False, sky=None if on else False)
        acc = s.accumulator(gparams(case, w=w, h=h))
        acc.add(spp)
        torch.cuda.synchronize()
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


# ---- 8. less variance where it should be

def quads(*qs):
    """A mesh of quads (corner, eu, ev, normal, material): two triangles each, the normal as given."""
    pos, nrm, pt, nt, mat = [], [], [], [], []
    for k, (c, eu, ev, n, m) in enumerate(qs):
        c, eu, ev = (np.array(a, np.float64) for a in (c, eu, ev))
        pos += [c, c + eu, c + eu + ev, c + ev]
        nrm.append(n)
        pt += [(4 * k, 4 * k + 1, 4 * k + 2), (4 * k, 4 * k + 2, 4 * k + 3)]
        nt += [(k, k, k)] * 2
        mat += [m] * 2
    return dict(pos=np.array(pos, F), nrm=np.array(nrm, F), pos_tri=np.array(pt, np.int32), nrm_tri=np.array(nt, np.int32),
                mat_id=np.array(mat, np.int32))


def near_panel():
    """(a) a 2 x 2 diffuse floor and a 1 x 1 emissive panel 0.05 above it, seen from inside the
    gap: the lower half of the image is floor no farther than 0.05 from the light."""
    mesh = quads(((-1, 0, -1), (0, 0, 2), (2, 0, 0), (0, 1, 0), 0), ((-0.5, 0.05, -0.5), (1, 0, 0), (0, 0, 1), (0, -1, 0), 1))
    kd = np.array([[0.75, 0.75, 0.75], [0, 0, 0]], F)
    ke = np.array([[0, 0, 0], [12, 12, 12]], F)
    cam = dict(CAM, look_from=(0.0, 0.025, 0.45), look_at=(0.0, 0.02, -1.0))
    return mesh, kd, ke, None, cam, DARK


def flat_sky():
    """(b) a floor and a low wall, open to a sky image whose texels lie within 10 % of their mean."""
    mesh = quads(((-2, 0, -2), (0, 0, 4), (4, 0, 0), (0, 1, 0), 0), ((-1, 0, -0.5), (2, 0, 0), (0, 0.6, 0), (0, 0, 1), 1))
    kd = np.array([[0.75, 0.75, 0.75], [0.6, 0.3, 0.3]], F)
    tex = (1.0 + 0.09 * np.random.default_rng(5).uniform(-1, 1, size=(8, 8, 3))).astype(F)
    assert np.abs(tex / tex.mean() - 1).max() <= 0.1
    cam = dict(CAM, look_from=(0.3, 1.2, 2.5), look_at=(0.0, 0.1, 0.0))
    return mesh, kd, None, tex, cam, ONE


def variance_of(scene, mis, spp=64):
    mesh, kd, ke, tex, cam, env = scene
    s = sptamd.Scene()
    s.add_arrays(mesh)
    s.commit(0)
    s.backend.set_albedo(kd)
    if ke is not None:
        s.backend.set_emission(ke)
        s.backend.set_light_sampling(True)
    if tex is not None:
        s.backend.set_envmap(tex, ROT)
        s.backend.set_sky_sampling(True)
    s.backend.set_mis(mis)
    acc = s.accumulator(sptamd.make_params(W, H, SPP, DEPTH, camera=cam, env=env, **KW))
    st = acc.add(spp)
    torch.cuda.synchronize()
    assert st["shadow_casts"] > 0
    return float(acc.variance.cpu().numpy().astype(np.float64).mean()), float(acc.film.cpu().numpy().astype(np.float64).mean())


@pytest.mark.parametrize("which", ["near_panel", "flat_sky"])
def test_mis_lowers_the_variance_where_it_should(which):
    """64 spp, 37 x 19: the image mean of the variance plane with the sampler alone over the one
    with MIS.  Measured once on an MI355X (profiles/mis/variance_ratio.txt):
    near_panel 24.4164 / 0.0837569 = 291.52, flat_sky 0.00872471 / 0.000688594 = 12.67; half of each
    is asserted, as §14 did.  The restatement on the CPU at 16 spp gives 228.6 and 12.77."""
    scene = near_panel() if which == "near_panel" else flat_sky()
    measured = MEASURED_RATIO_NEAR_PANEL if which == "near_panel" else MEASURED_RATIO_FLAT_SKY
    (v0, m0), (v1, m1) = variance_of(scene, False), variance_of(scene, True)
    ratio = v0 / v1
    print(f"{which}: variance sampler alone {v0:.6g} (image mean {m0:.5f}), with mis {v1:.6g} ({m1:.5f}), ratio {ratio:.2f}")
    assert measured is not None, "the ratio has not been measured"
    assert measured >= 1.5, "the scene does not show what it was built to show"
    assert ratio >= measured / 2


def test_cornell_variance_with_and_without_mis_is_finite():
    """The regular test render under light sampling, 64 spp: reported (profiles/mis/variance_ratio.txt),
    not asserted — MIS may cost a little where light sampling alone was already right."""
    v = {}
    for mis in (False, True):
        acc = make_scene("lights", mis=mis).accumulator(gparams("lights"))
        acc.add(64)
        torch.cuda.synchronize()
        v[mis] = float(acc.variance.cpu().numpy().astype(np.float64).mean())
    print(f"cornell_spheres --nee: variance without mis {v[False]:.6g}, with mis {v[True]:.6g}, ratio {v[False] / v[True]:.3f}")
    assert np.isfinite(v[False]) and np.isfinite(v[True]) and v[True] > 0
