"""Light sampling on the GPU (spt_scene_set_light_sampling): the
planes of a render with the switch on are the CPU restatement's
(tests/nee_ref.py over the oracle's paths) bit for bit — in every tree width and
builder, both work orders, under a sky constant and a sky image, with a mirror
material, with analytic spheres as occluder, emitter and receiver (bit-equal:
the shadow ray's sphere test is the oracle's own, through oracle_intersect) —
an empty table is the switch off; the accumulator's splits, pixel lists, tiles
and queued renders; geometry and emission updates rebuild the table; the
refusals; the counters; the LDS guard; and, statistically, the same expectation
with less variance."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import accum_ref as A
import envmap_ref as E
import hostile
import nee_ref as R
import oracle as O
import sptamd
from sptamd import _lib, scenes

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP, DEPTH = 37, 19, 8, 5
DETAIL = 0.05            # the cap keeps its 28 triangles at every detail <= 1/16
CAM = scenes.cornell_camera()
KW = dict(rr_start_depth=2)
PLANES = ("sum", "sum_sq", "film", "variance")
TEX = E.random_map(8, seed=21)
ROT = E.rotation((0.4, 1.0, -0.3), 63.0)
CLI = os.path.join(os.path.dirname(_lib.LIB_PATH), "spt_render_cli")
# test_light_sampling_lowers_the_variance: measured once on an MI355X, see there
MEASURED_VARIANCE_RATIO = 4.47


@functools.lru_cache(maxsize=None)
def cornell():
    m = scenes.cornell_spheres(DETAIL)
    kd, ke = scenes.smallpt_materials(m)
    assert int((ke[m["mat_id"]].max(axis=1) > 0).sum()) >= 8
    return m, kd, ke


def variant(name):
    """(mesh, albedo, emission) of the named scene."""
    m, kd, ke = cornell()
    m = dict(m)
    if name == "mirror":                         # the tessellated spheres' material reflects
        kinds = np.zeros(len(kd), np.uint32)
        kinds[4] = _lib.SPT_MAT_MIRROR
        m["kinds"] = kinds
    elif name in ("spheres", "sphere_emitter_only"):
        kd = np.concatenate([kd, np.array([[0.6, 0.6, 0.2]], F)])
        ke = np.concatenate([ke, np.array([[5.0, 4.0, 1.0]], F)])
        # an occluder under the light, an emitting sphere, a diffuse receiver
        m["spheres"] = np.array([[0.5, 0.62, 0.816, 0.09], [0.2, 0.5, 1.5, 0.08], [0.75, 0.2, 1.6, 0.15]], F)
        m["sphere_mat"] = np.array([3, 6, 1], np.int32)
        if name == "sphere_emitter_only":
            ke = ke.copy()
            ke[5] = 0
    elif name == "moved":                        # the light cap 0.2 to the left and a little lower
        pos = m["pos"].copy()
        sel = np.unique(m["pos_tri"][m["mat_id"] == 5])
        pos[sel] += np.array([-0.2, -0.05, 0.1], F)
        m["pos"] = pos
    elif name == "dimmer":
        ke = ke.copy()
        ke[5] = (3.0, 6.0, 1.5)
        ke[1] = (0.0, 0.2, 0.0)                  # the left wall glows: 32 more lights
    else:
        assert name == "base"
    return m, kd, ke


def make_scene(name="base", cfg=None, nee=True, sky=False):
    m, kd, ke = variant(name)
    s = sptamd.Scene(config=cfg)
    s.add_arrays(m)
    s.commit(0)
    s.backend.set_albedo(kd)
    s.backend.set_emission(ke)
    if sky:
        s.backend.set_envmap(TEX, ROT)
    if nee:
        s.backend.set_light_sampling(True)
    return s


def oparams(spp=SPP, env=(0.0, 0.0, 0.0), w=W, h=H):
    return O.reference_params(w, h, spp, DEPTH, camera=CAM, env=env, **KW)


def gparams(spp=SPP, env=(0.0, 0.0, 0.0), w=W, h=H, **kw):
    return sptamd.make_params(w, h, spp, DEPTH, camera=CAM, env=env, **KW, **kw)


@functools.lru_cache(maxsize=None)
def expected(name="base", env=(0.0, 0.0, 0.0), sky=False, on=True):
    """The planes, the contributions and the shadow-ray count of the restatement."""
    m, kd, ke = variant(name)
    count = {}
    x = R.contributions(m, oparams(env=env), kd, ke, sky=(TEX, ROT) if sky else None, on=on, count=count)
    assert np.isfinite(x).all()
    return dict(zip(PLANES, A.moments(x))), x, count.get("shadow_casts", 0)


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

def test_the_restatement_differs_from_the_plain_estimator_and_from_itself_without_the_bit():
    on, x, n = expected()
    off = expected(on=False)[0]
    assert n > 5000 and not np.array_equal(on["film"], off["film"])
    assert (x > 0).mean() > 10 * (expected(on=False)[1] > 0).mean()      # most paths now carry light


@pytest.mark.parametrize("build", [_lib.SPT_BUILD_HOST_SAH, _lib.SPT_BUILD_GPU_PLOC])
@pytest.mark.parametrize("width", [2, 6, 8])
def test_planes_equal_the_restatement(width, build):
    want, _, nshadow = expected()
    for order in (_lib.SPT_WORK_SAMPLE_MAJOR, _lib.SPT_WORK_PIXEL_MAJOR):
        cfg = sptamd.default_config()
        cfg.bvh_width, cfg.build, cfg.work_order = width, build, order
        s = make_scene(cfg=cfg)
        assert s.backend.stats["bvh_width"] == width and s.backend.light_sampling() == (True, 28)
        got, st = planes_of(s, gparams())
        assert st[0]["fused"] == 1 and st[0]["work_order"] == order and st[0]["film_slots_unwritten"] == 0
        assert st[0]["shadow_casts"] == nshadow
        assert_planes(got, want, f"width {width} build {build} order {order}")
        film, _ = render(s, gparams())
        np.testing.assert_array_equal(film, want["film"])


def test_sky_constant_and_sky_image():
    env = (0.3, 0.7, 1.0)
    want = expected(env=env)[0]
    assert not np.array_equal(want["film"], expected()[0]["film"])       # paths do leave through the open front
    got, _ = planes_of(make_scene(), gparams(env=env))
    assert_planes(got, want, "sky constant")
    want = expected(env=env, sky=True)[0]
    assert not np.array_equal(want["film"], expected(env=env)[0]["film"])
    for width in (2, 6, 8):
        cfg = sptamd.default_config()
        cfg.bvh_width = width
        got, _ = planes_of(make_scene(cfg=cfg, sky=True), gparams(env=env))
        assert_planes(got, want, f"sky image width {width}")


def test_mirror_material_clears_the_emission_bit():
    want, x, n = expected("mirror")
    assert not np.array_equal(want["film"], expected()[0]["film"]) and 0 < n < expected()[2]
    got, st = planes_of(make_scene("mirror"), gparams())
    assert st[0]["shadow_casts"] == n
    assert_planes(got, want, "mirror")


def test_analytic_spheres_occlude_emit_and_receive():
    want, x, n = expected("spheres")
    assert not np.array_equal(want["film"], expected()[0]["film"])
    for width in (2, 6):
        cfg = sptamd.default_config()
        cfg.bvh_width = width
        got, st = planes_of(make_scene("spheres", cfg=cfg), gparams())
        assert st[0]["shadow_casts"] == n
        assert_planes(got, want, f"spheres width {width}")


# ---- 2. an empty table is the switch off

def test_empty_tables_are_inert():
    m, kd, ke = variant("base")
    p = gparams()
    # an emitting sphere and no emitting triangle; then no emission at all
    for name, emi in (("sphere_emitter_only", None), ("base", np.zeros_like(ke))):
        off = make_scene(name, nee=False)
        on = make_scene(name, nee=False)
        if emi is not None:
            off.backend.set_emission(emi)
            on.backend.set_emission(emi)
        on.backend.set_light_sampling(True)
        assert on.backend.light_sampling() == (True, 0)
        a, sa = planes_of(off, p)
        b, sb = planes_of(on, p)
        assert_planes(b, a, name)
        assert sb[0]["shadow_casts"] == 0 and sb[0]["ray_casts"] == sa[0]["ray_casts"]
        # inert: the wavefront still runs
        film, st = render(on, gparams(pipeline="wavefront"))
        assert st["fused"] == 0
        np.testing.assert_array_equal(film, a["film"])
    assert a["film"].max() == 0                   # (the second scene is black)
    # switching off again gives the parent's estimator, bit for bit
    s = make_scene()
    s.backend.set_light_sampling(False)
    assert s.backend.light_sampling() == (False, 0)
    got, st = planes_of(s, p)
    assert_planes(got, expected(on=False)[0], "switched off")
    assert st[0]["shadow_casts"] == 0


# ---- 3. accumulator splits, lists, tiles, queued renders

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
    # two tiles of interleaved row groups give the one-tile image
    for t in range(2):
        film, _ = render(s, gparams(tile_index=t, tile_count=2, rows_per_group=3))
        np.testing.assert_array_equal(film, want["film"][:, sptamd.tile_rows(H, t, 2, 3)])
    # a render queued before the switch goes off keeps its estimator
    q = sptamd.queue_stream()
    film1, ticket = s.render_async(p, stream=q)
    s.backend.set_light_sampling(False)
    film2, _ = s.render(p)
    s.render_wait(ticket)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(film1.cpu().numpy(), want["film"])
    np.testing.assert_array_equal(film2.cpu().numpy(), expected(on=False)[0]["film"])


# ---- 4. updates rebuild the table

def test_update_geometry_moves_the_light():
    want = expected("moved")[0]
    assert not np.array_equal(want["film"], expected()[0]["film"])
    s = make_scene()
    m = variant("moved")[0]
    s.update_geometry(m["pos"], m["nrm"])
    got, _ = planes_of(s, gparams())
    assert_planes(got, want, "moved by update_geometry")
    fresh, _ = planes_of(make_scene("moved"), gparams())
    assert_planes(got, fresh, "a fresh scene at the new positions")


def test_set_emission_afterwards_changes_the_table():
    want, _, n = expected("dimmer")
    s = make_scene()
    s.backend.set_emission(variant("dimmer")[2])
    assert s.backend.light_sampling() == (True, 28 + 32)
    got, st = planes_of(s, gparams())
    assert st[0]["shadow_casts"] == n
    assert_planes(got, want, "set_emission after the switch")
    s.backend.set_emission(np.zeros((1, 3), F))           # no emitters: the table empties, the switch stays
    assert s.backend.light_sampling() == (True, 0)
    assert planes_of(s, gparams())[0]["film"].max() == 0


# ---- 5. refusals

def test_refusals(tmp_path):
    s = make_scene()
    film0, _ = render(s, gparams())
    for kw in (dict(pipeline="wavefront"),):
        with pytest.raises(sptamd.SptError) as e:
            s.render(gparams(**kw))
        assert e.value.code == _lib.SPT_ERR_INVALID and "light sampling" in str(e.value)
    p = gparams()
    p.flags |= _lib.SPT_FLAG_TRAVERSAL_STATS
    with pytest.raises(sptamd.SptError) as e:
        s.render(p)
    assert e.value.code == _lib.SPT_ERR_INVALID and "light sampling" in str(e.value)
    path = str(tmp_path / "scene.sptc")
    with pytest.raises(sptamd.SptError) as e:
        s.save(path)
    assert e.value.code == _lib.SPT_ERR_INVALID and "light sampling" in str(e.value) and not os.path.exists(path)
    assert _lib.lib.spt_scene_set_light_sampling(s.backend.handle, 7) == _lib.SPT_ERR_INVALID
    again, _ = render(s, gparams())
    np.testing.assert_array_equal(again, film0)
    # the config's pipeline choice does not matter either
    cfg = sptamd.default_config()
    cfg.pipeline = _lib.SPT_PIPELINE_WAVEFRONT
    film, st = render(make_scene(cfg=cfg), gparams())
    assert st["fused"] == 1
    np.testing.assert_array_equal(film, film0)
    # off: the file is the one the scene wrote before it ever had the switch (the header holds
    # the build's own time, so the two files come from one scene), and loads into a scene that takes it
    u = make_scene(nee=False)
    plain = str(tmp_path / "plain.sptc")
    u.save(plain)
    u.backend.set_light_sampling(True)
    u.backend.set_light_sampling(False)
    u.save(path)
    assert open(path, "rb").read() == open(plain, "rb").read()
    t = sptamd.Scene.load(path)
    t.backend.set_light_sampling(True)
    assert t.backend.light_sampling() == (True, 28)
    np.testing.assert_array_equal(render(t, gparams())[0], film0)


# ---- 6. the counters

def test_shadow_casts_and_ray_casts():
    _, _, n = expected()
    on, off = make_scene(), make_scene(nee=False)
    _, a = render(on, gparams())
    _, b = render(off, gparams(pipeline="fused"))
    assert a["shadow_casts"] == n and b["shadow_casts"] == 0
    for k in ("ray_casts", "continuations", "paths", "paths_started", "paths_terminated"):
        assert a[k] == b[k], k
    assert a["paths"] == W * H * SPP and a["film_slots_unwritten"] == 0


# ---- 7. the LDS guard

def test_lds_guard_counts_the_larger_park():
    """A tree whose stack fits the device's LDS beside the plain kernels' 32 B per
    lane and not beside the light-sampling kernels' 64 B: the setter answers
    SPT_ERR_LIMIT and launches nothing; eight entries fewer, it renders.  The
    tree is hostile.coincident's: exact copies of one triangle have equal Morton
    codes, so the GPU builder's tree is a chain whose depth grows with their
    number — found here by bisection for the device's LDS size (stack_slack adds
    the last entries)."""
    cap = torch.cuda.get_device_properties(0).shared_memory_per_block
    block, wide = 128, 2 * 128 * 16
    entries = (cap - wide - block * 32) // (block * 4)          # the deepest stack the plain kernels take
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
        except sptamd.SptError as e:                            # deeper than the device takes at all
            assert e.code == _lib.SPT_ERR_LIMIT
            have = entries + 1
        print(f"{n} copies: {have} stack entries of {entries}")
        if entries - 64 <= have <= entries - 8:
            chosen = (n, entries - have)
            break
        lo, hi = (n, hi) if have < entries - 64 else (lo, n)
    assert chosen, f"no stack of copies reaches {entries} stack entries with 8 <= stack_slack <= 64 (LDS {cap} B)"
    n, slack = chosen
    cam = hostile.camera("coincident")
    p = sptamd.make_params(16, 8, 2, 3, camera=cam, env=(0, 0, 0), **KW)

    def lit(s):
        s.backend.set_albedo(np.array([[0.7, 0.7, 0.7]], F))
        s.backend.set_emission(np.array([[1.0, 1.0, 1.0]], F))
        return s

    s = lit(deep(n, slack))
    film0, _ = render(s, p)
    with pytest.raises(sptamd.SptError) as e:
        s.backend.set_light_sampling(True)
    assert e.value.code == _lib.SPT_ERR_LIMIT and "LDS" in str(e.value) and "light sampling" in str(e.value)
    assert s.backend.light_sampling() == (False, 0)
    np.testing.assert_array_equal(render(s, p)[0], film0)
    t = lit(deep(n, slack - 8))
    t.backend.set_light_sampling(True)
    assert t.backend.light_sampling() == (True, n)
    film, st = render(t, p)
    assert st["fused"] == 1 and st["film_slots_unwritten"] == 0 and np.isfinite(film).all()


# ---- 8. the same expectation, with less variance

def test_same_expectation():
    """32 x 24: the switch off at 2^16 spp against on at 2^12 spp, means and variances of
    the mean from two accumulators; every pixel and channel within z <= 5
    (tests/independent.py's bound), the image mean likewise; no pixel skipped.

    Measured on an MI355X: image means 0.07741 (off) and 0.07722 (on), image z 1.33,
    worst pixel z 3.93.  (Light sampling weighs with the bounce sampler's own
    density, DESIGN.md §14: with the textbook cosine of the normalised normal
    one pixel on a tessellated sphere, shading normals of length 0.92, stood at
    z = 5.26.)"""
    w, h = 32, 24
    res = {}
    for on, spp in ((False, 1 << 16), (True, 1 << 12)):
        acc = make_scene(nee=on).accumulator(gparams(w=w, h=h))
        acc.add(spp)
        torch.cuda.synchronize()
        res[on] = (acc.film.cpu().numpy().astype(np.float64), acc.variance.cpu().numpy().astype(np.float64))
    (m0, v0), (m1, v1) = res[False], res[True]
    both0 = (v0 == 0) & (v1 == 0)
    np.testing.assert_array_equal(m1[both0], m0[both0])
    z = np.abs(m1 - m0) / np.sqrt(np.where(both0, 1.0, v0 + v1))
    zi = abs(m1.mean() - m0.mean()) / np.sqrt((v0.sum() + v1.sum()) / m0.size ** 2)
    print(f"same expectation: worst pixel z {z[~both0].max():.2f}, image z {zi:.2f}, means {m0.mean():.5f} {m1.mean():.5f}, "
          f"{int(both0.sum())} values with both variances 0")
    assert m0.mean() > 0.01
    assert z[~both0].max() <= 5.0
    assert zi <= 5.0


def test_light_sampling_lowers_the_variance():
    """64 spp: the image mean of the variance plane with the switch on against off
    (off: the parent's estimator, bit for bit — test_empty_tables_are_inert).
    Measured once on an MI355X: off 0.00858874, on 0.00192238, ratio 4.47
    (MEASURED_VARIANCE_RATIO, DESIGN.md §14, profiles/nee/variance_ratio.txt); half
    of it is asserted, the off estimate being firefly-dominated at 64 spp."""
    v = {}
    for on in (False, True):
        acc = make_scene(nee=on).accumulator(gparams())
        acc.add(64)
        torch.cuda.synchronize()
        v[on] = float(acc.variance.cpu().numpy().astype(np.float64).mean())
    ratio = v[False] / v[True]
    print(f"variance off {v[False]:.6g} on {v[True]:.6g} ratio {ratio:.2f}")
    assert v[True] < v[False]
    assert MEASURED_VARIANCE_RATIO is not None, "the ratio has not been measured"
    assert ratio >= MEASURED_VARIANCE_RATIO / 2


# ---- 9. the command-line host

def test_cli_nee_equals_the_python_api(tmp_path):
    """spt_render_cli applies no materials of its own: the emitters reach it through a
    scene cache, whose extra bytes carry the pbrt camera."""
    w, h, d, spp = 40, 24, 4, 4
    s = sptamd.Scene()
    s.add_triangle_mesh(scenes.scene_pbrt("cornell_spheres", DETAIL))
    s.commit(0)
    kd, ke = scenes.smallpt_materials(s.mesh)
    s.backend.set_albedo(kd)
    s.backend.set_emission(ke)
    path = str(tmp_path / "cornell.sptc")
    s.save(path)

    def cli(out, *flags):
        r = subprocess.run([CLI, "-w", str(w), "-h", str(h), "-d", str(d), "-s", str(spp), "--rr", "2", path, "-o", out]
                           + list(flags), capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stdout + r.stderr
        return sptamd.read_pfm(out).transpose(2, 0, 1)

    p = sptamd.make_params(w, h, spp, d, camera=s.pbrt_info["camera"], rr_start_depth=2)
    plain, _ = render(s, p)
    np.testing.assert_array_equal(cli(str(tmp_path / "off.pfm")), plain)
    s.backend.set_light_sampling(True)
    assert s.backend.light_sampling() == (True, 28)
    want, st = render(s, p)
    assert st["shadow_casts"] > 0 and not np.array_equal(want, plain)
    np.testing.assert_array_equal(cli(str(tmp_path / "on.pfm"), "--nee"), want)
    np.testing.assert_array_equal(cli(str(tmp_path / "acc.pfm"), "--nee", "-s", "2", "--passes", "2"), want)
