"""The restatements of light sampling, sky sampling and MIS (tests/nee_ref.py, sky_ref.py,
mis_ref.py) on glass, mirror spheres, textures and triangles without vertex normals, checked
without a GPU: with every switch off each of them is the oracle's own radiance bit for bit,
with MIS off the three agree, the scenes of tests/specular_scenes.py hold enough of every
event for tests/test_gpu_specular_sampling.py to mean something, smallpt's REFR rule in
float32 is the float64 one, and the substitute shading normal is the oracle's."""
import numpy as np
import pytest

import accum_ref as A
import mis_ref as M
import nee_ref as R
import oracle as O
import sky_ref as S
import specular_scenes as SS

F = np.float32
# test_scatter_weight_against_float64: measured, see there
MEASURED_WEIGHT_ERROR = 4.23e-5
MEASURED_UNITY_ERROR = 1.2e-7


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("name", ["specular", "textured", "no_normals", "some_normals"])
def test_off_equals_the_oracle(name):
    """Every switch off: the three restatements' per-sample radiance is accum_ref.contributions'
    (oracle_trace_sample's own L3) bit for bit — the glass weight after the roulette, the
    texture lookup and the substitute normals restated as the oracle has them."""
    m, kd, ke, tex = SS.variant(name)
    p = SS.oparams("spec_both_off")               # a tinted sky: escapes count
    sky = SS.sky_of("spec_both_off")
    ref = A.contributions(O.OracleScene(m, albedo=kd, emission=ke, textures=tex), SS.oparams("spec_off"))
    assert ref.mean() > 0.05
    np.testing.assert_array_equal(bits(R.contributions(m, SS.oparams("spec_off"), kd, ke, on=False, textures=tex)), bits(ref))
    np.testing.assert_array_equal(bits(M.contributions(m, SS.oparams("spec_off"), kd, ke, textures=tex)), bits(ref))
    np.testing.assert_array_equal(bits(S.contributions(m, SS.oparams("spec_off"), kd, ke, sky, on=False, textures=tex)), bits(ref))
    if name == "specular":
        # under the sky image the oracle has no lookup of its own: the three against each other
        a = R.contributions(m, p, kd, ke, sky=sky, on=False, textures=tex)
        np.testing.assert_array_equal(bits(S.contributions(m, p, kd, ke, sky, on=False, textures=tex)), bits(a))
        np.testing.assert_array_equal(bits(M.contributions(m, p, kd, ke, sky=sky, textures=tex)), bits(a))
        np.testing.assert_array_equal(bits(a), bits(SS.expected("spec_both_off")[1]))
    if tex is not None:                           # the images matter
        plain = A.contributions(O.OracleScene(m, albedo=kd, emission=ke), SS.oparams("spec_off"))
        assert not np.array_equal(plain, ref)


def test_the_three_agree_without_mis():
    m, kd, ke, _ = SS.variant("specular")
    a, b = {}, {}
    x = M.contributions(m, SS.oparams("spec_lights"), kd, ke, nee=True, count=a)
    np.testing.assert_array_equal(bits(x), bits(R.contributions(m, SS.oparams("spec_lights"), kd, ke, count=b)))
    assert a["shadow_casts"] == b["shadow_casts"] > 0 and all(a[k] == b[k] for k in R.EVENTS)
    np.testing.assert_array_equal(bits(x), bits(SS.expected("spec_lights")[1]))
    sky = SS.sky_of("spec_sky")
    md, _, ked, _ = SS.variant("dark")
    for case, mesh, emi, nee in (("spec_sky", md, ked, False), ("spec_both", m, ke, True)):
        a, b = {}, {}
        p, share = SS.oparams(case), SS.CASES[case]["share"]
        x = M.contributions(mesh, p, kd, emi, sky=sky, nee=nee, sky_on=True, share=share, count=a)
        y = S.contributions(mesh, p, kd, emi, sky, nee=nee, share=share, count=b)
        np.testing.assert_array_equal(bits(x), bits(y), err_msg=case)
        assert a["shadow_casts"] == b["shadow_casts"] > 0 and all(a[k] == b[k] for k in R.EVENTS), case
    assert SS.CASES["spec_both"]["share"] == 0.25


def test_event_floors():
    """What the specular scene's 37 x 19 x 8 paths of depth 7 hold, from the restatement alone.
    Measured: 583 continuing glass vertices on triangles and 6118 on spheres, 136 on the mirror
    sphere, 36 total internal reflections, 1860 Fresnel reflections and 4805 transmissions, 1428
    hits on an emissive triangle straight after a mirror or glass vertex (they count in full),
    215 escapes straight after one; light sampling: 7586 shadow rays, 1024 of them stopped by a
    mirror or glass surface.  Sky sampling on the dark variant under the sun map: 4399 shadow
    rays, 303 stopped by a mirror or glass surface, 167 of those by one of the analytic spheres
    (the glass ball around the camera stands in the room's open front, where the sun is).
    smallpt_analytic with its quad: 314 glass and 162 mirror vertices on spheres, 142 of 11049
    shadow rays stopped by one."""
    n = SS.expected("spec_lights_mis")[2]
    assert n["glass_on_triangles"] >= 300 and n["glass_on_spheres"] >= 3000 and n["mirror_on_spheres"] >= 100, n
    assert n["tir"] >= 10 and n["fresnel_reflections"] >= 1000 and n["transmissions"] >= 1000, n
    assert n["glass_on_triangles"] + n["glass_on_spheres"] == n["tir"] + n["fresnel_reflections"] + n["transmissions"]
    assert n["emitter_hits_after_specular"] >= 500 and n["shadow_rays_stopped_by_specular"] >= 500, n
    assert n["weighted_hits"] >= 1000
    for case in ("spec_sky", "textured_sky_mis"):
        n = SS.expected(case)[2]
        assert n["escapes_after_specular"] >= 100 and n["sky_rays_stopped_by_specular_sphere"] >= 100, (case, n)
    n = SS.expected("spec_both_mis")[2]
    assert n["escapes_after_specular"] >= 100 and n["weighted_escapes"] >= 100 and n["weighted_hits"] >= 1000, n
    for case in ("no_normals", "some_normals", "textured_lights_mis", "moved"):
        n = SS.expected(case)[2]
        assert n["glass_on_triangles"] >= 300 and n["shadow_casts"] >= 3000 and n["weighted_hits"] >= 1000, (case, n)
    n = SS.expected("smallpt_lights_mis")[2]
    assert n["glass_on_spheres"] >= 100 and n["mirror_on_spheres"] >= 100 and n["shadow_rays_stopped_by_specular"] >= 100, n
    # the samplers and MIS change the image, and the moved ball and the images too
    films = {c: SS.expected(c)[0]["film"] for c in ("spec_off", "spec_lights", "spec_lights_mis", "moved", "textured_lights_mis")}
    names = list(films)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not np.array_equal(films[a], films[b]), (a, b)


def sweep(n=5000, seed=11):
    """2 n unit normals and incoming directions of lengths 0.2 .. 5, the angle of incidence in n
    steps from 0 to pi / 2, from outside (the first n) and from inside the glass."""
    rng = np.random.default_rng(seed)
    nn = rng.normal(size=(2 * n, 3))
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    t = rng.normal(size=(2 * n, 3))
    t -= nn * np.einsum("ij,ij->i", t, nn)[:, None]
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    th = np.concatenate([np.linspace(0, np.pi / 2, n)] * 2)
    side = np.concatenate([-np.ones(n), np.ones(n)])
    d = (np.cos(th) * side)[:, None] * nn + np.sin(th)[:, None] * t
    d *= rng.uniform(0.2, 5, size=(2 * n, 1))
    return R.normalize(nn.astype(F)), d.astype(F)


def test_scatter_weight_against_float64():
    """smallpt's REFR rule in float32, one rounded operation at a time, against the same formula
    in float64 from the same float32 normals and directions: the specular scene's 6701 glass
    vertices and a sweep of 10^4 incidences from normal to grazing on both sides (2676 of them
    totally reflected).  Where float64's n . d and cos2t are farther than 1e-6 from 0 the side
    and the total-internal-reflection decision agree.  The weights' error is taken relative to
    the float64 weight, and to 0.01 where that is smaller: Tr = 1 - Re is a difference of numbers
    near 1, so toward grazing incidence, where Tr -> 0, the transmitted weight keeps an absolute
    error of the order of Re's and no relative accuracy (float64 9.4e-9 against float32 0 at the
    sweep's last angle).  Measured worst: 4.23e-5 on the sweep, a transmitted weight (the
    reflected one: 4.7e-6, just inside the critical angle, where cos2t is a small difference),
    2.7e-5 on the scene's vertices; 4 x 4.23e-5 is asserted.
    P wr + (1 - P) wt = 1 in float32: measured 1.2e-7 (one ulp), 4 x that asserted."""
    m, kd, ke, _ = SS.variant("specular")
    c = {"vertices": []}
    R.contributions(m, SS.oparams("spec_off"), kd, ke, on=False, count=c)
    vn = np.concatenate([v[0][~v[3]] for v in c["vertices"]])
    vd = np.concatenate([v[1][~v[3]] for v in c["vertices"]])
    assert len(vn) == c["glass_on_triangles"] + c["glass_on_spheres"] >= 3300
    worst = unity = 0.0
    for name, (n, d) in dict(scene=(vn, vd), sweep=sweep()).items():
        a, b = R.scatter_terms(n, d), R.scatter_terms(n, d, np.float64)
        nd64 = np.einsum("ij,ij->i", n.astype(np.float64), d.astype(np.float64) / np.linalg.norm(d.astype(np.float64), axis=1)[:, None])
        far = (np.abs(nd64) > 1e-6) & (np.abs(b["cos2t"]) > 1e-6)
        assert far.sum() >= len(n) - 4
        np.testing.assert_array_equal(a["into"][far], b["into"][far], err_msg=name)
        np.testing.assert_array_equal(a["tir"][far], b["tir"][far], err_msg=name)
        assert name == "scene" or (b["tir"].sum() > 2000 and (~b["tir"] & ~b["into"]).sum() > 2000)
        ok = far & ~b["tir"]
        for k in ("wr", "wt"):
            err = np.abs(a[k][ok].astype(np.float64) - b[k][ok]) / np.maximum(np.abs(b[k][ok]), 0.01)
            print(f"scatter_weight {name} {k}: worst error {err.max():.3g} of {ok.sum()}")
            worst = max(worst, float(err.max()))
        one = ((a["P"] * a["wr"]).astype(F) + ((F(1) - a["P"]).astype(F) * a["wt"]).astype(F)).astype(F)
        unity = max(unity, float(np.abs(one[ok].astype(np.float64) - 1.0).max()))
        for v in (a["refl"], a["tdir"][ok]):                     # unit directions
            assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1).max() < 1e-6
    print(f"scatter_weight: worst error {worst:.3g}, P wr + (1 - P) wt - 1 {unity:.3g}")
    assert worst <= 4 * MEASURED_WEIGHT_ERROR
    assert unity <= 4 * MEASURED_UNITY_ERROR


def test_scatter_weight_chooses_by_the_bits():
    n, d = sweep(200, seed=5)
    s = R.scatter_terms(n, d)
    ev = {}
    w = R.scatter_weight(n, d, np.where((np.arange(len(n)) % 2 == 0)[:, None] | s["tir"][:, None], s["refl"], s["tdir"]), events=ev)
    want = np.where(s["tir"], F(1), np.where(np.arange(len(n)) % 2 == 0, s["wr"], s["wt"]))
    np.testing.assert_array_equal(w, want)
    assert ev["tir"] == s["tir"].sum() > 0 and ev["fresnel_reflections"] > 50 and ev["transmissions"] > 50
    np.testing.assert_array_equal(R.scatter_weight(n, d, s["refl"], mirror=np.ones(len(n), bool)), np.ones(len(n), F))
    off = s["refl"].copy()
    off[3, 0] = np.nextafter(off[3, 0], F(2))
    with pytest.raises(AssertionError):
        R.scatter_weight(n, d, off, mirror=np.ones(len(n), bool))


def tilted_quads():
    """Two mirror quads, tilted so that their normals have three components: one without
    vertex normals at all in the first mesh, index -1 on one triangle of it in the second."""
    pos = np.array([[-1, 0.1, -1], [1, 0.3, -1.2], [1.1, 0.9, 0.8], [-0.9, 0.7, 1.0]], F)
    pt = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    base = dict(pos=pos, pos_tri=pt, mat_id=np.zeros(2, np.int32), kinds=np.array([1], np.uint32))
    some = dict(base, nrm=np.array([[0.1, 1.0, 0.2]], F), nrm_tri=np.array([[0, 0, 0], [-1, -1, -1]], np.int32))
    return base, some


def test_shading_normals_fallback_is_the_oracles():
    """The oracle's stored normals, read through oracle_trace_sample: a mirror's outgoing ray is
    dn - n (2 n . dn) of n = normalize(stored normal), so the recorded second ray equals the one
    restated from shading_normals bit for bit on every hit, and no other normal's."""
    cam = dict(SS.CAM, look_from=(0.1, 3.0, 0.4), look_at=(0.0, 0.4, 0.0), up=(0.0, 0.0, -1.0))
    p = O.reference_params(16, 12, 2, 2, camera=cam, env=(1.0, 1.0, 1.0))
    for mesh in tilted_quads():
        nrm = R.shading_normals(mesh)
        tv = R.tri_soup(mesh).reshape(-1, 3, 3).astype(np.float64)
        g = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        want_geo = np.ones(2, bool) if "nrm_tri" not in mesh else np.array([False, True])
        for t in range(2):
            if want_geo[t]:
                assert np.abs(nrm[t] - g[t]).max() < 1e-6 and np.array_equal(nrm[t, 0], nrm[t, 1])
            else:
                np.testing.assert_array_equal(nrm[t], np.broadcast_to(mesh["nrm"][0], (3, 3)))
        rays, ids, tuv, cnt, _, _, _ = R.paths(O.OracleScene(mesh, albedo=np.ones((1, 3), F)), p)
        hit = (ids[:, 0] >= 0) & (cnt > 1)
        assert hit.sum() > 100 and set(np.unique(ids[hit, 0])) == {0, 1}
        n = R.normalize(R.interpolated_normals(nrm, ids[hit, 0].astype(np.int64), tuv[hit, 0, 1], tuv[hit, 0, 2]))
        s = R.scatter_terms(n, rays[hit, 0, 3:6])
        assert R.same_bits(s["refl"], rays[hit, 1, 3:6]).all()
        nudged = n.copy()
        nudged[:, 0] = np.nextafter(nudged[:, 0], F(2))
        assert not R.same_bits(R.scatter_terms(nudged, rays[hit, 0, 3:6])["refl"], rays[hit, 1, 3:6]).all()


def test_reflectance_restates_the_lookup():
    m, kd, _, tex = SS.variant("textured")
    rng = np.random.default_rng(2)
    n = 64
    ids = rng.integers(0, len(m["pos_tri"]), n)
    ids[:4] = (-2, -3, -1, -4)
    u = rng.uniform(0, 1, n).astype(F)
    v = (rng.uniform(0, 1, n) * (1 - u)).astype(F)
    mat = np.where(ids >= 0, m["mat_id"][np.clip(ids, 0, None)], 3)
    mat[4:8] = (99, -1, 1, 3)
    got = R.reflectance(m, tex, mat, ids, u, v, kd)
    tc = m["tc"][m["tc_tri"]]
    for k in range(n):
        if mat[k] in tex and ids[k] != -1:
            uv = np.zeros(2, F)
            if ids[k] >= 0:
                w = F(F(1) - u[k]) - v[k]
                uv = (w * tc[ids[k], 0] + u[k] * tc[ids[k], 1]) + v[k] * tc[ids[k], 2]
            want = O.texture_eval(tex[int(mat[k])], float(uv[0]), float(uv[1]))
        else:
            want = kd[mat[k] if 0 <= mat[k] < len(kd) else 0]
        np.testing.assert_array_equal(got[k], want, err_msg=str(k))
    np.testing.assert_array_equal(R.reflectance(m, None, mat, ids, u, v, kd), kd[np.where((mat >= 0) & (mat < len(kd)), mat, 0)])
    assert len({tuple(x) for x in got[mat == 3]}) > 4            # the image varies over the hits
