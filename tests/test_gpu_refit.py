"""In-place geometry updates (spt_scene_update_geometry): the triangle records
and normals rewritten in their slots, the BVH refitted on the GPU.  The
closest hit does not depend on the tree, so after an update
films, ray casts and first-hit buffers equal bit for bit those of the CPU
oracle on the new mesh and of a scene freshly built from it — for both
builders, every tree width and child-group packing."""
import functools

import numpy as np
import pytest
import torch

import aov_ref
import oracle as O
import sptamd
from sptamd import _lib, scenes

pytestmark = pytest.mark.gpu

W, H, SPP, D = 48, 40, 4, 6
KW = dict(rr_start_depth=3, env=(1.0, 0.9, 0.8))
HOST, GPU = _lib.SPT_BUILD_HOST_SAH, _lib.SPT_BUILD_GPU_PLOC
# (bvh_width, builder, pack_groups); the GPU builder makes wide trees only
CONFIGS = [(8, HOST, 0), (8, HOST, 1), (8, GPU, 2), (6, HOST, 2), (6, GPU, 1), (6, GPU, 0), (2, HOST, 1)]
NRAYS = 65536


@functools.lru_cache(maxsize=None)
def base_mesh():
    return scenes.with_planar_uv(scenes.mitsuba_synth(detail=0.25))


@functools.lru_cache(maxsize=None)
def albedo():
    rng = np.random.default_rng(11)
    return rng.uniform(0.3, 0.95, size=(len(base_mesh()["kd"]), 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def deformed_pos(phase):
    """The fixed smooth field, ~1 % of the vertices thrown up to 40 units away
    (node extents cross several quantisation exponents) and a handful of
    triangles collapsed to a point or to a segment.  phase None: as built."""
    m = base_mesh()
    pos = np.asarray(m["pos"], np.float32)
    if phase is None:
        return pos
    out = (pos + 0.25 * np.sin(3.0 * pos[:, [1, 2, 0]] + np.float32(phase))).astype(np.float32)
    rng = np.random.default_rng(100 + int(phase * 10))
    far = rng.choice(len(pos), max(1, len(pos) // 100), replace=False)
    out[far] += rng.uniform(-40.0, 40.0, size=(len(far), 3)).astype(np.float32)
    pt = np.asarray(m["pos_tri"], np.int64).reshape(-1, 3)
    for i, t in enumerate(rng.choice(len(pt), 6, replace=False)):
        out[pt[t, 1]] = out[pt[t, 0]]                 # a segment
        if i % 2 == 0:
            out[pt[t, 2]] = out[pt[t, 0]]             # a point
    return out


def mesh_at(phase, base=None):
    m = dict(base_mesh() if base is None else base)
    m["pos"] = deformed_pos(phase)
    return m


def params(pipeline=None):
    return sptamd.make_params(W, H, SPP, D, pipeline=pipeline, **KW)


@functools.lru_cache(maxsize=None)
def oracle_film(phase):
    return O.OracleScene(mesh_at(phase), albedo=albedo()).render(O.reference_params(W, H, SPP, D, **KW))


@functools.lru_cache(maxsize=None)
def rays():
    rng = np.random.default_rng(3)
    o = rng.uniform([-3.0, -0.5, -3.0], [3.0, 4.0, 3.0], size=(NRAYS, 3)).astype(np.float32).T
    d = rng.normal(size=(3, NRAYS)).astype(np.float32)
    return np.ascontiguousarray(o), d


@functools.lru_cache(maxsize=None)
def oracle_hits(phase):
    o, d = rays()
    return O.OracleScene(mesh_at(phase)).intersect(o, d)


def config(width, build, pack):
    cfg = sptamd.default_config()
    cfg.bvh_width, cfg.build, cfg.pack_groups = width, build, pack
    return cfg


def scene(cfg, mesh, with_albedo=True):
    s = sptamd.Scene(config=cfg)
    s.add_arrays(mesh)
    s.commit(0)
    if with_albedo:
        s.backend.set_albedo(albedo())
    assert s.backend.stats["bvh_width"] == cfg.bvh_width and s.backend.stats["builder"] == cfg.build
    return s


def film_of(s, pipeline=None):
    f, st = s.render(params(pipeline))
    torch.cuda.synchronize()
    return f.cpu().numpy(), st


def assert_film(s, phase, pipeline=None, msg=""):
    got, st = film_of(s, pipeline)
    ref, casts = oracle_film(phase)
    np.testing.assert_array_equal(got, ref, err_msg=f"{msg} {pipeline}")
    assert st["ray_casts"] == casts, (msg, pipeline)


def saved(s, path):
    s.save(str(path))
    return open(path, "rb").read()


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,build,pack", CONFIGS)
def test_deformed_equals_oracle_and_fresh_build(width, build, pack):
    cfg = config(width, build, pack)
    s = scene(cfg, mesh_at(None))
    before = s.backend.stats
    s.update_geometry(deformed_pos(0.7), base_mesh()["nrm"])
    for pipeline in ("fused", "wavefront"):
        assert_film(s, 0.7, pipeline)
    o, d = rays()
    tri, t, _, _ = s.backend.intersect_raw(sptamd.Ray3.make(o, d))
    torch.cuda.synchronize()
    rt, rtt, _, _ = oracle_hits(0.7)
    np.testing.assert_array_equal(tri.cpu().numpy(), rt)
    hit = rt >= 0
    assert 0.2 < hit.mean() < 1.0
    np.testing.assert_array_equal(t.cpu().numpy()[hit], rtt[hit])
    fresh = scene(cfg, mesh_at(0.7))
    got, ref = aov_ref.gpu_planes(s, params()), aov_ref.gpu_planes(fresh, params())
    assert set(got) == {"albedo", "normal", "depth", "coverage"}
    for k in ref:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert got["coverage"].max() > 0
    st = _lib.SceneStats()
    _lib.check(_lib.lib.spt_scene_get_stats(s.backend.handle, st), "spt_scene_get_stats")
    assert st.as_dict() == before                      # "as built"


# 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,build,pack", [(8, HOST, 1), (8, GPU, 1), (6, HOST, 1), (6, GPU, 2), (2, HOST, 1)])
def test_identity_update_reproduces_the_build(width, build, pack, tmp_path):
    """bvh_build.cpp stores the exact child unions in a BVH2 node, so width 2
    is held to the same byte identity as the wide trees."""
    m = mesh_at(None)
    s = scene(config(width, build, pack), m)
    a = saved(s, tmp_path / "a.sptc")
    s.update_geometry(m["pos"], m["nrm"])
    b = saved(s, tmp_path / "b.sptc")
    assert a == b
    rs = s.backend.refit_stats()
    print("identity", width, build, rs)
    assert rs["updates"] == 1 and rs["area_built"] > 0
    assert abs(rs["area_now"] - rs["area_built"]) <= 1e-6 * rs["area_built"]


# 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,build,pack", [(8, GPU, 1), (6, HOST, 1), (2, HOST, 1)])
def test_no_drift(width, build, pack, tmp_path):
    m = mesh_at(None)
    s = scene(config(width, build, pack), m)
    a = saved(s, tmp_path / "a.sptc")
    for phase in (0.7, 1.9, 3.1):
        s.update_geometry(deformed_pos(phase), m["nrm"])
    assert saved(s, tmp_path / "moved.sptc") != a
    s.update_geometry(m["pos"], m["nrm"])
    assert saved(s, tmp_path / "b.sptc") == a          # boxes shrink back, nothing accumulates
    rs = s.backend.refit_stats()
    assert rs["updates"] == 4
    assert abs(rs["area_now"] - rs["area_built"]) <= 1e-6 * rs["area_built"]


# 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("some", [False, True])
def test_missing_normals_use_the_new_geometric_normal(some):
    base = dict(base_mesh())
    if some:
        nt = np.array(base["nrm_tri"], np.int32, copy=True).reshape(-1, 3)
        nt[::3, 1] = -1
        nt[1::7] = -1
        base["nrm_tri"] = nt
    else:
        base.pop("nrm_tri")
        base.pop("nrm")
    cfg = config(6, HOST, 1)
    s = scene(cfg, mesh_at(None, base))
    s.update_geometry(deformed_pos(1.9), base.get("nrm"))
    fresh = scene(cfg, mesh_at(1.9, base))
    got, ref = aov_ref.gpu_planes(s, params()), aov_ref.gpu_planes(fresh, params())
    for k in ref:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    built = aov_ref.gpu_planes(scene(cfg, mesh_at(None, base)), params())
    assert not np.array_equal(built["normal"], ref["normal"])
    ofilm, casts = O.OracleScene(mesh_at(1.9, base), albedo=albedo()).render(O.reference_params(W, H, SPP, D, **KW))
    got_film, st = film_of(s)
    np.testing.assert_array_equal(got_film, ofilm)
    np.testing.assert_array_equal(film_of(fresh)[0], ofilm)
    assert st["ray_casts"] == casts


# 5 ------------------------------------------------------------------------------------------
def test_queued_work_sees_its_own_geometry():
    m = mesh_at(None)
    s = scene(config(6, HOST, 1), m)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    phases, tickets, films = [], [], []

    def queue(phase):
        f = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
        _, t = s.render_async(params(), film=f, stream=streams[len(tickets) % 2])
        phases.append(phase)
        tickets.append(t)
        films.append(f)

    queue(None)
    queue(None)
    s.update_geometry(deformed_pos(0.7), m["nrm"])     # renders 0 and 1 may still be running
    queue(0.7)
    s.update_geometry(deformed_pos(1.9), m["nrm"])
    queue(1.9)
    stats = [s.render_wait(t) for t in tickets]
    torch.cuda.synchronize()
    for i, (phase, f, st) in enumerate(zip(phases, films, stats)):
        ref, casts = oracle_film(phase)
        np.testing.assert_array_equal(f.cpu().numpy(), ref, err_msg=f"render {i}")
        assert st["ray_casts"] == casts, i
    assert len({films[i].cpu().numpy().tobytes() for i in (0, 2, 3)}) == 3


# 6 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,build,pack", [(6, GPU, 2), (2, HOST, 1)])
def test_cache_loaded_scene(width, build, pack, tmp_path):
    m = mesh_at(None)
    src = scene(config(width, build, pack), m)
    src.save(str(tmp_path / "a.sptc"))
    s = sptamd.Scene.load(str(tmp_path / "a.sptc"))
    assert s.mesh is None
    with pytest.raises(ValueError):
        s.update_geometry(deformed_pos(0.7))
    s.update_geometry(deformed_pos(0.7), m["nrm"], pos_tri=m["pos_tri"], nrm_tri=m["nrm_tri"])
    assert_film(s, 0.7, msg="loaded")
    s.save(str(tmp_path / "b.sptc"))
    again = sptamd.Scene.load(str(tmp_path / "b.sptc"))
    assert_film(again, 0.7, msg="saved after the update")
    again.update_geometry(deformed_pos(1.9), m["nrm"], pos_tri=m["pos_tri"], nrm_tri=m["nrm_tri"])
    assert_film(again, 1.9, msg="updated again")


# 7 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,build,pack", [(6, HOST, 1), (8, GPU, 1), (2, HOST, 1)])
def test_device_arrays(width, build, pack):
    m = mesh_at(None)
    s = scene(config(width, build, pack), m)
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()  # noqa: E731
    pt, nt = up(m["pos_tri"], np.int32), up(m["nrm_tri"], np.int32)
    pos, nrm = up(deformed_pos(0.7), np.float32), up(m["nrm"], np.float32)
    torch.cuda.synchronize()
    s.update_geometry(pos, nrm, pos_tri=pt, nrm_tri=nt, stream=side)
    f = torch.empty((3, H, W), dtype=torch.float32, device="cuda")
    _, ticket = s.render_async(params(), film=f, stream=other)   # queued right after, on another stream
    st = s.render_wait(ticket)
    torch.cuda.synchronize()
    ref, casts = oracle_film(0.7)
    np.testing.assert_array_equal(f.cpu().numpy(), ref)
    assert st["ray_casts"] == casts
    host = scene(config(width, build, pack), m)
    host.update_geometry(deformed_pos(0.7), m["nrm"])
    np.testing.assert_array_equal(film_of(host)[0], ref)
    with pytest.raises(TypeError):
        s.backend.update_geometry(m["pos_tri"], pos)              # a host array beside device positions


# 8 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
def test_errors_leave_the_scene_alone(device, tmp_path):
    m = mesh_at(None)
    s = scene(config(6, HOST, 1), m)
    s.update_geometry(deformed_pos(0.7), m["nrm"])
    a = saved(s, tmp_path / "a.sptc")
    updates = s.backend.refit_stats()["updates"]
    pt = np.array(m["pos_tri"], np.int32, copy=True).reshape(-1, 3)
    nt = np.array(m["nrm_tri"], np.int32, copy=True).reshape(-1, 3)
    pos, nrm = deformed_pos(1.9), np.asarray(m["nrm"], np.float32)
    bad_pos, bad_nrm = pt.copy(), nt.copy()
    bad_pos[len(pt) // 2, 1] = len(pos)                # == nvert
    bad_nrm[7, 2] = -2                                 # below -1
    conv = (lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device \
        else (lambda a: a)
    cases = {"ntri": (pt[:-1], pos, nt[:-1], nrm), "position index": (bad_pos, pos, nt, nrm),
             "normal index": (pt, pos, bad_nrm, nrm)}
    for name, (a_pt, a_pos, a_nt, a_nrm) in cases.items():
        with pytest.raises(sptamd.SptError) as e:
            s.backend.update_geometry(conv(a_pt), conv(a_pos), conv(a_nt), conv(a_nrm))
        assert e.value.code == _lib.SPT_ERR_INVALID, name
    # NULL positions, through the C ABI
    h = s.backend.handle
    ptd = conv(pt)
    ptr = ptd.data_ptr() if device else ptd.ctypes.data
    rc = (_lib.lib.spt_scene_update_geometry_device(h, ptr, None, len(pos), len(pt), None, None, 0, None) if device
          else _lib.lib.spt_scene_update_geometry(h, ptr, None, len(pos), len(pt), None, None, 0))
    assert rc == _lib.SPT_ERR_INVALID and b"NULL positions" in _lib.lib.spt_last_error()
    assert s.backend.refit_stats()["updates"] == updates
    assert saved(s, tmp_path / "b.sptc") == a          # exactly as it was
    assert_film(s, 0.7, msg="after the refused updates")


# 9 ------------------------------------------------------------------------------------------
def test_other_setters_are_unaffected():
    m = mesh_at(None)
    nm = len(m["kd"])
    emi = np.zeros((nm, 3), np.float32)
    emi[4] = (2.0, 1.5, 1.0)
    tex = scenes.checker(8, 8, cell=1)
    sph = np.array([[0.0, 0.6, 0.0, 0.35], [0.7, 0.3, 0.4, 0.2]], np.float32)
    sph_mat = np.array([2, 3], np.int32)
    kinds = np.zeros(nm, np.uint32)
    kinds[3] = 1                                       # mirror
    s = scene(config(6, HOST, 1), m)
    be = s.backend
    be.set_emission(emi)
    be.set_texture(1, tex)
    be.set_spheres(sph, sph_mat)
    be.set_material_kinds(kinds)
    s.update_geometry(deformed_pos(3.1), m["nrm"])
    osc = O.OracleScene(mesh_at(3.1), albedo=albedo(), emission=emi, textures={1: tex}, spheres=sph,
                        sphere_mat=sph_mat, kinds=kinds)
    ref, casts = osc.render(O.reference_params(W, H, SPP, D, **KW))
    got, st = film_of(s)
    np.testing.assert_array_equal(got, ref)
    assert st["ray_casts"] == casts
    assert not np.array_equal(ref, oracle_film(3.1)[0])


# 10 -----------------------------------------------------------------------------------------
def tiny_meshes():
    rng = np.random.default_rng(21)
    one = (np.array([[-1.0, 0.2, -1.0], [1.5, 0.4, -0.5], [0.0, 1.8, 0.5]], np.float32), np.arange(3).reshape(1, 3))
    p9 = rng.uniform(-1.5, 1.5, size=(27, 3)).astype(np.float32) + np.float32([0, 1.0, 0])
    nine = (p9, np.arange(27).reshape(9, 3))
    grid = np.stack(np.meshgrid(np.linspace(-2, 2, 5), np.linspace(-2, 2, 5)), -1).reshape(-1, 2)
    plane = np.concatenate([grid[:, :1], np.full((25, 1), 0.25), grid[:, 1:]], 1).astype(np.float32)
    quads = [(r * 5 + c, r * 5 + c + 1, r * 5 + c + 6, r * 5 + c + 5) for r in range(4) for c in range(4)]
    ptri = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])
    return {"one": one, "nine": nine, "plane": (plane, ptri),
            "none": (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))}


@pytest.mark.parametrize("width", [8, 6, 2])
@pytest.mark.parametrize("name", ["one", "nine", "plane", "none", "point"])
def test_smallest_trees(width, name):
    pos, tri = tiny_meshes()["nine" if name == "point" else name]
    tri = np.ascontiguousarray(tri, np.int32)
    rng = np.random.default_rng(5)
    if name == "point":
        new = np.tile(np.float32([0.3, 0.9, -0.2]), (len(pos), 1))        # every vertex at one point
    elif name == "plane":
        new = pos.copy()
        new[:, [0, 2]] += rng.uniform(-0.3, 0.3, size=(len(pos), 2)).astype(np.float32)
        new[:, 1] = np.float32(0.5)                                       # still one plane: zero extent in y
    else:
        new = (pos + rng.uniform(-0.8, 0.8, size=pos.shape)).astype(np.float32)
    s = scene(config(width, HOST, 1), {"pos": pos, "pos_tri": tri}, with_albedo=False)
    s.backend.set_albedo(np.float32([[0.7, 0.6, 0.5]]))
    s.update_geometry(new)
    new_mesh = {"pos": new, "pos_tri": tri}
    assert s.mesh["pos"] is not pos and np.array_equal(s.mesh["pos"], new)
    osc = O.OracleScene(new_mesh, albedo=np.float32([[0.7, 0.6, 0.5]]))
    ref, casts = osc.render(O.reference_params(W, H, SPP, D, **KW))
    got, st = film_of(s)
    np.testing.assert_array_equal(got, ref)
    assert st["ray_casts"] == casts
    o, d = rays()
    o, d = np.ascontiguousarray(o[:, :4096]), np.ascontiguousarray(d[:, :4096])
    d[1] = -np.abs(d[1])
    o[1] += 3.0
    out = s.backend.intersect_raw(sptamd.Ray3.make(o, d))
    torch.cuda.synchronize()
    rt, rtt, _, _ = osc.intersect(o, d)
    np.testing.assert_array_equal(out[0].cpu().numpy(), rt)
    np.testing.assert_array_equal(out[1].cpu().numpy()[rt >= 0], rtt[rt >= 0])
    rs = s.backend.refit_stats()
    if name == "none":
        sky = np.broadcast_to(np.float32(KW["env"])[:, None, None], ref.shape)
        np.testing.assert_array_equal(ref, sky)
        assert rs["updates"] == 0 and rs["plan_bytes"] == 0
    else:
        assert rs["nodes"] == s.backend.stats["nodes"] and rs["tris"] == len(tri)
        if name in ("one", "nine", "plane"):
            assert (rt >= 0).any()


NF_RAYS = 4096


@functools.lru_cache(maxsize=None)
def non_finite_pos():
    """deformed_pos(0.7) with one triangle all NaN, one +inf and one -inf coordinate."""
    pos = np.array(deformed_pos(0.7), copy=True)
    pt = np.asarray(base_mesh()["pos_tri"], np.int64).reshape(-1, 3)
    broken = pt[[5, 600, 6000]]
    pos[broken[0]] = np.nan
    pos[broken[1, 0], 0] = np.inf
    pos[broken[2, 1], 2] = -np.inf
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def non_finite_oracle_hits():
    """The brute-force oracle (no tree) over the first NF_RAYS rays on the mesh
    of non_finite_pos() without its broken triangles: (ids in the full mesh's
    numbering, t, the broken triangles)."""
    m = mesh_at(None)
    pos = non_finite_pos()
    pt = np.asarray(m["pos_tri"], np.int64).reshape(-1, 3)
    nt = np.asarray(m["nrm_tri"], np.int64).reshape(-1, 3)
    bad = ~np.isfinite(pos[pt]).all(axis=(1, 2))
    keep = np.flatnonzero(~bad)
    used = np.zeros(len(pos), bool)
    used[pt[keep]] = True                                # vertices only the broken triangles use may be non-finite
    clean = dict(m, pos=np.where(used[:, None], pos, np.float32(0.0)), pos_tri=pt[keep].astype(np.int32),
                 nrm_tri=nt[keep].astype(np.int32), mat_id=np.asarray(m["mat_id"])[keep])
    clean.pop("tc_tri", None)
    clean.pop("tc", None)
    o, d = rays()
    rt, rtt, _, _ = O.OracleScene(clean, use_bvh=False).intersect(o[:, :NF_RAYS], d[:, :NF_RAYS])
    return np.where(rt >= 0, keep[np.maximum(rt, 0)], -1).astype(np.int32), rtt, np.flatnonzero(bad)


def assert_non_finite_hits(s):
    """Every finite triangle is still reachable: ids and t over the first
    NF_RAYS rays equal the brute-force oracle's on the mesh without the broken
    triangles."""
    o, d = rays()
    o, d = np.ascontiguousarray(o[:, :NF_RAYS]), np.ascontiguousarray(d[:, :NF_RAYS])
    tri, t, _, _ = s.backend.intersect_raw(sptamd.Ray3.make(o, d))
    torch.cuda.synchronize()
    rt, rtt, _ = non_finite_oracle_hits()
    hit = rt >= 0
    assert hit.mean() >= 0.2, hit.mean()                 # a fair share of the rays hits (else: other rays)
    np.testing.assert_array_equal(tri.cpu().numpy(), rt)
    np.testing.assert_array_equal(t.cpu().numpy()[hit], rtt[hit])


def test_non_finite_positions_do_not_fault():
    """Infinite and NaN coordinates are taken as the builders take them (the
    widest quantisation step; such triangles are never hit)."""
    m = mesh_at(None)
    s = scene(config(6, HOST, 1), m)
    pos = np.array(deformed_pos(0.7), copy=True)
    pt = np.asarray(m["pos_tri"], np.int64).reshape(-1, 3)
    broken = pt[[5, 600, 6000]]
    pos[broken[0]] = np.nan
    pos[broken[1, 0], 0] = np.inf
    pos[broken[2, 1], 2] = -np.inf
    assert np.array_equal(pos, non_finite_pos(), equal_nan=True)
    s.update_geometry(pos, m["nrm"])
    got, st = film_of(s)
    assert np.isfinite(got).all() and st["film_slots_unwritten"] == 0
    o, d = rays()
    tri = s.backend.intersect_raw(sptamd.Ray3.make(o, d))[0].cpu().numpy()
    bad_tris = np.flatnonzero(~np.isfinite(pos[pt]).all(axis=(1, 2)))
    assert len(bad_tris) >= 3 and not np.isin(tri, bad_tris).any()
    assert np.array_equal(bad_tris, non_finite_oracle_hits()[2])
    assert_non_finite_hits(s)                              # and every finite triangle is still reachable
    s.update_geometry(deformed_pos(0.7), m["nrm"])         # and the tree recovers
    assert_film(s, 0.7, msg="after the non-finite update")


# 11 -----------------------------------------------------------------------------------------
def test_stats():
    m = mesh_at(None)
    s = scene(config(6, GPU, 1), m)
    be = s.backend
    zero = be.refit_stats()
    assert all(v == 0 for v in zero.values()), zero
    before = dict(be.stats)
    s.update_geometry(deformed_pos(0.7), m["nrm"])
    rs = be.refit_stats()
    print("stats", rs)
    assert rs["updates"] == 1
    assert rs["nodes"] == before["nodes"] and rs["tris"] == before["ntri"] == len(m["pos_tri"])
    assert 1 <= rs["levels"] <= before["max_depth"]
    assert rs["plan_bytes"] > 0 and rs["plan_ms"] > 0 and rs["update_ms"] > 0 and rs["refit_ms"] > 0
    assert rs["update_ms"] >= rs["refit_ms"]
    assert rs["area_now"] > rs["area_built"] > 0          # the scattered vertices
    s.update_geometry(deformed_pos(1.9), m["nrm"])
    rs2 = be.refit_stats()
    assert rs2["updates"] == 2 and rs2["plan_ms"] == rs["plan_ms"] and rs2["area_built"] == rs["area_built"]
    st = _lib.SceneStats()
    _lib.check(_lib.lib.spt_scene_get_stats(be.handle, st), "spt_scene_get_stats")
    assert st.as_dict() == before
