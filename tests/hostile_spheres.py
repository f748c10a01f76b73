"""Hostile analytic spheres (spt_scene_set_spheres) for the trace tests: 256
overlapping spheres, smallpt-style wall spheres of radius 1e2 to 1e4, small
spheres seen from a hundred radii away, spheres wholly outside the triangle
mesh's bounds, spheres and no triangles, exact float32 ties, and the rays cast
at them.  Pure numpy, seeded; no GPU.  tests/test_hostile_spheres_ref.py
checks the reference on them against float64, tests/test_gpu_hostile_spheres.py
the kernels.

sphere_records restates sphere_t (csrc/spt_internal.h, oracle/oracle.c) in
numpy float32, one rounded operation at a time; sphere_f64 is the float64
reference of one (ray, sphere) pair, free of the cancellation of b b - a c;
error_model is the unit the float32 discriminant and roots are measured in;
decidable() says which pairs float32 can be asked about at all.

BEYOND holds the families outside the validity range of the float32 roots
(walls of radius 1e5, r / distance of 1e-3 and 3e-4, rays leaving the surface
of a sphere of radius 1e3): nothing about them is asserted against float64,
they are measured."""
import functools
import zlib

import numpy as np

import hostile

F = np.float32
EPS = 2.0 ** -24
G = 8.0                       # the guard of decidable(): a condition, not a tolerance
FAMILIES = ("unit256", "walls_1e2", "walls_1e3", "walls_1e4", "small_far", "outside", "alone", "tie")
BEYOND = ("walls_1e5", "small_far_1e-3", "small_far_3e-4", "surface_1e3")
RAY_SETS = ("aimed", "interval", "inside", "surface", "grazing", "degenerate")
# what the float64 legs run on: alone has unit256's spheres, tie is exact by construction
F64_FAMILIES = ("unit256", "walls_1e2", "walls_1e3", "walls_1e4", "small_far", "outside")
F64_SETS = ("aimed", "interval", "inside", "surface", "grazing")
SURFACE_RMAX = 30.0           # in the envelope, surface rays start on spheres of r <= 30
# materials of every family: 0 the triangles, 1-4 diffuse colours, 5 mirror, 6 glass, 7 an emitter
ALBEDO = np.array([[0.7, 0.6, 0.5], [0.75, 0.25, 0.25], [0.25, 0.75, 0.25], [0.25, 0.25, 0.75], [0.8, 0.8, 0.3],
                   [0.95, 0.95, 0.95], [0.99, 0.99, 0.99], [0.1, 0.1, 0.1]], F)
EMISSION = np.array([[0, 0, 0]] * 7 + [[6.0, 5.0, 3.0]], F)
KINDS = np.array([0, 0, 0, 0, 0, 1, 2, 0], np.uint32)
EMITTER = 7


def _mesh(tv, spheres, emitter=0, mats=None):
    m = dict(hostile.soup(np.asarray(tv, np.float64).reshape(-1, 9)))
    m["mat_id"] = np.zeros(len(m["pos_tri"]), np.int32)
    sph = np.ascontiguousarray(spheres, F).reshape(-1, 4)
    assert 0 < len(sph) <= 256 and np.isfinite(sph).all() and (sph[:, 3] > 0).all()
    sm = (1 + np.arange(len(sph)) % 6).astype(np.int32) if mats is None else np.asarray(mats, np.int32).copy()
    sm[emitter] = EMITTER
    m["spheres"], m["sphere_mat"], m["kinds"] = sph, sm, KINDS.copy()
    for k in ("mat_id", "spheres", "sphere_mat", "kinds"):
        m[k].setflags(write=False)
    return m


def without_spheres(mesh):
    return {k: v for k, v in mesh.items() if k not in ("spheres", "sphere_mat", "kinds")}


def _unit_ball(rng, n):
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u


def unit256(triangles=True, seed=201):
    """256 spheres, centres uniform in [-1, 1]^3, r in [0.05, 0.5]: they overlap
    heavily.  Spheres 17 and 200 are bit-identical copies of 5 and 90 (the lower
    index must win), 40-43 a concentric nest.  With 40 triangles through the
    cloud, or none."""
    rng = np.random.default_rng(seed)
    sph = np.concatenate([rng.uniform(-1, 1, size=(256, 3)), rng.uniform(0.05, 0.5, size=(256, 1))], 1).astype(F)
    sph[17], sph[200] = sph[5], sph[90]
    for j, r in enumerate((0.45, 0.3, 0.2, 0.1)):
        sph[40 + j] = (0.3, -0.2, 0.1, r)
    tv = np.zeros((0, 9))
    if triangles:
        c = rng.uniform(-1, 1, size=(40, 1, 3))
        tv = (c + rng.normal(size=(40, 3, 3)) * 0.5).reshape(40, 9)
    return _mesh(tv, sph, emitter=3)


IDENTICAL = ((5, 17), (90, 200))


def walls(R, seed=202):
    """Six spheres of radius R round the cube [0, 1]^3 as smallpt places its
    walls, four spheres of r 0.1 to 0.2 inside, and two triangles across the room."""
    R = float(R)
    sph = [(-R, .5, .5, R), (1 + R, .5, .5, R), (.5, -R, .5, R), (.5, 1 + R, .5, R), (.5, .5, -R, R), (.5, .5, 1 + R, R),
           (0.27, 0.165, 0.47, 0.165), (0.73, 0.2, 0.3, 0.2), (0.4, 0.7, 0.6, 0.12), (0.7, 0.6, 0.75, 0.1)]
    tv = [[0.1, 0.45, 0.1, 0.6, 0.45, 0.15, 0.15, 0.5, 0.7], [0.9, 0.9, 0.1, 0.9, 0.3, 0.5, 0.55, 0.95, 0.6]]
    return _mesh(tv, sph, emitter=8, mats=[1, 3, 4, 4, 2, 4, 5, 6, 7, 2])


def small_far(ratios=(1e-1, 1e-2), n=200, seed=203):
    """n spheres at distance 100 from the origin with r / distance from
    `ratios` in turn, seen from about the origin; one small triangle fan there."""
    rng = np.random.default_rng(seed)
    c = _unit_ball(rng, n) * 100.0
    r = 100.0 * np.asarray(ratios)[np.arange(n) % len(ratios)]
    tv = rng.normal(size=(6, 9)) * 0.5
    return _mesh(tv, np.concatenate([c, r[:, None]], 1), emitter=1)


def outside_mesh():
    """A 4 x 4 grid of quads in z = 0 over [-1, 1]^2 and two small pyramids to z = +-0.5."""
    xs = np.linspace(-1, 1, 5)
    tv = []
    for i in range(4):
        for j in range(4):
            a, b, c, d = (xs[i], xs[j], 0), (xs[i + 1], xs[j], 0), (xs[i + 1], xs[j + 1], 0), (xs[i], xs[j + 1], 0)
            tv += [a + b + c, a + c + d]
    for z in (0.5, -0.5):
        for a, b in (((-.25, -.25, 0), (.25, -.25, 0)), ((.25, -.25, 0), (.25, .25, 0)), ((.25, .25, 0), (-.25, .25, 0))):
            tv.append(a + b + (0.0, 0.0, z))
    return np.array(tv, np.float64)


OUTSIDE_HALF = np.array([1.0, 1.0, 0.5])


def outside(seed=204):
    """outside_mesh() with 24 spheres wholly outside its bounding box, four on
    each of the six sides, and sphere 24 enclosing the whole mesh (glass)."""
    rng = np.random.default_rng(seed)
    sph = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            for _ in range(4):
                r = rng.uniform(0.15, 0.6)
                c = rng.uniform(-0.8, 0.8, size=3)
                c[axis] = sign * (OUTSIDE_HALF[axis] + r + rng.uniform(0.05, 1.5))
                sph.append((*c, r))
    sph.append((0.05, -0.03, 0.02, 1.8))
    sph = np.array(sph, F)
    lo = np.abs(sph[:24, :3].astype(np.float64)) - sph[:24, 3:4] - OUTSIDE_HALF
    assert (lo.max(axis=1) > 0).all()                         # each is beyond one face of the box, whole
    mats = (1 + np.arange(25) % 5).astype(np.int32)
    mats[24] = 6
    mats[3], mats[20] = 5, 5
    return _mesh(outside_mesh(), sph, emitter=9, mats=mats)


def tie():
    """Exact float32 ties.  The ray o = (0, 0, 5), d = (0, 0, -1) meets sphere 0
    (0, 0, 0; 1) and triangle 0 in z = 1 at t = 4 exactly: the triangle, tested
    first, is kept.  At x = 10 the same with the triangle in z = 1 - 2^-21, one
    float of t further (t = 4 + 2^-21): sphere 1 wins.  Spheres 2 and 3 at
    x = 20 coincide: the lower index wins."""
    z1 = 1.0 - 2.0 ** -21
    # (the second triangle's edge functions at the ray are 2, 2 and 4: its t = 4 + 2^-21 is exact)
    tv = [[-1, -1, 1, 2, -1, 1, -1, 2, 1], [8, 0, z1, 12, -2, z1, 10, 1, z1]]
    sph = [(0, 0, 0, 1), (10, 0, 0, 1), (20, 0, 0, 1), (20, 0, 0, 1), (30, 0.25, 0, 0.5)]
    return _mesh(tv, sph, emitter=4)


TIE_RAYS = (np.array([[0, 0, 5], [10, 0, 5], [20, 0, 5], [0, 0, 5], [10, 0, 5]], F),
            np.array([[0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, -2], [0, 0, -2]], F))
# (id, t) the reference must report for TIE_RAYS, closest hit
TIE_EXPECT = ((0, 4.0), (-3, 4.0), (-4, 4.0), (0, 2.0), (-3, 2.0))


@functools.lru_cache(maxsize=None)
def family(name):
    if name.startswith("walls_") or name.startswith("surface_"):   # surface_<R>: walls(R), the surface rays start on the walls
        return walls(float(name.split("_")[1]))
    if name.startswith("small_far_"):
        return small_far(ratios=(float(name[10:]),), seed=205)
    return {"unit256": unit256, "alone": lambda: unit256(triangles=False), "small_far": small_far,
            "outside": outside, "tie": tie}[name]()


def camera(name):
    """A camera that sees the family's spheres (and its mesh, where it has one)."""
    eye, at = {"unit256": ((0.3, 0.4, 4.0), (0.0, 0.0, 0.0)), "alone": ((0.3, 0.4, 4.0), (0.0, 0.0, 0.0)),
               "outside": ((3.5, 2.5, 6.0), (0.0, 0.0, 0.0)), "tie": ((10.0, 3.0, 30.0), (10.0, 0.0, 0.0))}.get(
                   name, ((0.5, 0.5, 0.95), (0.5, 0.4, 0.0)))
    return dict(look_from=eye, look_at=at, up=(0.0, 1.0, 0.0), lens_radius=0.0, focal_dist=1.0,
                fov_y=float(F(F(40.0) / F(180.0)) * F(np.pi)), film_size_y=0.035)


# ------------------------------------------------------------------------------------------ rays

def _origins(name, sph, k, rng):
    """Origins outside sphere k: inside the room for the walls, about the origin
    for the far spheres, 1.5 to 6 radii from the centre otherwise."""
    n = len(k)
    if name.startswith("walls") or name.startswith("surface_"):
        near = sph[k, :3] + _unit_ball(rng, n) * (sph[k, 3] * rng.uniform(1.5, 4.0, size=n))[:, None]
        room = rng.uniform(0.02, 0.98, size=(n, 3))
        return np.where((k < 6)[:, None], room, np.clip(near, 0.01, 0.99))
    if name.startswith("small_far"):
        return rng.uniform(-1.0, 1.0, size=(n, 3))
    return sph[k, :3] + _unit_ball(rng, n) * (sph[k, 3] * rng.uniform(1.5, 6.0, size=n))[:, None]


@functools.lru_cache(maxsize=None)
def rays(name, n_aimed=6000, n_inside=2500, n_surface=2500, n_grazing=2000, n_degenerate=996):
    """The rays of a family: {set: (o (3, n), d (3, n), tmin, tmax)} float32,
    read-only, about 20 000 in all, and {set: k} the sphere each ray is about."""
    sph = family(name)["spheres"].astype(np.float64)
    ns = len(sph)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    out, which = {}, {}
    # aimed: from outside, at a point within 1.3 r of a centre, |d| over exp(+-3)
    k = rng.integers(0, ns, size=n_aimed)
    o = _origins(name, sph, k, rng).astype(F)
    p = sph[k, :3] + _unit_ball(rng, n_aimed) * (1.3 * sph[k, 3] * rng.uniform(size=n_aimed) ** (1 / 3))[:, None]
    s = np.exp(rng.uniform(-3, 3, size=n_aimed))
    d = ((p - o) * s[:, None]).astype(F)
    if name == "tie":                                            # the exact ties lead the set
        o[:5], d[:5], k[:5], s[:5] = TIE_RAYS[0], TIE_RAYS[1], (0, 1, 2, 0, 1), (0.25, 0.25, 0.25, 0.5, 0.5)
    out["aimed"], which["aimed"] = (o, d, np.zeros(n_aimed, F), np.full(n_aimed, 1e20, F)), k
    # interval: the same rays; the target is at t = 1 / s, the roots about it
    tmin = rng.uniform(0.0, 1.2, size=n_aimed) / s
    tmax = tmin + rng.uniform(size=n_aimed) * (2.0 / s - tmin)
    out["interval"], which["interval"] = (o, d, tmin.astype(F), tmax.astype(F)), k
    # inside: origins inside a sphere, |d| over exp(+-6)
    k = rng.integers(0, ns, size=n_inside)
    io = sph[k, :3] + _unit_ball(rng, n_inside) * (0.95 * sph[k, 3] * rng.uniform(size=n_inside) ** (1 / 3))[:, None]
    idd = _unit_ball(rng, n_inside) * np.exp(rng.uniform(-6, 6, size=(n_inside, 1)))
    out["inside"], which["inside"] = (io.astype(F), idd.astype(F), np.zeros(n_inside, F), np.full(n_inside, 1e20, F)), k
    # surface: from a float32 point of a sphere's surface, any direction, |d| over exp(+-1), tmin = 1e-3
    ok = np.arange(6) if name.startswith("surface_") else np.flatnonzero(sph[:, 3] <= SURFACE_RMAX)
    if name == "walls_1e5" or name.startswith("small_far_"):
        ok = np.arange(ns)
    k = ok[rng.integers(0, len(ok), size=n_surface)]
    so = sph[k, :3] + _unit_ball(rng, n_surface) * sph[k, 3:4]
    if name.startswith("walls") or name.startswith("surface_"):  # the part of a wall that faces the room
        room = rng.uniform(0.0, 1.0, size=(n_surface, 3))
        u = room - sph[k, :3]
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        so = np.where((k < 6)[:, None], sph[k, :3] + u * sph[k, 3:4], so)
    sd = _unit_ball(rng, n_surface) * np.exp(rng.uniform(-1, 1, size=(n_surface, 1)))
    out["surface"] = (so.astype(F), sd.astype(F), np.full(n_surface, 1e-3, F), np.full(n_surface, 1e20, F))
    which["surface"] = k
    # grazing: impact parameter r (1 +- 10^U(-7, -2)), from 1 + 10^U(-3, -1.5) radii off the centre
    k = rng.integers(0, ns, size=n_grazing)
    u = _unit_ball(rng, n_grazing)
    w = np.cross(u, _unit_ball(rng, n_grazing))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    imp = sph[k, 3] * (1.0 + rng.choice([-1.0, 1.0], size=n_grazing) * 10.0 ** rng.uniform(-7, -2, size=n_grazing))
    dist = np.maximum(imp, sph[k, 3]) * (1.0 + 10.0 ** rng.uniform(-3, -1.5, size=n_grazing))
    sin = imp / dist
    cos = np.sqrt(1.0 - sin * sin)
    go = sph[k, :3] + u * dist[:, None]
    gd = (-u * cos[:, None] + w * sin[:, None]) * (sph[k, 3] * np.exp(rng.uniform(-1, 1, size=n_grazing)))[:, None]
    out["grazing"] = (go.astype(F), gd.astype(F), np.zeros(n_grazing, F), np.full(n_grazing, 1e20, F))
    which["grazing"] = k
    # degenerate directions (hostile.rays)
    zo, zd = out["aimed"][0][:n_degenerate].copy(), out["aimed"][1][:n_degenerate].copy()
    zd[0::6, 0] = 0.0
    zd[1::6, 1] = -0.0
    zd[2::6, 2] = 1e-30
    zd[3::6, :] = 0.0
    zd[4::6, 0] = 0.0
    zd[4::6, 2] = 0.0
    zd[5::6, 0] = np.nan
    out["degenerate"] = (zo, zd, np.zeros(len(zo), F), np.full(len(zo), 1e20, F))
    which["degenerate"] = which["aimed"][:n_degenerate]
    res = {}
    for st, (ro, rd, t0, t1) in out.items():
        arrs = (np.ascontiguousarray(ro.T, F), np.ascontiguousarray(rd.T, F), np.ascontiguousarray(t0, F),
                np.ascontiguousarray(t1, F))
        for a in arrs:
            a.setflags(write=False)
        res[st] = arrs
    for a in which.values():
        a.setflags(write=False)
    return res, which


@functools.lru_cache(maxsize=None)
def all_rays(name):
    """Every set of a family as one batch (o, d, tmin, tmax) and {set: slice}."""
    sets, _ = rays(name)
    cat = tuple(np.ascontiguousarray(np.concatenate([sets[s][i] for s in RAY_SETS], axis=-1)) for i in range(4))
    for a in cat:
        a.setflags(write=False)
    spans, at = {}, 0
    for s in RAY_SETS:
        n = sets[s][0].shape[1]
        spans[s] = slice(at, at + n)
        at += n
    return cat, spans


# ------------------------------------------------------------------------------------------ float32

def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _sphere_t(sp, o, d, tmin, tmax):
    """sphere_t of rays (3, n) against spheres sp (n, 4), float32 throughout: (t, root)."""
    with np.errstate(all="ignore"):
        op = (sp[:, 0] - o[0], sp[:, 1] - o[1], sp[:, 2] - o[2])
        a = _dot(d, d)
        b = _dot(op, d)
        c = _dot(op, op) - sp[:, 3] * sp[:, 3]
        det = b * b - a * c
        ok = det >= 0
        sq = np.sqrt(det)
        t0, t1 = (b - sq) / a, (b + sq) / a
        in0 = ok & (t0 >= tmin) & (t0 <= tmax)
        in1 = ok & ~in0 & (t1 >= tmin) & (t1 <= tmax)
    assert all(x.dtype == F for x in (a, b, c, det, sq, t0, t1))
    t = np.where(in0, t0, np.where(in1, t1, F(np.inf))).astype(F)
    return t, np.where(in0, 0, np.where(in1, 1, -1))


def _f32_rays(o, d, tmin, tmax):
    o, d = np.asarray(o, F).reshape(3, -1), np.asarray(d, F).reshape(3, -1)
    return o, d, np.asarray(tmin, F), np.asarray(tmax, F)


def sphere_records(spheres, o, d, tmin, tmax, k):
    """sphere_t (csrc/spt_internal.h, oracle/oracle.c) of ray i against sphere
    k[i] alone, restated in numpy float32 one rounded operation at a time:
    (t, root), t = +inf and root = -1 for a miss, root 0 the nearer root."""
    o, d, tmin, tmax = _f32_rays(o, d, tmin, tmax)
    return _sphere_t(np.asarray(spheres, F).reshape(-1, 4)[np.asarray(k)], o, d, tmin, tmax)


def trace_spheres(spheres, o, d, tmin, tmax, held=None, anyhit=False):
    """The kernels' loop over all spheres after the triangles: `held` is the
    triangle pass's (id, t, u, v) (None: no triangles); a sphere strictly nearer
    than what is held wins, a tie keeps what is held, id = -2 - k; any-hit takes
    the first sphere hit, and only where no triangle was hit.  (id, t, u, v),
    t / u / v of a miss 0 as oracle_intersect leaves them."""
    o, d, tmin, tmax = _f32_rays(o, d, tmin, tmax)
    n = o.shape[1]
    sph = np.asarray(spheres, F).reshape(-1, 4)
    if held is None:
        held = (np.full(n, -1, np.int32), np.zeros(n, F), np.zeros(n, F), np.zeros(n, F))
    hid, t, u, v = (np.array(x, copy=True) for x in held)
    ht = np.where(hid != -1, t, tmax).astype(F)
    live = hid == -1 if anyhit else np.ones(n, bool)
    for k in range(len(sph)):
        ts, _ = _sphere_t(np.broadcast_to(sph[k], (n, 4)), o, d, tmin, ht)
        win = live & (ts < ht)
        ht = np.where(win, ts, ht)
        hid = np.where(win, -2 - k, hid).astype(np.int32)
        u, v = np.where(win, F(0), u), np.where(win, F(0), v)
        if anyhit:
            live = live & ~win
    t = np.where(hid != -1, ht, t).astype(F)
    return hid, t, u.astype(F), v.astype(F)


# ------------------------------------------------------------------------------------------ float64

def sphere_f64(spheres, o, d, tmin, tmax, k):
    """The float64 reference of ray i against sphere k[i]: a dict of dlen (|d|), det (the
    discriminant b b - a c as a (r^2 - |op - (b / a) d|^2), no cancellation),
    lo / hi (the roots from q = b + sign(b) sqrt(det) as q / a and c / q, NaN
    without real roots), t and root (the root sphere_t's rule takes in [tmin,
    tmax]: inf / -1 for a miss), and the terms of error_model."""
    D = np.float64
    sp = np.asarray(spheres, F).reshape(-1, 4)[np.asarray(k)].astype(D)
    o, d = np.asarray(o, F).reshape(3, -1).astype(D).T, np.asarray(d, F).reshape(3, -1).astype(D).T
    tmin, tmax = np.asarray(tmin, F).astype(D), np.asarray(tmax, F).astype(D)
    r = sp[:, 3]
    op = sp[:, :3] - o
    with np.errstate(all="ignore"):
        a, b, op2 = (d * d).sum(1), (op * d).sum(1), (op * op).sum(1)
        perp = op - (b / a)[:, None] * d
        det = a * (r * r - (perp * perp).sum(1))
        sq = np.sqrt(np.maximum(det, 0.0))
        q = b + np.where(b < 0, -1.0, 1.0) * sq
        lop = np.sqrt(op2)
        c = (lop - r) * (lop + r)
        r0, r1 = q / a, np.where(q != 0, c / q, q / a)
        real = det >= 0
        lo, hi = np.where(real, np.minimum(r0, r1), np.nan), np.where(real, np.maximum(r0, r1), np.nan)
        in0 = real & (lo >= tmin) & (lo <= tmax)
        in1 = real & ~in0 & (hi >= tmin) & (hi <= tmax)
    return dict(a=a, b=b, op2=op2, dlen=np.sqrt(a), r=r, det=det, lo=lo, hi=hi, tmin=tmin, tmax=tmax,
                t=np.where(in0, lo, np.where(in1, hi, np.inf)), root=np.where(in0, 0, np.where(in1, 1, -1)))


def error_model(ref):
    """(E_det, E_t) of sphere_f64's dict: with eps = 2^-24 and scale = b^2 +
    a (|op|^2 + r^2), E_det = eps scale and E_t = eps ((|b| + sq) / a + scale /
    (2 sq a)), sq = sqrt(|det|) and no smaller than sqrt(E_det): the float32
    discriminant is only known to E_det, so its root is not known better than
    that (this floor acts on undecidable pairs only)."""
    with np.errstate(all="ignore"):
        scale = ref["b"] ** 2 + ref["a"] * (ref["op2"] + ref["r"] ** 2)
        e_det = EPS * scale
        sq = np.sqrt(np.maximum(np.abs(ref["det"]), e_det))
        e_t = EPS * ((np.abs(ref["b"]) + sq) / ref["a"] + scale / (2.0 * sq * ref["a"]))
    return e_det, e_t


def decidable(ref, guard=G):
    """|det| > G E_det and, with real roots, both more than G E_t from tmin and from tmax."""
    e_det, e_t = error_model(ref)
    with np.errstate(all="ignore"):
        ok = np.isfinite(ref["det"]) & (np.abs(ref["det"]) > guard * e_det)
        far = np.ones(len(ok), bool)
        for root in (ref["lo"], ref["hi"]):
            for end in (ref["tmin"], ref["tmax"]):
                far &= np.abs(root - end) > guard * e_t
    return ok & ((ref["det"] < 0) | far)
