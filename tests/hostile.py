"""Hostile geometry for the traversal tests: triangle soups whose trees are
deep, span dozens of binades, sit far from the origin or are made of
coincident triangles, and the rays cast through them.  Pure numpy, seeded; no
GPU.  tests/test_hostile_ref.py checks the reference on them,
tests/test_gpu_hostile.py the kernels, tests/test_sanitize_inputs.py and
tests/native/soup_build.cpp the host builders.

Every family is a soup of at most about 3000 triangles whose coordinates are
at most 2^30 in magnitude, so that no float32 product of the ray-triangle
test overflows."""
import functools

import numpy as np

FAMILIES = ("mixed_scale", "corner_chain", "far_small", "coincident", "slivers", "flat_axes", "nonfinite")
RAY_SETS = ("aimed", "interval", "surface", "through", "degenerate")
CHAIN_N = 120


def soup(tv):
    """(n, 9) vertex triples -> a mesh dict (every triangle with its own three vertices)."""
    tv = np.ascontiguousarray(tv, np.float32).reshape(-1, 9)
    pos = tv.reshape(-1, 3).copy()
    pos.setflags(write=False)
    tri = np.arange(len(pos), dtype=np.int32).reshape(-1, 3)
    tri.setflags(write=False)
    return {"pos": pos, "pos_tri": tri}


def tri_soup(mesh):
    """The (n, 9) float32 soup of a mesh dict (spt_bvh_build_stats' input)."""
    pos, pt = np.asarray(mesh["pos"], np.float32), np.asarray(mesh["pos_tri"], np.int64).reshape(-1, 3)
    return np.ascontiguousarray(pos[pt].reshape(-1, 9))


def mixed_scale(n=3000, seed=101, span=12.0):
    """Each triangle a normal(0, 1) blob times exp(uniform(-span, span)): sizes
    and distances from the origin over twenty binades in one tree."""
    rng = np.random.default_rng(seed)
    return soup(rng.normal(size=(n, 9)) * np.exp(rng.uniform(-span, span, size=(n, 1))))


def corner_chain(n=CHAIN_N):
    """n right triangles in the plane z = 0 sharing the corner at the origin,
    legs 2^((k - n/2) / 2): every box holds all the smaller ones."""
    leg = np.exp2((np.arange(n) - n / 2) / 2.0)
    tv = np.zeros((n, 9))
    tv[:, 3] = leg
    tv[:, 7] = leg
    return soup(tv)


def far_small(n=3000, seed=103):
    """Unit-sized triangles centred at normal * 1e5: quantisation frames far from the origin."""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(n, 1, 3)) * 1e5
    return soup((c + rng.normal(size=(n, 3, 3)) * 0.5).reshape(n, 9))


def coincident(seed=104):
    """600 copies of one triangle and 200 copies each in three planes slightly
    off it, ids shuffled: full leaves, equal Morton codes, the tie rule."""
    rng = np.random.default_rng(seed)
    base = np.array([[-1.0, 0.1, -0.8], [1.2, 0.3, -0.5], [0.1, 0.2, 1.1]])
    nrm = np.cross(base[1] - base[0], base[2] - base[0])
    nrm /= np.linalg.norm(nrm)
    stacks = [base] * 600
    for k in (1, 2, 3):
        stacks += [base + nrm * (k * 2.0 ** -10)] * 200
    tv = np.stack(stacks)[rng.permutation(1200)]
    return soup(tv.reshape(-1, 9))


def stack_ids(mesh):
    """coincident(): for every triangle the smallest id among its exact copies."""
    tv = tri_soup(mesh)
    _, inv = np.unique(tv, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    first = np.full(inv.max() + 1, len(tv), np.int64)
    np.minimum.at(first, inv, np.arange(len(tv)))
    return first[inv]


def slivers(n=3000, seed=105):
    """Needles of aspect ratio 1e5 in random directions through one region:
    large overlapping boxes, so the traversal stack stays full."""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(n, 3)) * 0.5
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = np.cross(d, rng.normal(size=(n, 3)))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    length = rng.uniform(1.0, 10.0, size=(n, 1))
    return soup(np.concatenate([c - d * length / 2, c + d * length / 2, c + e * length * 1e-5], 1))


def flat_axes(q=22):
    """Three mutually orthogonal axis-aligned grids of triangles through the
    origin: nodes of zero extent (the e = -100 exponent byte)."""
    xs = np.linspace(-1.0, 1.0, q + 1)
    a, b = (g.ravel() for g in np.meshgrid(xs[:-1], xs[:-1], indexing="ij"))
    h = xs[1] - xs[0]
    z = np.zeros_like(a)
    quads = [np.stack([a, b], 1), np.stack([a + h, b], 1), np.stack([a + h, b + h], 1), np.stack([a, b + h], 1)]
    tris2 = np.concatenate([np.stack([quads[0], quads[1], quads[2]], 1), np.stack([quads[0], quads[2], quads[3]], 1)])
    out = []
    for axis in range(3):
        v = np.insert(tris2, axis, z[0], axis=2)        # (n, 3, 3) with a zero coordinate at `axis`
        out.append(v.reshape(-1, 9))
    return soup(np.concatenate(out))


def nonfinite(n=3000, seed=107):
    """mixed_scale over a narrower range with NaN, +inf and -inf put into about
    5 % of the triangles (one coordinate, one vertex, or the whole triangle)."""
    rng = np.random.default_rng(seed)
    tv = np.array(tri_soup(mixed_scale(n, seed, span=4.0)), np.float32)
    bad = rng.choice(n, n // 20, replace=False)
    for i, t in enumerate(bad):
        val = (np.nan, np.inf, -np.inf)[i % 3]
        kind = (i // 3) % 3
        if kind == 0:
            tv[t, rng.integers(0, 9)] = val
        elif kind == 1:
            k = 3 * rng.integers(0, 3)
            tv[t, k:k + 3] = val
        else:
            tv[t] = val
    return soup(tv)


@functools.lru_cache(maxsize=None)
def family(name):
    return {"mixed_scale": mixed_scale, "corner_chain": corner_chain, "far_small": far_small,
            "coincident": coincident, "slivers": slivers, "flat_axes": flat_axes, "nonfinite": nonfinite}[name]()


def finite_tris(mesh):
    return np.isfinite(tri_soup(mesh)).all(axis=1)


def tri_size(tv):
    """The longest edge per triangle, float64 (0 for a triangle without area)."""
    v = np.asarray(tv, np.float64).reshape(-1, 3, 3)
    edge = np.max([np.linalg.norm(v[:, a] - v[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))], axis=0)
    area = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    return np.where(area > 0, edge, 0.0)


# ------------------------------------------------------------------------------------------ rays

def _aimed(tv, size, rng, n):
    """n rays aimed at interior points (barycentrics >= 0.1) of random
    triangles from 0.5 to 4 triangle sizes away and at most 60 degrees off the
    normal (the float32 edge functions of a needle of aspect 1e5 seen at a
    grazing angle have no sign to speak of), the target at t = 1.  The float32
    ray is checked in float64: a ray whose point o + d has a barycentric
    below 0.05 in its triangle's plane is redrawn."""
    v = np.asarray(tv, np.float64).reshape(-1, 3, 3)
    ok = np.flatnonzero(size > 0)
    o_out, d_out, t_out = [], [], []
    need = n
    while need > 0:
        t = ok[rng.integers(0, len(ok), size=2 * need)]
        b = rng.dirichlet((1.0, 1.0, 1.0), size=len(t)) * 0.7 + 0.1
        p = (b[:, :, None] * v[t]).sum(1)
        u = rng.normal(size=(len(t), 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        nrm = np.cross(v[t, 1] - v[t, 0], v[t, 2] - v[t, 0])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        cos = (u * nrm).sum(1, keepdims=True)
        u = np.where(np.abs(cos) < 0.5, u + nrm * np.where(cos < 0, -1.0, 1.0), u)   # pulled towards the normal
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = (p + u * (size[t] * rng.uniform(0.5, 4.0, size=len(t)))[:, None]).astype(np.float32)
        d = (p - o).astype(np.float32)
        q = o.astype(np.float64) + d.astype(np.float64)
        e1, e2, r = v[t, 1] - v[t, 0], v[t, 2] - v[t, 0], q - v[t, 0]
        g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
        r1, r2 = (r * e1).sum(1), (r * e2).sum(1)
        det = g11 * g22 - g12 * g12
        with np.errstate(all="ignore"):
            bu, bv = (g22 * r1 - g12 * r2) / det, (g11 * r2 - g12 * r1) / det
        good = (det > 0) & (np.minimum(np.minimum(bu, bv), 1 - bu - bv) >= 0.05) & (np.abs(d).max(1) > 0)
        take = np.flatnonzero(good)[:need]
        o_out.append(o[take]); d_out.append(d[take]); t_out.append(t[take])
        need -= len(take)
    return np.concatenate(o_out), np.concatenate(d_out), np.concatenate(t_out)


@functools.lru_cache(maxsize=None)
def rays(name, n_aimed=6000, n_surface=4000, n_through=3000, n_degenerate=996):
    """The rays of a family: {set: (o (3, n), d (3, n), tmin, tmax)} float32,
    read-only, about 20 000 in all, and the triangles the aimed rays aim at."""
    mesh = family(name)
    tv = tri_soup(mesh).astype(np.float64)
    fin = finite_tris(mesh)
    size = np.where(fin, np.nan_to_num(tri_size(np.where(fin[:, None], tv, 0.0))), 0.0)
    rng = np.random.default_rng(1000 + FAMILIES.index(name))
    f32 = np.float32
    out = {}
    o, d, target = _aimed(tv, size, rng, n_aimed)
    n = len(o)
    out["aimed"] = (o.T, d.T, np.zeros(n, f32), np.full(n, 1e20, f32))
    tmin = rng.uniform(0.0, 1.2, size=n).astype(f32)
    tmax = (tmin + rng.uniform(0.0, 1.0, size=n) * (2.0 - tmin)).astype(f32)
    out["interval"] = (o.T, d.T, tmin, tmax)
    # surface rays, as bounces leave: from a point of a triangle, in any direction
    ok = np.flatnonzero(size > 0)
    t = ok[rng.integers(0, len(ok), size=n_surface)]
    b = rng.dirichlet((1.0, 1.0, 1.0), size=n_surface)
    v = tv.reshape(-1, 3, 3)
    so = (b[:, :, None] * v[t]).sum(1).astype(f32)
    sd = (rng.normal(size=(n_surface, 3)) * size[t][:, None]).astype(f32)
    out["surface"] = (so.T, sd.T, np.full(n_surface, 1e-3, f32), np.full(n_surface, 1e20, f32))
    # through rays: from 1e3 scene diameters outside, at a point of a triangle or of the bounds
    pts = v[fin].reshape(-1, 3)
    lo, hi = pts.min(0), pts.max(0)
    diam = np.linalg.norm(hi - lo)
    u = rng.normal(size=(n_through, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    to = (0.5 * (lo + hi) + u * 1e3 * diam).astype(f32)
    tt = ok[rng.integers(0, len(ok), size=n_through)]
    aim = (rng.dirichlet((1.0, 1.0, 1.0), size=n_through)[:, :, None] * v[tt]).sum(1)
    box = rng.uniform(lo, hi, size=(n_through, 3))
    aim = np.where((np.arange(n_through) % 4 == 3)[:, None], box, aim)
    td = (aim - to).astype(f32)
    out["through"] = (to.T, td.T, np.zeros(n_through, f32), np.full(n_through, 1e20, f32))
    # degenerate directions (test_gpu_isect.py::test_axis_aligned_and_degenerate_rays)
    go, gd = o[:n_degenerate].copy(), d[:n_degenerate].copy()
    gd[0::6, 0] = 0.0
    gd[1::6, 1] = -0.0
    gd[2::6, 2] = 1e-30
    gd[3::6, :] = 0.0
    gd[4::6, 0] = 0.0
    gd[4::6, 2] = 0.0
    gd[5::6, 0] = np.nan
    out["degenerate"] = (go.T, gd.T, np.zeros(len(go), f32), np.full(len(go), 1e20, f32))
    res = {}
    for k, arrs in out.items():
        arrs = tuple(np.ascontiguousarray(a, f32) for a in arrs)
        for a in arrs:
            a.setflags(write=False)
        res[k] = arrs
    target.setflags(write=False)
    return res, target


def all_rays(name):
    """Every set of a family as one batch (o, d, tmin, tmax) and {set: slice}."""
    sets, _ = rays(name)
    cat = tuple(np.ascontiguousarray(np.concatenate([sets[s][i] for s in RAY_SETS], axis=-1)) for i in range(4))
    spans, at = {}, 0
    for s in RAY_SETS:
        n = sets[s][0].shape[1]
        spans[s] = slice(at, at + n)
        at += n
    return cat, spans


def residual(mesh, o, d, tri, t, u, v):
    """|o + t d - (w p0 + u p1 + v p2)| in float64 over the triangle's longest
    edge, for the records with tri >= 0 (NaN elsewhere)."""
    tv = tri_soup(mesh).astype(np.float64).reshape(-1, 3, 3)
    o, d = np.asarray(o, np.float64).reshape(3, -1).T, np.asarray(d, np.float64).reshape(3, -1).T
    hit = np.asarray(tri) >= 0
    ids = np.where(hit, tri, 0)
    p = tv[ids]
    t, u, v = (np.asarray(x, np.float64) for x in (t, u, v))
    q = (1.0 - u - v)[:, None] * p[:, 0] + u[:, None] * p[:, 1] + v[:, None] * p[:, 2]
    edge = np.max([np.linalg.norm(p[:, a] - p[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))], axis=0)
    with np.errstate(all="ignore"):
        r = np.linalg.norm(o + t[:, None] * d - q, axis=1) / edge
    return np.where(hit, r, np.nan)


def camera(name):
    """A camera inside the bounds looking at the densest region: from the
    median vertex towards the mean of the vertices nearest to it."""
    mesh = family(name)
    tris = tri_soup(mesh).astype(np.float64).reshape(-1, 3, 3)[finite_tris(mesh)]
    pts = tris.reshape(-1, 3)
    eye = at = None
    if name == "corner_chain":
        # above the shared corner, at the middle of the chain's scales: half the chain fills the view
        eye, at = np.array([0.3, 0.3, 1.0]), np.array([0.2, 0.2, 0.0])
    elif name == "far_small":
        # the cloud is all but empty: a size off the triangle nearest the median centroid
        c = tris.mean(1)
        t = tris[np.argmin(np.linalg.norm(c - np.median(c, axis=0), axis=1))]
        n = np.cross(t[1] - t[0], t[2] - t[0])
        at = t.mean(0)
        eye = at + n / np.linalg.norm(n) * 1.2 + np.array([0.2, 0.1, 0.0])
    if eye is not None:
        return dict(look_from=tuple(float(x) for x in eye), look_at=tuple(float(x) for x in at), up=(0.0, 1.0, 0.0),
                    lens_radius=0.0, focal_dist=1.0,
                    fov_y=float(np.float32(np.float32(40.0) / np.float32(180.0)) * np.float32(np.pi)),
                    film_size_y=0.035)
    med = np.median(pts, axis=0)
    dist = np.linalg.norm(pts - med, axis=1)
    near = pts[np.argsort(dist)[: max(8, len(pts) // 4)]]
    scale = max(np.median(dist), 1e-6)
    eye = med + np.array([0.3, 0.5, 1.0]) * scale
    at = near.mean(0)
    if np.linalg.norm(at - eye) < 1e-3 * scale:
        at = eye - np.array([0.0, 0.0, scale])
    return dict(look_from=tuple(float(x) for x in eye), look_at=tuple(float(x) for x in at), up=(0.0, 1.0, 0.0),
                lens_radius=0.0, focal_dist=1.0,
                fov_y=float(np.float32(np.float32(40.0) / np.float32(180.0)) * np.float32(np.pi)), film_size_y=0.035)


def woop_records(mesh, o, d, tri):
    """The watertight ray-triangle test (Woop et al. 2013, as oracle.c
    woop_test_r and spt_math.h woop_core state it) of ray i against triangle
    tri[i] alone, restated in numpy float32 operation by operation: (inside,
    t, u, v).  Any record a tracer reports for that pair has to be this one
    bit for bit, whichever triangle an any-hit query stopped at."""
    f32, f64 = np.float32, np.float64
    o, d = np.asarray(o, f32).reshape(3, -1).T, np.asarray(d, f32).reshape(3, -1).T
    n = len(o)
    tv = tri_soup(mesh).reshape(-1, 3, 3)[np.where(np.asarray(tri) >= 0, tri, 0)]
    a = np.abs(d)
    kz = np.where(a[:, 0] > a[:, 1], np.where(a[:, 0] > a[:, 2], 0, 2), np.where(a[:, 1] > a[:, 2], 1, 2))
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    i = np.arange(n)
    swap = d[i, kz] < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(all="ignore"):
        sz = f32(1.0) / d[i, kz]
        sx, sy = d[i, kx] * sz, d[i, ky] * sz
        A, B, C = (tv[:, k] - o for k in range(3))
        ax, ay = A[i, kx] - sx * A[i, kz], A[i, ky] - sy * A[i, kz]
        bx, by = B[i, kx] - sx * B[i, kz], B[i, ky] - sy * B[i, kz]
        cx, cy = C[i, kx] - sx * C[i, kz], C[i, ky] - sy * C[i, kz]
        U, V, W = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
        z = (U == 0) | (V == 0) | (W == 0)
        dU = (cx.astype(f64) * by.astype(f64) - cy.astype(f64) * bx.astype(f64)).astype(f32)
        dV = (ax.astype(f64) * cy.astype(f64) - ay.astype(f64) * cx.astype(f64)).astype(f32)
        dW = (bx.astype(f64) * ay.astype(f64) - by.astype(f64) * ax.astype(f64)).astype(f32)
        U, V, W = np.where(z, dU, U), np.where(z, dV, V), np.where(z, dW, W)
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        az, bz, cz = sz * A[i, kz], sz * B[i, kz], sz * C[i, kz]
        T = (U * az + V * bz) + W * cz
        t, u, v = T / det + f32(0.0), V / det + f32(0.0), W / det + f32(0.0)
    inside = ~mixed & (det != 0) & np.isfinite(t)
    return inside, t.astype(f32), u.astype(f32), v.astype(f32)
