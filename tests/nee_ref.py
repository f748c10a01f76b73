"""numpy restatement of light sampling (include/spt.h
spt_scene_set_light_sampling), written from the definition, not from the
library: the light table in float64, everything a path does with it in
float32, one rounded operation at a time.

  table     members = triangles whose material emits, in triangle order
            area = |(v1 - v0) x (v2 - v0)| / 2, w = area max(Le)  (bad w -> 0)
            cdf_i = f32(sum_{j<=i} w_j / sum w), last = 1; pdfA_i = f32(w_i / (sum w area_i))
  uniforms  light_uniform(pixel, sample, cast, k), k = 0, 1, 2: a 32-bit hash, top 24 bits
  vertex    i = the smallest index with xi0 < cdf_i
            (b1, b2) = xi2 > xi1 ? (xi1 / 2, xi2 - xi1 / 2) : (xi1 - xi2 / 2, xi2 / 2)
            y = ((1 - b1) - b2) v0 + b1 v1 + b2 v2;  d = y - x;  rl = 1 / sqrt(d . d)
            interval [0.001 rl, 1 + 0.001 rl]  (0.001 rl > 1: nothing)
            M = (bx by bz) = Frame3 of the bounce sampler's normal n as it takes it (a
            triangle's interpolated normal, not normalised; nl on a sphere), det = bx . (by x bz),
            v = (d . by x bz, d . bz x bx, d . bx x by), cx = ((v_y det) |det|) / ((v . v)^2 ((rl rl) rl))
            — pi times the density of the direction of M l, l cosine-distributed about +y;
            (n . d) rl for an orthonormal frame.  cy = |ng . d| rl, g = (((cx cy) rl) rl) / (pi pdfA)
            cx > 0, cy > 0, g < inf, c = (T Le) g != 0: the shadow ray is traced;
            its closest hit in the interval is triangle ids_i: L = L + c
  emission  the hit after such a vertex adds no emission if it is a triangle

The paths themselves — rays, hits, (t, u, v) — come from the oracle
(oracle_trace_sample), the throughput is restated from the reflectance (the
albedo table, or the material's image through oracle.texture_eval), a Python
rr_uniform and, after the roulette, the scatter weight of a glass vertex
(scatter_weight: smallpt's REFR rule, the branch read off the next ray's
direction bits), and a shadow ray's closest hit is oracle_intersect's over the
same interval (tree-independent by DESIGN.md §2's rules).  The marks are set at
diffuse vertices only; a mirror or glass vertex samples nothing.  contributions()
returns the per-sample x_s for accum_ref.moments."""
import ctypes

import numpy as np

import oracle as O

F = np.float32
U = np.uint32
PI = F(3.14159265358979323846)
TMIN = F(0.001)


# ---- the table

def tri_soup(mesh):
    return np.asarray(mesh["pos"], F)[np.asarray(mesh["pos_tri"]).reshape(-1, 3)].reshape(-1, 9)


def light_table(tv, mat, emission):
    """ids (uint32), cdf, pdfA (float32), and per light the vertices (n, 9), the unit
    geometric normal (n, 3) and Le (n, 3), of (T, 9) float32 vertices, T material
    ids (None: 0) and (M, 3) emission (None: no emitters)."""
    tv = np.asarray(tv, F).reshape(-1, 9)
    none = (np.zeros(0, U), np.zeros(0, F), np.zeros(0, F), np.zeros((0, 9), F), np.zeros((0, 3), F), np.zeros((0, 3), F))
    if emission is None or len(tv) == 0:
        return none
    emi = np.asarray(emission, F).reshape(-1, 3)
    mat = np.zeros(len(tv), np.int64) if mat is None else np.asarray(mat, np.int64).reshape(-1)
    ok = (mat >= 0) & (mat < len(emi))
    member = ok & np.any(emi[np.where(ok, mat, 0)] != 0, axis=1)
    ids = np.nonzero(member)[0]
    if len(ids) == 0:
        return none
    v = tv[ids].astype(np.float64)
    le = emi[mat[ids]]
    with np.errstate(all="ignore"):
        cr = np.cross(v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3])
        ln = np.sqrt((cr * cr).sum(axis=1))
        area = 0.5 * ln
        w = area * np.max(le, axis=1).astype(np.float64)
        w = np.where(np.isfinite(w) & (w > 0), w, 0.0)
        run = np.cumsum(w)                       # sequential
        total = run[-1] if len(run) else 0.0
        if not (total > 0 and np.isfinite(total)):
            return none
        cdf = (run / total).astype(F)
        cdf[-1] = F(1)
        pdf = np.where(w > 0, w / (total * np.where(area > 0, area, 1.0)), 0.0).astype(F)
        good = np.isfinite(ln) & (ln > 0)
        ng = np.where(good[:, None], cr / np.where(good, ln, 1.0)[:, None], 0.0).astype(F)
    return ids.astype(U), cdf, pdf, tv[ids], ng, le.astype(F)


# ---- the side streams

def _hash(h, s1, m1, s2, m2, s3):
    h = h.astype(U)
    h ^= h >> U(s1)
    h = (h * U(m1)).astype(U)
    h ^= h >> U(s2)
    h = (h * U(m2)).astype(U)
    h ^= h >> U(s3)
    return ((h >> U(8)).astype(F) * F(1.0 / 16777216.0)).astype(F)


def light_uniform(pixel, sample, depth, k):
    pixel, sample, depth = (np.asarray(a, np.uint64).astype(U) for a in (pixel, sample, depth))
    with np.errstate(over="ignore"):
        h = (pixel * U(0x8DA6B343)) ^ ((sample + U(0x2545F491)).astype(U) * U(0xD8163841)) ^ \
            ((depth * U(3) + U(k) + U(1)).astype(U) * U(0xCB1AB31F))
        return _hash(h, 15, 0x2C1B3C6D, 12, 0x297A2D39, 15)


def rr_uniform(pixel, sample, depth):
    pixel, sample, depth = (np.asarray(a, np.uint64).astype(U) for a in (pixel, sample, depth))
    with np.errstate(over="ignore"):
        h = (pixel * U(0x9E3779B1)) ^ ((sample + U(0x7F4A7C15)).astype(U) * U(0x85EBCA77)) ^ \
            ((depth + U(1)).astype(U) * U(0xC2B2AE3D))
        return _hash(h, 16, 0x85EBCA6B, 13, 0xC2B2AE35, 16)


# ---- the vertex

def tri_map(xi1, xi2):
    """Heitz's square-to-triangle map: (b1, b2), float32."""
    xi1, xi2 = np.asarray(xi1, F), np.asarray(xi2, F)
    up = xi2 > xi1
    h1, h2 = (xi1 / F(2)).astype(F), (xi2 / F(2)).astype(F)
    b1 = np.where(up, h1, (xi1 - h2).astype(F)).astype(F)
    b2 = np.where(up, (xi2 - h1).astype(F), h2).astype(F)
    return b1, b2


def dot(a, b):
    return ((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F) + (a[..., 2] * b[..., 2]).astype(F)


def normalize(v):
    with np.errstate(all="ignore"):
        inv = (F(1) / np.sqrt(dot(v, v)).astype(F)).astype(F)
        return (v * inv[..., None]).astype(F)


def cross(a, b):
    return np.stack([((a[..., 1] * b[..., 2]).astype(F) - (a[..., 2] * b[..., 1]).astype(F)).astype(F),
                     ((a[..., 2] * b[..., 0]).astype(F) - (a[..., 0] * b[..., 2]).astype(F)).astype(F),
                     ((a[..., 0] * b[..., 1]).astype(F) - (a[..., 1] * b[..., 0]).astype(F)).astype(F)], axis=-1)


def frame(n):
    """Frame3 of the normal n as given (coordframe.h:17-30): bx, by, bz."""
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    sign = np.copysign(F(1), ny).astype(F)
    with np.errstate(all="ignore"):
        a = (F(-1) / (sign + ny).astype(F)).astype(F)
        b = ((nz * nx).astype(F) * a).astype(F)
        bx = np.stack([(sign + ((nx * nx).astype(F) * a).astype(F)).astype(F), -nx, b], axis=-1)
        bz = np.stack([(sign * b).astype(F), ((-sign) * nz).astype(F),
                       (F(1) + (((sign * nz).astype(F) * nz).astype(F) * a).astype(F)).astype(F)], axis=-1)
    return bx.astype(F), n.astype(F), bz.astype(F)


def light_sample(table, x, nh, T, xi0, xi1, xi2):
    """For vertices x (n, 3) with the bounce sampler's normals nh and throughputs T: (traced, d,
    tmin, tmax, c, id) — whether a shadow ray is traced, its direction and interval,
    the contribution it carries and the triangle its closest hit must be."""
    ids, cdf, pdf, tv, ng, le = table
    i = np.minimum(np.searchsorted(cdf, np.asarray(xi0, F), side="right"), len(cdf) - 1)
    assert np.all(np.asarray(xi0, F) < cdf[i]) and np.all((i == 0) | (np.asarray(xi0, F) >= cdf[np.maximum(i - 1, 0)]))
    b1, b2 = tri_map(xi1, xi2)
    b0 = ((F(1) - b1).astype(F) - b2).astype(F)
    v = tv[i]
    y = (((b0[:, None] * v[:, 0:3]).astype(F) + (b1[:, None] * v[:, 3:6]).astype(F)).astype(F)
         + (b2[:, None] * v[:, 6:9]).astype(F)).astype(F)
    d = (y - x).astype(F)
    with np.errstate(all="ignore"):
        rl = (F(1) / np.sqrt(dot(d, d)).astype(F)).astype(F)
        tmin = (TMIN * rl).astype(F)
        tmax = (F(1) + tmin).astype(F)
        bx, by, bz = frame(np.asarray(nh, F))
        c1, c2, c3 = cross(by, bz), cross(bz, bx), cross(bx, by)
        det = dot(bx, c1).astype(F)
        v = np.stack([dot(d, c1), dot(d, c2), dot(d, c3)], axis=-1).astype(F)
        vv = dot(v, v).astype(F)
        cx = (((v[..., 1] * det).astype(F) * np.abs(det)).astype(F)
              / ((vv * vv).astype(F) * ((rl * rl).astype(F) * rl).astype(F)).astype(F)).astype(F)
        cy = (np.abs(dot(ng[i], d)) * rl).astype(F)
        g = ((((cx * cy).astype(F) * rl).astype(F) * rl).astype(F) / (PI * pdf[i]).astype(F)).astype(F)
        ok = (tmin <= F(1)) & (cx > 0) & (cy > 0) & (g < np.inf)
        c = ((T * le[i]).astype(F) * g[:, None]).astype(F)
    c = np.where(ok[:, None], c, F(0)).astype(F)
    traced = ok & np.any(c != 0, axis=1)
    return traced, d, tmin, tmax, c, ids[i]


# ---- mirror and glass (include/spt.h SPT_MAT_MIRROR / SPT_MAT_GLASS: smallpt's SPEC and REFR)

def scatter_terms(n, d_in, dtype=F):
    """smallpt's REFR rule at unit normals n (m, 3) for incoming directions d_in, every
    operation rounded to dtype: refl, tdir, the total-internal-reflection flag tir, cos2t,
    Re, P and the two weights wr = Re / P, wt = Tr / (1 - P)."""
    X = dtype
    n, d = np.asarray(n, X), np.asarray(d_in, X)

    def dt(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    def unit(v):
        return v * (X(1) / np.sqrt(dt(v, v)))[..., None]

    with np.errstate(all="ignore"):
        dn = unit(d)
        ndd = dt(n, dn)
        refl = dn - n * (X(2) * ndd)[..., None]
        into = ndd < 0
        nl = np.where(into[..., None], n, -n)
        nnt = np.where(into, X(1) / X(1.5), X(1.5) / X(1))
        ddn = dt(dn, nl)
        cos2t = X(1) - (nnt * nnt) * (X(1) - ddn * ddn)
        tir = cos2t < 0
        ks = np.where(into, X(1), X(-1)) * (ddn * nnt + np.sqrt(np.where(tir, X(0), cos2t)))
        tdir = unit(dn * nnt[..., None] - n * ks[..., None])
        R0 = (X(0.5) * X(0.5)) / (X(2.5) * X(2.5))
        c = X(1) - np.where(into, -ddn, dt(tdir, n))
        Re = R0 + (X(1) - R0) * ((((c * c) * c) * c) * c)
        Tr = X(1) - Re
        P = X(0.25) + X(0.5) * Re
        wr, wt = Re / P, Tr / (X(1) - P)
    out = dict(refl=refl, tdir=tdir, tir=tir, into=into, cos2t=cos2t, Re=Re, P=P, wr=wr, wt=wt)
    assert all(v.dtype == (bool if k in ("tir", "into") else X) for k, v in out.items())
    return out


def same_bits(a, b):
    return np.all(np.ascontiguousarray(a, F).view(U) == np.ascontiguousarray(b, F).view(U), axis=-1)


def scatter_weight(n, d_in, d_out, mirror=None, events=None):
    """The weight (m,) float32 a mirror or glass vertex multiplies into the throughput: glass
    Re / P where the path left along refl, Tr / (1 - P) along tdir, 1 at a total internal
    reflection; mirror (mask `mirror`) 1.  d_out, the next ray's direction, is one of the
    restated directions bit for bit, or this asserts.  events: a dict whose counts of total
    internal reflections, Fresnel reflections and transmissions are raised."""
    s = scatter_terms(n, d_in)
    d_out = np.asarray(d_out, F)
    mirror = np.zeros(len(d_out), bool) if mirror is None else np.asarray(mirror, bool)
    is_r, is_t = same_bits(d_out, s["refl"]), same_bits(d_out, s["tdir"])
    only_r = mirror | s["tir"]
    assert np.all(is_r[only_r]), "a mirror or a total internal reflection leaves along refl"
    fres = ~only_r
    assert np.all(is_r[fres] ^ is_t[fres]), "a glass vertex leaves along exactly one of refl, tdir"
    w = np.where(only_r, F(1), np.where(is_r, s["wr"], s["wt"])).astype(F)
    if events is not None:
        events["tir"] = events.get("tir", 0) + int((s["tir"] & ~mirror).sum())
        events["fresnel_reflections"] = events.get("fresnel_reflections", 0) + int((fres & is_r).sum())
        events["transmissions"] = events.get("transmissions", 0) + int((fres & is_t).sum())
    return w


# ---- a render

# what contributions() counts beside shadow_casts (count=): continuing glass and mirror vertices
# by surface, the glass vertices' three outcomes, hits on an emissive triangle and escapes
# straight after a mirror or glass vertex (they count in full), and shadow rays whose closest
# hit is a mirror or glass surface (sky_ref: the sky's shadow rays stopped by such a sphere)
EVENTS = ("glass_on_triangles", "glass_on_spheres", "mirror_on_spheres", "tir", "fresnel_reflections", "transmissions",
          "emitter_hits_after_specular", "escapes_after_specular", "shadow_rays_stopped_by_specular",
          "sky_rays_stopped_by_specular_sphere")


def emits(emi, m):
    """The material m has a non-zero row in the emission table."""
    return (m >= 0) & (m < len(emi)) & np.any(emi[np.clip(m, 0, len(emi) - 1)] != 0, axis=-1)


def hit_kinds(hid, mat_id, sph_mat, kinds):
    """The material kind at each hit id (0 at a miss, and without a kinds table)."""
    hid = np.asarray(hid, np.int64)
    m = np.where(hid >= 0, mat_id[np.clip(hid, 0, max(len(mat_id) - 1, 0))] if len(mat_id) else 0, -1)
    if sph_mat is not None:
        m = np.where(hid < -1, sph_mat[np.clip(-2 - hid, 0, len(sph_mat) - 1)], m)
    if len(kinds) == 0:
        return np.zeros(len(hid), np.int64)
    return np.where((hid != -1) & (m >= 0) & (m < len(kinds)), kinds[np.clip(m, 0, len(kinds) - 1)], 0)


def shading_normals(mesh):
    """(T, 3, 3): the three vertex normals of every triangle, as the scene stores them — a
    vertex without one (index -1 or past the array, or a mesh without nrm_tri) takes
    normalize(cross(v1 - v0, v2 - v0)) in float32."""
    tv = tri_soup(mesh).reshape(-1, 3, 3)
    g = normalize(cross((tv[:, 1] - tv[:, 0]).astype(F), (tv[:, 2] - tv[:, 0]).astype(F)))
    out = np.repeat(g[:, None, :], 3, axis=1).astype(F)
    if mesh.get("nrm_tri") is None or mesh.get("nrm") is None:
        return out
    nt = np.asarray(mesh["nrm_tri"], np.int64).reshape(-1, 3)
    nrm = np.asarray(mesh["nrm"], F).reshape(-1, 3)
    ok = (nt >= 0) & (nt < len(nrm))
    return np.where(ok[..., None], nrm[np.clip(nt, 0, max(len(nrm) - 1, 0))], out).astype(F)


def texcoords(mesh):
    """(T, 3, 2) float32: the three texcoords of every triangle, (0, 0) where missing; None
    for a mesh without them."""
    if mesh.get("tc_tri") is None or mesh.get("tc") is None:
        return None
    tt = np.asarray(mesh["tc_tri"], np.int64).reshape(-1, 3)
    tc = np.asarray(mesh["tc"], F).reshape(-1, 2)
    ok = (tt >= 0) & (tt < len(tc))
    return np.where(ok[..., None], tc[np.clip(tt, 0, max(len(tc) - 1, 0))], F(0)).astype(F)


def reflectance(mesh, textures, m, id, u, v, albedo=None):
    """(n, 3) float32: what a bounce at hit `id` (>= 0 a triangle, < -1 a sphere) with
    barycentrics (u, v) and material m multiplies into the throughput — the material's
    image (textures: {material: (H, W, 3)}) at the texcoord (w c0 + u c1) + v c2, w = (1 - u) - v,
    (0, 0) on a sphere or a mesh without texcoords; else albedo[m], an m past the table taking
    row 0.  albedo: default mesh["albedo"]."""
    albedo = np.asarray(mesh["albedo"] if albedo is None else albedo, F).reshape(-1, 3)
    m, id = np.asarray(m, np.int64), np.asarray(id, np.int64)
    out = albedo[np.where((m >= 0) & (m < len(albedo)), m, 0)].astype(F)
    if not textures:
        return out
    tc = texcoords(mesh)
    u, v = np.asarray(u, F), np.asarray(v, F)
    w = ((F(1) - u).astype(F) - v).astype(F)
    for k in np.nonzero(np.isin(m, [int(t) for t in textures]) & (id != -1))[0]:
        tu = tv = F(0)
        if tc is not None and id[k] >= 0:
            c = tc[id[k]]
            tu = ((w[k] * c[0, 0]).astype(F) + (u[k] * c[1, 0]).astype(F)).astype(F) + (v[k] * c[2, 0]).astype(F)
            tv = ((w[k] * c[0, 1]).astype(F) + (u[k] * c[1, 1]).astype(F)).astype(F) + (v[k] * c[2, 1]).astype(F)
        out[k] = O.texture_eval(textures[int(m[k])], float(tu), float(tv))
    return out


def interpolated_normals(nrm, id, u, v):
    """(w n0 + u n1) + v n2 of the hit triangles, not normalised; row 0's where id is no triangle."""
    u, v = np.asarray(u, F), np.asarray(v, F)
    w = ((F(1) - u).astype(F) - v).astype(F)
    nv = nrm[np.clip(id, 0, len(nrm) - 1)] if len(nrm) else np.zeros((len(u), 3, 3), F)
    return (((w[:, None] * nv[:, 0]).astype(F) + (u[:, None] * nv[:, 1]).astype(F)).astype(F)
            + (v[:, None] * nv[:, 2]).astype(F)).astype(F)


def specular_weights(nrm, sph, kind, cont, id, tuv, d_in, x_next, d_next, events=None):
    """(N,) float32: scatter_weight of the continuing (`cont`) mirror and glass vertices of one
    cast, 1 elsewhere.  The unit normal is normalize(sn) on a triangle and normalize(hp - c),
    hp the next ray's origin, on a sphere.  events: counts by kind and surface are raised."""
    sw = np.ones(len(id), F)
    k = np.nonzero(cont & (kind != 0))[0]
    if events is not None:
        for name, sel in (("glass_on_triangles", (kind[k] == 2) & (id[k] >= 0)), ("glass_on_spheres", (kind[k] == 2) & (id[k] < -1)),
                          ("mirror_on_spheres", (kind[k] != 2) & (id[k] < -1))):
            events[name] = events.get(name, 0) + int(sel.sum())
    if len(k) == 0:
        return sw
    n = normalize(interpolated_normals(nrm, id[k], tuv[k, 1], tuv[k, 2]))
    if sph is not None:
        c4 = sph[np.clip(-2 - id[k], 0, len(sph) - 1)]
        n = np.where((id[k] < -1)[:, None], normalize((x_next[k] - c4[:, 0:3]).astype(F)), n).astype(F)
    sw[k] = scatter_weight(n, d_in[k], d_next[k], mirror=kind[k] != 2, events=events)
    if events is not None and "vertices" in events:          # a list: (n, d_in, d_out, mirror) of every cast
        events["vertices"].append((n, d_in[k].copy(), d_next[k].copy(), kind[k] != 2))
    return sw


def paths(osc, p, rows=None):
    """The oracle's casts of every (sample, row, column): rays (N, D, 6), ids (N, D),
    tuv (N, D, 3), the cast count (N,) and the global pixel and sample of each."""
    rows = [int(r) for r in (range(p.height) if rows is None else rows)]
    D = p.max_depth
    n = p.spp * len(rows) * p.width
    rays, ids, tuv = np.zeros((n, D, 6), F), np.full((n, D), -1, np.int32), np.zeros((n, D, 3), F)
    cnt, pix, smp = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    L = np.zeros(3, F)
    k = 0
    for s in range(p.spp):
        for y in rows:
            for px in range(p.width):
                cnt[k] = O.lib.oracle_trace_sample(osc.h, ctypes.byref(p), px, y, s, rays[k].ctypes.data,
                                                   ids[k].ctypes.data, tuv[k].ctypes.data, L.ctypes.data)
                pix[k], smp[k] = y * p.width + px, s
                k += 1
    return rays, ids, tuv, cnt, pix, smp, (p.spp, len(rows), p.width)


def contributions(mesh, p, albedo, emission, light_mesh=None, sky=None, rows=None, on=True, count=None, textures=None):
    """x[s] (spp, 3, rows, width) float32 of the scene `mesh` (its "spheres" /
    "sphere_mat" / "kinds" keys included) under OracleParams p with light sampling on.
    light_mesh: the mesh the table is built from (default: mesh).  sky: None (the
    constant p.env) or (tex, rot) for an environment map.  on=False: the plain
    estimator, restated the same way.  textures: {material: (H, W, 3) image}.
    count: a dict that receives shadow_casts and the events of EVENTS."""
    albedo = np.asarray(albedo, F).reshape(-1, 3)
    emi = None if emission is None else np.asarray(emission, F).reshape(-1, 3)
    osc = O.OracleScene(mesh, albedo=albedo, emission=emi, textures=textures)
    rays, ids, tuv, cnt, pix, smp, shape = paths(osc, p, rows)
    N, D = ids.shape
    mat_id = np.asarray(mesh["mat_id"], np.int64) if mesh.get("mat_id") is not None else np.zeros(len(mesh["pos_tri"]), np.int64)
    sph = None if mesh.get("spheres") is None else np.asarray(mesh["spheres"], F).reshape(-1, 4)
    sph_mat = None if sph is None else np.asarray(mesh["sphere_mat"], np.int64)
    kinds = np.zeros(0, np.int64) if mesh.get("kinds") is None else np.asarray(mesh["kinds"], np.int64)
    lm = mesh if light_mesh is None else light_mesh
    table = light_table(tri_soup(lm), lm.get("mat_id"), emi)
    on = on and len(table[0]) > 0
    nrm = shading_normals(mesh)
    env = np.array(list(p.env), F)
    T, L = np.ones((N, 3), F), np.zeros((N, 3), F)
    bit, active = np.zeros(N, bool), np.ones(N, bool)
    after_spec = np.zeros(N, bool)                 # the ray of this cast left a mirror or glass vertex
    ev = dict.fromkeys(EVENTS, 0)
    if count is not None and "vertices" in count:  # a list that receives every mirror and glass vertex
        ev["vertices"] = count["vertices"]
    shadow_casts = 0
    for j in range(D):
        assert np.array_equal(active, cnt > j)
        idj = ids[:, j].astype(np.int64)
        miss = active & (idj == -1)
        ev["escapes_after_specular"] += int((miss & after_spec).sum())
        if miss.any():
            E = np.broadcast_to(env, (N, 3))
            if sky is not None:
                import envmap_ref
                E = (env * envmap_ref.lookup(sky[0], sky[1], rays[:, j, 3:6])).astype(F)
            L = np.where(miss[:, None], (L + (T * E).astype(F)).astype(F), L)
        hit = active & (idj != -1)
        tri = idj >= 0
        m = np.where(tri, mat_id[np.clip(idj, 0, len(mat_id) - 1)], 0)
        if sph is not None:
            m = np.where(idj < -1, sph_mat[np.clip(-2 - idj, 0, len(sph_mat) - 1)], m)
        if emi is not None:
            em = hit & (m >= 0) & (m < len(emi)) & ~(bit & tri)
            L = np.where(em[:, None], (L + (T * emi[np.clip(m, 0, len(emi) - 1)]).astype(F)).astype(F), L)
            ev["emitter_hits_after_specular"] += int((em & tri & after_spec & emits(emi, m)).sum())
        cont = hit & (j + 1 < D)
        T = np.where(cont[:, None], (T * reflectance(mesh, textures, m, idj, tuv[:, j, 1], tuv[:, j, 2], albedo)).astype(F), T)
        if j + 1 >= p.rr_start_depth:
            q = np.max(T, axis=1)
            rr = cont & (q < 1)
            die = rr & (rr_uniform(pix, smp, np.full(N, j)) >= q)
            with np.errstate(all="ignore"):
                T = np.where((rr & ~die)[:, None], (T / q[:, None]).astype(F), T)
            cont = cont & ~die
        kind = np.where((m >= 0) & (m < len(kinds)), kinds[np.clip(m, 0, max(len(kinds) - 1, 0))] if len(kinds) else 0, 0)
        if j + 1 < D:                              # the scatter weight: after the roulette, continuing paths only
            sw = specular_weights(nrm, sph, kind, cont, idj, tuv[:, j], rays[:, j, 3:6], rays[:, j + 1, 0:3],
                                  rays[:, j + 1, 3:6], ev)
            T = np.where(cont[:, None], (T * sw[:, None]).astype(F), T)
        after_spec = cont & (kind != 0)
        diffuse = cont & (kind == 0)
        if on and diffuse.any():
            k = np.nonzero(diffuse)[0]
            assert np.all(cnt[k] > j + 1)
            x = rays[k, j + 1, 0:3]                     # the bounce ray starts at the hit point
            u, v = tuv[k, j, 1], tuv[k, j, 2]
            w = ((F(1) - u).astype(F) - v).astype(F)
            nv = nrm[np.clip(idj[k], 0, len(nrm) - 1)]
            sn = (((w[:, None] * nv[:, 0]).astype(F) + (u[:, None] * nv[:, 1]).astype(F)).astype(F)
                  + (v[:, None] * nv[:, 2]).astype(F)).astype(F)
            nh = sn                                    # as the bounce sampler takes it: not normalised
            if sph is not None:
                onsph = idj[k] < -1
                c4 = sph[np.clip(-2 - idj[k], 0, len(sph) - 1)]
                ns = normalize((x - c4[:, 0:3]).astype(F))
                nl = np.where((dot(ns, rays[k, j, 3:6]) < 0)[:, None], ns, -ns).astype(F)
                nh = np.where(onsph[:, None], nl, nh).astype(F)
            xi = [light_uniform(pix[k], smp[k], np.full(len(k), j), kk) for kk in range(3)]
            traced, d, tmin, tmax, c, lid = light_sample(table, x, nh, T[k], *xi)
            t = np.nonzero(traced)[0]
            shadow_casts += len(t)
            if len(t):
                hid = osc.intersect(x[t].T.copy(), d[t].T.copy(), tmin=tmin[t], tmax=tmax[t], closest=True)[0]
                vis = t[hid == lid[t].astype(np.int64)]
                L[k[vis]] = (L[k[vis]] + c[vis]).astype(F)
                ev["shadow_rays_stopped_by_specular"] += int((hit_kinds(hid, mat_id, sph_mat, kinds) != 0).sum())
        bit = diffuse & on
        active = cont
    if count is not None:
        count.update(ev)
        count["shadow_casts"] = shadow_casts
    S, R, Wd = shape
    return np.ascontiguousarray(np.moveaxis(L.reshape(S, R, Wd, 3), -1, 1))
