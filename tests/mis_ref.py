"""numpy restatement of multiple importance sampling between a vertex's shadow
ray and its bounce ray (include/spt.h spt_scene_set_mis), written
from the definition, not from the library, on top of nee_ref and sky_ref: the
tables, the side streams, the oracle's paths and the shadow rays' hits are
theirs.  float32, one rounded operation at a time.

In "pi x solid-angle density" units, at a diffuse vertex that bounces:

  cx(n, d)   nee_ref / sky_ref's cx: pi times the bounce sampler's density toward d
  cb         cx(nh, dir_bounce), rl = 1 / sqrt(dir . dir): carried to the path's next shade
  cl         ((pi pdfA) r2) / cy, cy = |ng . d| rl; r2 = 1 / (rl rl) at the sampling vertex,
             (t t) (d . d) at a bounce ray's hit
  cs         pi sky_pdf(d)
  s          1 with one table; share (sky) and f32(1 - share) (triangles) with both

  shadow ray toward a triangle    c = (T Le) q,        q = cx / (cx + s cl)    (no / (1 - share) afterwards)
  shadow ray toward the sky       c = (T (env M)) q,   q = cx / (cx + s cs)    (no / share afterwards)
  the next hit, bit 0 set, on a triangle whose material emits
                                  L = L + (T Le) w,    w = cb / (cb + s cl_hit), the member found by its id
  the next escape, bit 1 set      L = L + (T (env M)) w,  w = cb / (cb + s cs(d))

  degenerate  q: s c* zero, negative or NaN -> +inf (no shadow ray); with the tests cx > 0,
              cy > 0 (pdf > 0) and q < inf as before.  A sum that is +inf gives q = 0: c = 0, no ray.
              w: cb not positive -> 1; the hit triangle not in the table, pdfA not positive
              or cy not positive -> 1; s c* zero, negative or NaN -> 1; the sum +inf -> 0.

contributions() is sky_ref.contributions' loop (and nee_ref's, without a sky
image) with these weights; mis=False it computes exactly what they compute."""
import numpy as np

import envmap_ref as E
import nee_ref as R
import oracle as O
import sky_ref as S

F = np.float32
U = np.uint32
PI = R.PI
INF = F(np.inf)


# ---- the weights

def bounce_cx(nh, d, rl):
    return S.bounce_cx(np.asarray(nh, F), np.asarray(d, F), np.asarray(rl, F))


def inv_len(d):
    with np.errstate(all="ignore"):
        return (F(1) / np.sqrt(R.dot(d, d)).astype(F)).astype(F)


def light_cl(pdfA, r2, cy):
    with np.errstate(all="ignore"):
        return (((PI * np.asarray(pdfA, F)).astype(F) * np.asarray(r2, F)).astype(F) / np.asarray(cy, F)).astype(F)


def shadow_factor(c, sb):
    """q = c / (c + sb), +inf where the shadow-ray sampler cannot produce the direction."""
    c, sb = np.asarray(c, F), np.asarray(sb, F)
    with np.errstate(all="ignore"):
        q = (c / (c + sb).astype(F)).astype(F)
    return np.where(sb > 0, q, INF).astype(F)


def bounce_weight(c, sb):
    """w = c / (c + sb) of what a bounce ray finds."""
    c, sb = np.asarray(c, F), np.asarray(sb, F)
    with np.errstate(all="ignore"):
        den = (c + sb).astype(F)
        w = np.where(den < INF, (c / den).astype(F), F(0))
    return np.where(~(c > 0) | ~(sb > 0), F(1), w).astype(F)


def shadow_weight(c, sb):
    """The shadow-ray sampler's own weight sb / (c + sb) — q is this times the c / sb its
    sample is weighed with.  0 where it traces no ray (c or sb not positive), 1 where the
    sum is not finite."""
    c, sb = np.asarray(c, F), np.asarray(sb, F)
    with np.errstate(all="ignore"):
        den = (c + sb).astype(F)
        w = np.where(den < INF, (sb / den).astype(F), F(1))
    return np.where(~(c > 0) | ~(sb > 0), F(0), w).astype(F)


def light_hit_weight(cb, s, ng, pdfA, d, t):
    cb, s, pdfA, t = (np.asarray(a, F) for a in (cb, s, pdfA, t))
    ng, d = np.asarray(ng, F), np.asarray(d, F)
    with np.errstate(all="ignore"):
        dd = R.dot(d, d).astype(F)
        cy = (np.abs(R.dot(ng, d)) * (F(1) / np.sqrt(dd).astype(F)).astype(F)).astype(F)
        cl = light_cl(pdfA, ((t * t).astype(F) * dd).astype(F), cy)
        w = bounce_weight(cb, (s * cl).astype(F))
    return np.where(~(pdfA > 0) | ~(cy > 0), F(1), w).astype(F)


def escape_weight(cb, s, pdf):
    with np.errstate(all="ignore"):
        return bounce_weight(cb, (np.asarray(s, F) * (PI * np.asarray(pdf, F)).astype(F)).astype(F))


# ---- the vertex

def light_sample(table, x, nh, T, xi0, xi1, xi2, s):
    """nee_ref.light_sample with the MIS factor: (traced, d, tmin, tmax, c, id)."""
    ids, cdf, pdf, tv, ng, le = table
    i = np.minimum(np.searchsorted(cdf, np.asarray(xi0, F), side="right"), len(cdf) - 1)
    b1, b2 = R.tri_map(xi1, xi2)
    b0 = ((F(1) - b1).astype(F) - b2).astype(F)
    v = tv[i]
    y = (((b0[:, None] * v[:, 0:3]).astype(F) + (b1[:, None] * v[:, 3:6]).astype(F)).astype(F)
         + (b2[:, None] * v[:, 6:9]).astype(F)).astype(F)
    d = (y - x).astype(F)
    with np.errstate(all="ignore"):
        rl = inv_len(d)
        tmin = (R.TMIN * rl).astype(F)
        tmax = (F(1) + tmin).astype(F)
        cx = bounce_cx(nh, d, rl)
        cy = (np.abs(R.dot(ng[i], d)) * rl).astype(F)
        cl = light_cl(pdf[i], (F(1) / (rl * rl).astype(F)).astype(F), cy)
        q = shadow_factor(cx, (F(s) * cl).astype(F))
        ok = (tmin <= F(1)) & (cx > 0) & (cy > 0) & (q < INF)
        c = ((T * le[i]).astype(F) * q[:, None]).astype(F)
    c = np.where(ok[:, None], c, F(0)).astype(F)
    return ok & np.any(c != 0, axis=1), d, tmin, tmax, c, ids[i]


def sky_sample(table, tex, rot, env, nh, T, xi0, xi1, xi2, xi3, s):
    """sky_ref.sky_sample with the MIS factor: (traced, d, tmin, c)."""
    d, _, _ = S.sky_direction(table, rot, xi0, xi1, xi2, xi3)
    env = np.asarray(env, F)
    with np.errstate(all="ignore"):
        rl = inv_len(d)
        cx = bounce_cx(nh, d, rl)
        pdf = S.sky_pdf(table, rot, d)
        q = shadow_factor(cx, (F(s) * (PI * pdf).astype(F)).astype(F))
        ok = (cx > 0) & (pdf > 0) & (q < INF)
        M = E.lookup(tex, rot, d)
        c = ((T * (env * M).astype(F)).astype(F) * q[:, None]).astype(F)
    c = np.where(ok[:, None], c, F(0)).astype(F)
    return ok & np.any(c != 0, axis=1), d, (R.TMIN * rl).astype(F), c


# ---- a render

def contributions(mesh, p, albedo, emission, sky=None, nee=False, sky_on=False, share=0.5, mis=False, light_mesh=None,
                  rows=None, count=None, textures=None):
    """x[s] (spp, 3, rows, width) float32 of the scene `mesh` under OracleParams p.  sky: None
    (the constant p.env) or (tex, rot); nee / sky_on: the two samplers' switches; share: the
    sky's where both tables are non-empty; mis: the switch of §16.  textures: {material:
    (H, W, 3) image}.  count: a dict that receives shadow_casts, the numbers of weighted
    hits and escapes, and nee_ref.EVENTS."""
    albedo = np.asarray(albedo, F).reshape(-1, 3)
    emi = None if emission is None else np.asarray(emission, F).reshape(-1, 3)
    osc = O.OracleScene(mesh, albedo=albedo, emission=emi, textures=textures)
    rays, ids, tuv, cnt, pix, smp, shape = R.paths(osc, p, rows)
    N, D = ids.shape
    mat_id = np.asarray(mesh["mat_id"], np.int64) if mesh.get("mat_id") is not None else np.zeros(len(mesh["pos_tri"]), np.int64)
    sph = None if mesh.get("spheres") is None else np.asarray(mesh["spheres"], F).reshape(-1, 4)
    sph_mat = None if sph is None else np.asarray(mesh["sphere_mat"], np.int64)
    kinds = np.zeros(0, np.int64) if mesh.get("kinds") is None else np.asarray(mesh["kinds"], np.int64)
    lm = mesh if light_mesh is None else light_mesh
    ltab = R.light_table(R.tri_soup(lm), lm.get("mat_id"), emi)
    nee = bool(nee) and len(ltab[0]) > 0
    tex = rot = stab = None
    if sky is not None:
        tex, rot = np.asarray(sky[0], F), np.asarray(sky[1], F).reshape(3, 3)
        stab = S.sky_table(tex) if sky_on else None
    on = stab is not None
    mis = bool(mis) and (on or nee)
    share = F(share)
    both = on and nee
    s_sky = share if both else F(1)
    s_tri = (F(1) - share).astype(F) if both else F(1)
    lids, lpdf, lng = ltab[0].astype(np.int64), ltab[2], ltab[4]
    nrm = R.shading_normals(mesh)
    env = np.array(list(p.env), F)
    T, L = np.ones((N, 3), F), np.zeros((N, 3), F)
    bit_tri, bit_sky, active = np.zeros(N, bool), np.zeros(N, bool), np.ones(N, bool)
    cb = np.zeros(N, F)
    after_spec = np.zeros(N, bool)                 # the ray of this cast left a mirror or glass vertex
    ev = dict.fromkeys(R.EVENTS, 0)
    shadow_casts = hits_w = escapes_w = 0
    for j in range(D):
        assert np.array_equal(active, cnt > j)
        idj = ids[:, j].astype(np.int64)
        dj_ray = rays[:, j, 3:6]
        miss = active & (idj == -1)
        ev["escapes_after_specular"] += int((miss & after_spec & ~bit_sky).sum())
        if miss.any():
            Ev = np.broadcast_to(env, (N, 3))
            if sky is not None:
                Ev = (env * E.lookup(tex, rot, dj_ray)).astype(F)
            full = miss & ~bit_sky
            L = np.where(full[:, None], (L + (T * Ev).astype(F)).astype(F), L)
            part = miss & bit_sky & mis
            if part.any():
                k = np.nonzero(part)[0]
                w = escape_weight(cb[k], s_sky, S.sky_pdf(stab, rot, dj_ray[k]))
                L[k] = (L[k] + ((T[k] * Ev[k]).astype(F) * w[:, None]).astype(F)).astype(F)
                escapes_w += len(k)
        hit = active & (idj != -1)
        tri = idj >= 0
        m = np.where(tri, mat_id[np.clip(idj, 0, len(mat_id) - 1)], 0)
        if sph is not None:
            m = np.where(idj < -1, sph_mat[np.clip(-2 - idj, 0, len(sph_mat) - 1)], m)
        if emi is not None:
            emits = hit & (m >= 0) & (m < len(emi))
            em = emits & ~(bit_tri & tri)
            L = np.where(em[:, None], (L + (T * emi[np.clip(m, 0, len(emi) - 1)]).astype(F)).astype(F), L)
            ev["emitter_hits_after_specular"] += int((em & tri & after_spec & R.emits(emi, m)).sum())
            part = emits & bit_tri & tri & mis
            if part.any():
                k = np.nonzero(part)[0]
                pos = np.clip(np.searchsorted(lids, idj[k]), 0, len(lids) - 1)
                found = lids[pos] == idj[k]
                w = light_hit_weight(cb[k], s_tri, lng[pos], lpdf[pos], dj_ray[k], tuv[k, j, 0])
                w = np.where(found, w, F(1)).astype(F)
                le = emi[m[k]]
                L[k] = (L[k] + ((T[k] * le).astype(F) * w[:, None]).astype(F)).astype(F)
                hits_w += len(k)
        cont = hit & (j + 1 < D)
        T = np.where(cont[:, None], (T * R.reflectance(mesh, textures, m, idj, tuv[:, j, 1], tuv[:, j, 2], albedo)).astype(F), T)
        if j + 1 >= p.rr_start_depth:
            q = np.max(T, axis=1)
            rr = cont & (q < 1)
            die = rr & (R.rr_uniform(pix, smp, np.full(N, j)) >= q)
            with np.errstate(all="ignore"):
                T = np.where((rr & ~die)[:, None], (T / q[:, None]).astype(F), T)
            cont = cont & ~die
        kind = np.where((m >= 0) & (m < len(kinds)), kinds[np.clip(m, 0, max(len(kinds) - 1, 0))] if len(kinds) else 0, 0)
        if j + 1 < D:                              # the scatter weight: after the roulette, continuing paths only
            sw = R.specular_weights(nrm, sph, kind, cont, idj, tuv[:, j], dj_ray, rays[:, j + 1, 0:3], rays[:, j + 1, 3:6], ev)
            T = np.where(cont[:, None], (T * sw[:, None]).astype(F), T)
        after_spec = cont & (kind != 0)
        diffuse = cont & (kind == 0)
        if (on or nee) and diffuse.any():
            k = np.nonzero(diffuse)[0]
            assert np.all(cnt[k] > j + 1)
            x = rays[k, j + 1, 0:3]                     # the bounce ray starts at the hit point
            u, v = tuv[k, j, 1], tuv[k, j, 2]
            w = ((F(1) - u).astype(F) - v).astype(F)
            nv = nrm[np.clip(idj[k], 0, len(nrm) - 1)]
            nh = (((w[:, None] * nv[:, 0]).astype(F) + (u[:, None] * nv[:, 1]).astype(F)).astype(F)
                  + (v[:, None] * nv[:, 2]).astype(F)).astype(F)
            if sph is not None:
                onsph = idj[k] < -1
                c4 = sph[np.clip(-2 - idj[k], 0, len(sph) - 1)]
                ns = R.normalize((x - c4[:, 0:3]).astype(F))
                nl = np.where((R.dot(ns, rays[k, j, 3:6]) < 0)[:, None], ns, -ns).astype(F)
                nh = np.where(onsph[:, None], nl, nh).astype(F)
            if mis:
                db = rays[k, j + 1, 3:6]
                cb[k] = bounce_cx(nh, db, inv_len(db))
            dj = np.full(len(k), j)
            if both:
                pick_sky = S.sky_uniform(pix[k], smp[k], dj, 4) < share
            else:
                pick_sky = np.full(len(k), on)
            ks = np.nonzero(pick_sky)[0]
            if len(ks):
                xi = [S.sky_uniform(pix[k[ks]], smp[k[ks]], dj[ks], kk) for kk in range(4)]
                if mis:
                    traced, d, tmin, c = sky_sample(stab, tex, rot, env, nh[ks], T[k[ks]], *xi, s_sky)
                else:
                    traced, d, tmin, c = S.sky_sample(stab, tex, rot, env, nh[ks], T[k[ks]], *xi)
                    if nee:
                        with np.errstate(all="ignore"):
                            c = (c / share).astype(F)
                t = np.nonzero(traced)[0]
                shadow_casts += len(t)
                if len(t):
                    hid = osc.intersect(x[ks[t]].T.copy(), d[t].T.copy(), tmin=tmin[t],
                                        tmax=np.full(len(t), np.inf, F), closest=True)[0]
                    vis = t[hid == -1]
                    L[k[ks[vis]]] = (L[k[ks[vis]]] + c[vis]).astype(F)
                    hk = R.hit_kinds(hid, mat_id, sph_mat, kinds)
                    ev["shadow_rays_stopped_by_specular"] += int((hk != 0).sum())
                    ev["sky_rays_stopped_by_specular_sphere"] += int(((hk != 0) & (hid < -1)).sum())
            kt = np.nonzero(~pick_sky)[0]
            if nee and len(kt):
                xi = [R.light_uniform(pix[k[kt]], smp[k[kt]], dj[kt], kk) for kk in range(3)]
                if mis:
                    traced, d, tmin, tmax, c, lid = light_sample(ltab, x[kt], nh[kt], T[k[kt]], *xi, s_tri)
                else:
                    traced, d, tmin, tmax, c, lid = R.light_sample(ltab, x[kt], nh[kt], T[k[kt]], *xi)
                    if on:
                        with np.errstate(all="ignore"):
                            c = (c / (F(1) - share).astype(F)).astype(F)
                t = np.nonzero(traced)[0]
                shadow_casts += len(t)
                if len(t):
                    hid = osc.intersect(x[kt[t]].T.copy(), d[t].T.copy(), tmin=tmin[t], tmax=tmax[t], closest=True)[0]
                    vis = t[hid == lid[t].astype(np.int64)]
                    L[k[kt[vis]]] = (L[k[kt[vis]]] + c[vis]).astype(F)
                    ev["shadow_rays_stopped_by_specular"] += int((R.hit_kinds(hid, mat_id, sph_mat, kinds) != 0).sum())
        bit_tri = diffuse & nee
        bit_sky = diffuse & on
        active = cont
    if count is not None:
        count.update(ev)
        count.update(shadow_casts=shadow_casts, weighted_hits=hits_w, weighted_escapes=escapes_w)
    Sn, Rr, Wd = shape
    return np.ascontiguousarray(np.moveaxis(L.reshape(Sn, Rr, Wd, 3), -1, 1))
