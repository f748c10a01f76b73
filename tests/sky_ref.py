"""numpy restatement of sky sampling (include/spt.h
spt_scene_set_sky_sampling), written from the definition, not from the
library: the table in float64, everything a path does with it in float32, one
rounded operation at a time.

  table     Y = max(|r|, |g|, |b|);  Ybar(i, j) = sum_{dy} sum_{dx} (k(dx) k(dy)) Y(wrap(i + dx, j + dy)),
            k = (1/8, 3/4, 1/8), added in that order from 0;  w = Ybar / l^3, l = |p_c| of the
            texel centre's octahedron point (bad w -> 0);  row_j = sum_i w, total = sum_j row_j
            marg_j = f32(sum_{j'<=j} row / total), cond(i, j) = f32(sum_{i'<=i} w / row_j), the last
            entries 1;  pdf(i, j) = f32((w / total) (n n / 4))
  uniforms  sky_uniform(pixel, sample, cast, k), k = 0 .. 4: a 32-bit hash, top 24 bits
  vertex    j = smallest index with xi0 < marg_j, i = smallest with xi1 < cond(i, j)
            a = ((i + xi2) / n) 2 - 1, b likewise from j, xi3;  p = unfold(a, b);  d = R^T p
            rl = 1 / sqrt(d . d);  cx as light sampling's (nee_ref), of the bounce sampler's normal
            pdf(d) = pdf[cell of the lookup's (a, b) of R d, clamped] (|e| / s)^3
            g = cx / (pi pdf(d));  cx > 0, pdf > 0, g < inf;  c = (T (env M(d))) g != 0: the shadow
            ray d is traced over [0.001 rl, inf); it meets nothing: L = L + c
  share     light sampling on too: xi4 < share samples the sky, c / share; else the triangles
            (nee_ref.light_sample), c / (1 - share)
  escape    the ray after such a vertex adds no sky if it escapes

contributions() extends nee_ref.contributions' loop with the second bit and the share."""
import numpy as np

import envmap_ref as E
import nee_ref as R
import oracle as O  # noqa: F401  (the oracle library is loaded by nee_ref's import too)

F = np.float32
U = np.uint32
PI = R.PI
TMIN = R.TMIN


# ---- the table

def sky_table(tex):
    """(marg (n,), cond (n, n), pdf (n, n)) float32 and P (n, n) float64, the cells'
    probabilities; None for an empty table.  tex: (n, n, 3), row j, column i."""
    tex = np.asarray(tex, F)
    n = tex.shape[0]
    assert tex.shape == (n, n, 3)
    with np.errstate(all="ignore"):
        Y = np.fmax(np.fmax(np.abs(tex[..., 0]), np.abs(tex[..., 1])), np.abs(tex[..., 2])).astype(np.float64)
        jj, ii = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        k = (0.125, 0.75, 0.125)
        yb = np.zeros((n, n))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                wi, wj = E.wrap(n, ii + dx, jj + dy)
                yb = yb + (k[dx + 1] * k[dy + 1]) * Y[wj, wi]
        a = (ii + 0.5) / n * 2.0 - 1.0
        b = (jj + 0.5) / n * 2.0 - 1.0
        z = 1.0 - np.abs(a) - np.abs(b)
        x = np.where(z < 0, (1.0 - np.abs(b)) * np.where(a < 0, -1.0, 1.0), a)
        y = np.where(z < 0, (1.0 - np.abs(a)) * np.where(b < 0, -1.0, 1.0), b)
        l = np.sqrt((x * x + y * y) + z * z)
        w = yb / ((l * l) * l)
        w = np.where(np.isfinite(w) & (w > 0), w, 0.0)
        runw = np.cumsum(w, axis=1)                       # sequential along a row
        row = runw[:, -1]
        runr = np.cumsum(row)
        total = runr[-1]
        if not (total > 0 and np.isfinite(total)):
            return None
        marg = (runr / total).astype(F)
        marg[-1] = F(1)
        cond = np.where(row[:, None] > 0, runw / np.where(row > 0, row, 1.0)[:, None], 0.0).astype(F)
        cond[:, -1] = F(1)
        pdf = ((w / total) * ((float(n) * float(n)) / 4.0)).astype(F)
    return marg, cond, pdf, w / total


# ---- the side stream

def sky_uniform(pixel, sample, depth, k):
    pixel, sample, depth = (np.asarray(a, np.uint64).astype(U) for a in (pixel, sample, depth))
    with np.errstate(over="ignore"):
        h = (pixel * U(0xB5297A4D)) ^ ((sample + U(0x68E31DA4)).astype(U) * U(0x1B56C4E9)) ^ \
            ((depth * U(5) + U(k) + U(1)).astype(U) * U(0xA3D8F1C7))
        return R._hash(h, 16, 0x7FEB352D, 15, 0x846CA68B, 16)


# ---- the vertex

def unfold(a, b):
    """(a, b) of the octahedral square -> p on the L1 octahedron, float32 (..., 3)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    fa, fb = np.abs(a), np.abs(b)
    z = ((F(1) - fa).astype(F) - fb).astype(F)
    up = (fa + fb).astype(F) <= F(1)
    x = np.where(up, a, ((F(1) - fb).astype(F) * E.sgn(a)).astype(F))
    y = np.where(up, b, ((F(1) - fa).astype(F) * E.sgn(b)).astype(F))
    return np.stack([x, y, z], axis=-1).astype(F)


def search(cdf, xi):
    """The smallest index with xi < cdf[index], per row of cdf (m, n) and xi (m,)."""
    i = (np.asarray(xi, F)[:, None] >= cdf).sum(axis=1)
    assert i.max() < cdf.shape[1]
    return i


def sky_direction(table, rot, xi0, xi1, xi2, xi3):
    """(d, i, j): the world direction d = R^T p drawn from the table and its cell."""
    marg, cond = table[0], table[1]
    n = len(marg)
    j = search(np.broadcast_to(marg, (len(xi0), n)), xi0)
    i = search(cond[j], xi1)
    fn = F(n)
    a = ((((i.astype(F) + np.asarray(xi2, F)).astype(F) / fn).astype(F) * F(2)).astype(F) - F(1)).astype(F)
    b = ((((j.astype(F) + np.asarray(xi3, F)).astype(F) / fn).astype(F) * F(2)).astype(F) - F(1)).astype(F)
    p = unfold(a, b)
    r = np.asarray(rot, F).reshape(3, 3)
    d = np.stack([(((r[0, k] * p[:, 0]).astype(F) + (r[1, k] * p[:, 1]).astype(F)).astype(F)
                   + (r[2, k] * p[:, 2]).astype(F)).astype(F) for k in range(3)], axis=-1)
    return d, i, j


def sky_pdf(table, rot, d):
    """The sampler's solid-angle density in the world directions d (m, 3), float32."""
    pdf = table[2]
    n = pdf.shape[0]
    d = np.asarray(d, F)
    r = np.asarray(rot, F).reshape(3, 3)
    with np.errstate(all="ignore"):
        e = [(((r[k, 0] * d[:, 0]).astype(F) + (r[k, 1] * d[:, 1]).astype(F)).astype(F)
              + (r[k, 2] * d[:, 2]).astype(F)).astype(F) for k in range(3)]
        ex, ey, ez = e
        s = ((np.abs(ex) + np.abs(ey)).astype(F) + np.abs(ez)).astype(F)
        valid = (s > 0) & (s < np.inf)
        ss = np.where(valid, s, F(1))
        a, b = (ex / ss).astype(F), (ey / ss).astype(F)
        fa = ((F(1) - np.abs(b)).astype(F) * E.sgn(a)).astype(F)
        fb = ((F(1) - np.abs(a)).astype(F) * E.sgn(b)).astype(F)
        low = ez < 0
        a, b = np.where(low, fa, a), np.where(low, fb, b)
        fn = F(n)
        fi = np.floor((((a * F(0.5)).astype(F) + F(0.5)).astype(F) * fn).astype(F))
        fj = np.floor((((b * F(0.5)).astype(F) + F(0.5)).astype(F) * fn).astype(F))
        i = np.clip(fi.astype(np.int64), 0, n - 1)
        j = np.clip(fj.astype(np.int64), 0, n - 1)
        ln = np.sqrt((((ex * ex).astype(F) + (ey * ey).astype(F)).astype(F) + (ez * ez).astype(F)).astype(F)).astype(F)
        q = (ln / ss).astype(F)
        out = (pdf[j, i] * ((q * q).astype(F) * q).astype(F)).astype(F)
    return np.where(valid, out, F(0)).astype(F)


def bounce_cx(nh, d, rl):
    """pi times the bounce sampler's density toward d (nee_ref.light_sample's cx)."""
    with np.errstate(all="ignore"):
        bx, by, bz = R.frame(np.asarray(nh, F))
        c1, c2, c3 = R.cross(by, bz), R.cross(bz, bx), R.cross(bx, by)
        det = R.dot(bx, c1).astype(F)
        v = np.stack([R.dot(d, c1), R.dot(d, c2), R.dot(d, c3)], axis=-1).astype(F)
        vv = R.dot(v, v).astype(F)
        return (((v[..., 1] * det).astype(F) * np.abs(det)).astype(F)
                / ((vv * vv).astype(F) * ((rl * rl).astype(F) * rl).astype(F)).astype(F)).astype(F)


def sky_sample(table, tex, rot, env, nh, T, xi0, xi1, xi2, xi3):
    """(traced, d, tmin, c): whether a shadow ray is traced from vertices with the
    bounce sampler's normals nh and throughputs T, its direction, the start of
    its interval and the contribution it carries."""
    d, _, _ = sky_direction(table, rot, xi0, xi1, xi2, xi3)
    env = np.asarray(env, F)
    with np.errstate(all="ignore"):
        rl = (F(1) / np.sqrt(R.dot(d, d)).astype(F)).astype(F)
        cx = bounce_cx(nh, d, rl)
        pdf = sky_pdf(table, rot, d)
        g = (cx / (PI * pdf).astype(F)).astype(F)
        ok = (cx > 0) & (pdf > 0) & (g < np.inf)
        M = E.lookup(tex, rot, d)
        c = ((T * (env * M).astype(F)).astype(F) * g[:, None]).astype(F)
    c = np.where(ok[:, None], c, F(0)).astype(F)
    traced = ok & np.any(c != 0, axis=1)
    return traced, d, (TMIN * rl).astype(F), c


# ---- a render

def contributions(mesh, p, albedo, emission, sky, on=True, nee=False, share=0.5, light_mesh=None, rows=None, count=None,
                  textures=None):
    """x[s] (spp, 3, rows, width) float32 of the scene `mesh` under OracleParams p and the
    sky image sky = (tex, rot), with sky sampling `on`, light sampling `nee` and the
    given share.  textures: {material: (H, W, 3) image}.  count: a dict that receives
    shadow_casts, the numbers of sky shadow rays that were visible and occluded, and
    nee_ref.EVENTS."""
    tex, rot = np.asarray(sky[0], F), np.asarray(sky[1], F).reshape(3, 3)
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
    nee = nee and len(ltab[0]) > 0
    stab = sky_table(tex)
    on = on and stab is not None
    share = F(share)
    nrm = R.shading_normals(mesh)
    env = np.array(list(p.env), F)
    T, L = np.ones((N, 3), F), np.zeros((N, 3), F)
    bit_tri, bit_sky, active = np.zeros(N, bool), np.zeros(N, bool), np.ones(N, bool)
    after_spec = np.zeros(N, bool)                 # the ray of this cast left a mirror or glass vertex
    ev = dict.fromkeys(R.EVENTS, 0)
    shadow_casts = vis_sky = occ_sky = 0
    for j in range(D):
        assert np.array_equal(active, cnt > j)
        idj = ids[:, j].astype(np.int64)
        miss = active & (idj == -1) & ~bit_sky
        ev["escapes_after_specular"] += int((miss & after_spec).sum())
        if miss.any():
            Ev = (env * E.lookup(tex, rot, rays[:, j, 3:6])).astype(F)
            L = np.where(miss[:, None], (L + (T * Ev).astype(F)).astype(F), L)
        hit = active & (idj != -1)
        tri = idj >= 0
        m = np.where(tri, mat_id[np.clip(idj, 0, len(mat_id) - 1)], 0)
        if sph is not None:
            m = np.where(idj < -1, sph_mat[np.clip(-2 - idj, 0, len(sph_mat) - 1)], m)
        if emi is not None:
            em = hit & (m >= 0) & (m < len(emi)) & ~(bit_tri & tri)
            L = np.where(em[:, None], (L + (T * emi[np.clip(m, 0, len(emi) - 1)]).astype(F)).astype(F), L)
            ev["emitter_hits_after_specular"] += int((em & tri & after_spec & R.emits(emi, m)).sum())
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
            sw = R.specular_weights(nrm, sph, kind, cont, idj, tuv[:, j], rays[:, j, 3:6], rays[:, j + 1, 0:3],
                                    rays[:, j + 1, 3:6], ev)
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
            dj = np.full(len(k), j)
            if on and nee:
                pick_sky = sky_uniform(pix[k], smp[k], dj, 4) < share
            else:
                pick_sky = np.full(len(k), on)
            ks = np.nonzero(pick_sky)[0]
            if len(ks):
                xi = [sky_uniform(pix[k[ks]], smp[k[ks]], dj[ks], kk) for kk in range(4)]
                traced, d, tmin, c = sky_sample(stab, tex, rot, env, nh[ks], T[k[ks]], *xi)
                if nee:
                    with np.errstate(all="ignore"):
                        c = (c / share).astype(F)
                t = np.nonzero(traced)[0]
                shadow_casts += len(t)
                if len(t):
                    hid = osc.intersect(x[ks[t]].T.copy(), d[t].T.copy(), tmin=tmin[t],
                                        tmax=np.full(len(t), np.inf, F), closest=True)[0]
                    vis = t[hid == -1]
                    vis_sky += len(vis)
                    occ_sky += len(t) - len(vis)
                    L[k[ks[vis]]] = (L[k[ks[vis]]] + c[vis]).astype(F)
                    hk = R.hit_kinds(hid, mat_id, sph_mat, kinds)
                    ev["shadow_rays_stopped_by_specular"] += int((hk != 0).sum())
                    ev["sky_rays_stopped_by_specular_sphere"] += int(((hk != 0) & (hid < -1)).sum())
            kt = np.nonzero(~pick_sky)[0]
            if nee and len(kt):
                xi = [R.light_uniform(pix[k[kt]], smp[k[kt]], dj[kt], kk) for kk in range(3)]
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
        count.update(shadow_casts=shadow_casts, sky_visible=vis_sky, sky_occluded=occ_sky)
    S, Rr, Wd = shape
    return np.ascontiguousarray(np.moveaxis(L.reshape(S, Rr, Wd, 3), -1, 1))
