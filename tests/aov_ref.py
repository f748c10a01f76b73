"""Reference for spt_render_aov (include/spt.h), used by the GPU tests.

The first cast of every (pixel, sample) comes from the CPU oracle
(oracle_trace_sample: ray, hit id, t, u, v).  The un-normalised shading
normal, material id and texcoord of the triangle hits come from the existing
spt_hit_info_compute on those rays and hits.  Everything else is restated
here in numpy float32 in the documented operation order: normalise as
v * (1 / sqrt(v.v)), sphere normal from (o + t d) - c, albedo from the table
or the image, the sample-ordered f32 sum from 0, then / float32(spp).
"""
import ctypes

import numpy as np
import torch

import oracle as O
from sptamd import _lib

F = np.float32


def first_hits(osc, p, rows):
    """Oracle first casts of every pixel of `rows` and every sample: dict of
    arrays shaped (len(rows), W, spp[, 3])."""
    n, w, spp = len(rows), p.width, p.spp
    out = dict(o=np.zeros((n, w, spp, 3), F), d=np.zeros((n, w, spp, 3), F), id=np.full((n, w, spp), -1, np.int32),
               t=np.zeros((n, w, spp), F), u=np.zeros((n, w, spp), F), v=np.zeros((n, w, spp), F))
    rays = np.zeros((p.max_depth, 6), F)
    ids = np.zeros(p.max_depth, np.int32)
    tuv = np.zeros((p.max_depth, 3), F)
    rad = np.zeros(3, F)
    for i, y in enumerate(rows):
        for x in range(w):
            for s in range(spp):
                k = O.lib.oracle_trace_sample(osc.h, ctypes.byref(p), x, int(y), s, rays.ctypes.data, ids.ctypes.data,
                                              tuv.ctypes.data, rad.ctypes.data)
                assert k >= 1
                out["o"][i, x, s] = rays[0, :3]
                out["d"][i, x, s] = rays[0, 3:]
                out["id"][i, x, s] = ids[0]
                if ids[0] != -1:
                    out["t"][i, x, s], out["u"][i, x, s], out["v"][i, x, s] = tuv[0]
    return out


def hit_info(scene, h):
    """spt_hit_info_compute on the oracle's rays and hits: un-normalised shading
    normal (N, 3), material id (N,), texcoord (N, 2) per sample (flattened)."""
    dev = scene.backend.device
    n = h["id"].size
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    o, d = up(h["o"].reshape(n, 3).T), up(h["d"].reshape(n, 3).T)
    tri, t, u, v = up(h["id"].reshape(n)), up(h["t"].reshape(n)), up(h["u"].reshape(n)), up(h["v"].reshape(n))
    sn = torch.zeros((3, n), dtype=torch.float32, device=dev)
    tc = torch.zeros((2, n), dtype=torch.float32, device=dev)
    mat = torch.zeros(n, dtype=torch.int32, device=dev)
    rays = _lib.Rays(o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), d[0].data_ptr(), d[1].data_ptr(),
                     d[2].data_ptr(), None, None)
    hits = _lib.Hits(tri.data_ptr(), t.data_ptr(), u.data_ptr(), v.data_ptr())
    info = _lib.HitInfo()
    info.snx, info.sny, info.snz = sn[0].data_ptr(), sn[1].data_ptr(), sn[2].data_ptr()
    info.tcu, info.tcv, info.mat_id = tc[0].data_ptr(), tc[1].data_ptr(), mat.data_ptr()
    _lib.check(_lib.lib.spt_hit_info_compute(scene.backend.handle, ctypes.byref(rays), ctypes.byref(hits), None, 0, n,
                                             ctypes.byref(info), None), "spt_hit_info_compute")
    torch.cuda.synchronize()
    return sn.cpu().numpy().T.copy(), mat.cpu().numpy(), tc.cpu().numpy().T.copy()


def reference_planes(scene, mesh, h, albedo=None, textures=None):
    """The eight planes from first_hits' dict `h`: {"albedo": (3, rows, W),
    "normal": (3, rows, W), "depth": (rows, W), "coverage": (rows, W)}."""
    rows, w, spp = h["id"].shape
    n = rows * w * spp
    ids = h["id"].reshape(n)
    o, d, t = h["o"].reshape(n, 3), h["d"].reshape(n, 3), h["t"].reshape(n)
    sn, mat, tc = hit_info(scene, h)
    hit, sph = ids != -1, ids < -1
    mat = mat.astype(np.int64)
    if sph.any():
        k = -2 - ids[sph]
        c = np.asarray(mesh["spheres"], F)[k, :3]
        x = (o[sph] + t[sph, None] * d[sph]).astype(F)     # o + t d, as scatter() forms the hit point
        sn[sph] = x - c
        sm = mesh.get("sphere_mat")
        mat[sph] = 0 if sm is None else np.asarray(sm, np.int64)[k]
        tc[sph] = 0.0                                        # spheres look their image up at (0, 0)
    sn[~hit] = 0.0
    len2 = ((sn[:, 0] * sn[:, 0] + sn[:, 1] * sn[:, 1]) + sn[:, 2] * sn[:, 2]).astype(F)
    ok = hit & (len2 > 0) & np.isfinite(len2)
    inv = np.zeros(n, F)
    inv[ok] = F(1.0) / np.sqrt(len2[ok])
    normal = np.where(ok[:, None], sn * inv[:, None], F(0.0)).astype(F)
    alb = np.ones((1, 3), F) if albedo is None else np.asarray(albedo, F).reshape(-1, 3)
    m0 = np.where((mat >= 0) & (mat < len(alb)), mat, 0)
    rf = alb[m0].copy()
    for m, img in (textures or {}).items():
        for i in np.nonzero(hit & (mat == m))[0]:
            rf[i] = O.texture_eval(img, float(tc[i, 0]), float(tc[i, 1]))
    rf[~hit] = 0.0
    cov = hit.astype(F)
    depth = np.where(hit, t, F(0.0)).astype(F)

    def resolve(a):  # sample-ordered f32 sum from 0, then / float32(spp)
        a = a.reshape((rows, w, spp) + a.shape[1:])
        acc = np.zeros((rows, w) + a.shape[3:], F)
        for s in range(spp):
            acc = (acc + a[:, :, s]).astype(F)
        return (acc / F(spp)).astype(F)

    return {"albedo": np.ascontiguousarray(np.moveaxis(resolve(rf), -1, 0)),
            "normal": np.ascontiguousarray(np.moveaxis(resolve(normal), -1, 0)),
            "depth": resolve(depth), "coverage": resolve(cov)}


def gpu_planes(scene, params, **kw):
    res = scene.render_aov(params, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}
