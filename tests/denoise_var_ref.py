"""numpy restatement of spt_denoise_var's filter (include/spt.h; the spatial
filter of Schied et al. 2017), parametrised by dtype, and the heteroscedastic
synthetic inputs its tests share.  Written from the definition, not from the
kernel:

  v_0(p) = max((var_r + var_g) + var_b, 0)
  iteration i = 0 .. iterations-1, step 2^i:
    vt(p) = sum g v_i(q) / sum g over the 3 x 3 adjacent taps inside the image,
            g = g1[|dx|] g1[|dy|], g1 = {1/2, 1/4};
    e_c = |c_i(p) - c_i(q)|^2 / (sigma_variance^2 vt(p) + 1e-10);
    e_n, e_a, e_z, the 5 x 5 taps q = p + 2^i (dx, dy) and k as spt_denoise (denoise_ref.py);
    w = k exp(-(e_c + e_n + e_a + e_z));
    c_{i+1}(p) = sum w c_i(q) / sum w;   v_{i+1}(p) = sum w^2 v_i(q) / (sum w)^2.
"""
import numpy as np

import denoise_ref as R

G1 = (0.5, 0.25)
STD_LO, STD_HI = 0.03, 0.3


def v0(variance, dtype=np.float64):
    v = np.asarray(variance).astype(dtype)
    return np.maximum((v[0] + v[1]) + v[2], np.dtype(dtype).type(0))


def atrous_var(color, variance, normal=None, albedo=None, depth=None, iterations=5, sigma_variance=4.0,
               sigma_normal=0.0, sigma_albedo=0.0, sigma_depth=0.0, dtype=np.float64):
    """color, variance, normal, albedo: (3, H, W); depth: (H, W).  A None guide
    or a sigma <= 0 disables the term.  Every operation runs in `dtype`.
    Returns (filtered colour (3, H, W), filtered variance (H, W))."""
    T = np.dtype(dtype).type
    c = np.asarray(color).astype(dtype)
    v = v0(variance, dtype)
    n = None if normal is None or sigma_normal <= 0 else np.asarray(normal).astype(dtype)
    a = None if albedo is None or sigma_albedo <= 0 else np.asarray(albedo).astype(dtype)
    z = None if depth is None or sigma_depth <= 0 else np.asarray(depth).astype(dtype)
    for i in range(iterations):
        step = 1 << i
        den_c = None
        if sigma_variance > 0:
            gv = np.zeros(v.shape, dtype)
            gs = np.zeros(v.shape, dtype)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    vw = R._views(v, dy, dx)
                    if vw is None:
                        continue
                    (py, px), (qy, qx) = vw
                    g = T(G1[abs(dx)]) * T(G1[abs(dy)])
                    gv[py, px] += g * v[qy, qx]
                    gs[py, px] += g
            den_c = T(sigma_variance) * T(sigma_variance) * (gv / gs) + T(1e-10)
        num = np.zeros_like(c)
        den = np.zeros(c.shape[1:], dtype)
        vnum = np.zeros(c.shape[1:], dtype)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                vw = R._views(c, dy * step, dx * step)
                if vw is None:
                    continue
                (py, px), (qy, qx) = vw
                e = np.zeros(c[0, py, px].shape, dtype)
                if den_c is not None:
                    e = e + ((c[:, py, px] - c[:, qy, qx]) ** 2).sum(0) / den_c[py, px]
                if n is not None:
                    e = e + ((n[:, py, px] - n[:, qy, qx]) ** 2).sum(0) / (T(sigma_normal) * T(sigma_normal))
                if a is not None:
                    e = e + ((a[:, py, px] - a[:, qy, qx]) ** 2).sum(0) / (T(sigma_albedo) * T(sigma_albedo))
                if z is not None:
                    zp = z[py, px]
                    e = e + (zp - z[qy, qx]) ** 2 / (T(sigma_depth) * T(sigma_depth) * np.maximum(zp * zp, T(1e-12)))
                w = T(R.H[abs(dx)]) * T(R.H[abs(dy)]) * np.exp(-e)
                num[:, py, px] += w * c[:, qy, qx]
                den[py, px] += w
                vnum[py, px] += (w * w) * v[qy, qx]
        c = (num / den).astype(dtype)
        v = (vnum / (den * den)).astype(dtype)
    return c, v


def synthetic(seed=5, w=R.W, h=R.HGT):
    """denoise_ref.synthetic's regions with heteroscedastic noise: the per-pixel
    standard deviation rises from 0.03 at the left edge to 0.3 at the right, and
    the sky is exactly converged (no noise, variance 0).  Adds `variance`
    (3, H, W): the true per-channel variance of each pixel, and `std` (H, W)."""
    d = R.synthetic(seed=seed, w=w, h=h)
    rng = np.random.default_rng(seed + 1000)
    std = np.broadcast_to(np.linspace(STD_LO, STD_HI, w), (h, w)).copy()
    std[d["sky"]] = 0.0
    clean = d["clean"].astype(np.float64)
    color = clean + rng.normal(0.0, 1.0, clean.shape) * std
    d["color"] = np.ascontiguousarray(color, dtype=np.float32)
    d["variance"] = np.ascontiguousarray(np.broadcast_to(std * std, clean.shape), dtype=np.float32)
    d["std"] = std
    return d


def tolerance(kw):
    """((tol colour, tol variance), (f64 colour, f64 variance)): 8 x max|f32
    restatement - f64 restatement| of each output for the filter arguments kw
    (the factor allows for expf and summation-order differences between numpy
    and the device, as in denoise_ref.tolerance)."""
    c64, v64 = atrous_var(dtype=np.float64, **kw)
    c32, v32 = atrous_var(dtype=np.float32, **kw)
    return ((8.0 * float(np.abs(c32.astype(np.float64) - c64).max()),
             8.0 * float(np.abs(v32.astype(np.float64) - v64).max())), (c64, v64))
