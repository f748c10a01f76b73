"""numpy restatement of spt_denoise's filter (include/spt.h; Dammertz et al.
2010), parametrised by dtype, and the synthetic inputs the denoiser tests
share.  Written from the definition, not from the kernel:

  iteration i = 0 .. iterations-1, step 2^i; for pixel p the 5 x 5 taps
  q = p + 2^i (dx, dy) inside the image; k = h[|dx|] h[|dy|], h = {3/8, 1/4, 1/16};
  w = k exp(-(e_c + e_n + e_a + e_z)),
  e_c = |c_i(p) - c_i(q)|^2 / (sigma_color 2^-i)^2,  e_n = |n(p) - n(q)|^2 / sigma_normal^2,
  e_a = |a(p) - a(q)|^2 / sigma_albedo^2,  e_z = (z(p) - z(q))^2 / (sigma_depth^2 max(z(p)^2, 1e-12));
  c_{i+1}(p) = sum w c_i(q) / sum w.
"""
import numpy as np

H = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
W, HGT = 37, 19
NOISE_STD = 0.1


def _views(a, dy, dx):
    """(centre view, tap view) of a's last two axes for the taps inside the image."""
    h, w = a.shape[-2:]
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def atrous(color, normal=None, albedo=None, depth=None, iterations=5, sigma_color=0.0, sigma_normal=0.0,
           sigma_albedo=0.0, sigma_depth=0.0, dtype=np.float64):
    """color, normal, albedo: (3, H, W); depth: (H, W).  A None guide or a
    sigma <= 0 disables the term.  Every operation runs in `dtype`."""
    T = np.dtype(dtype).type
    c = np.asarray(color).astype(dtype)
    n = None if normal is None or sigma_normal <= 0 else np.asarray(normal).astype(dtype)
    a = None if albedo is None or sigma_albedo <= 0 else np.asarray(albedo).astype(dtype)
    z = None if depth is None or sigma_depth <= 0 else np.asarray(depth).astype(dtype)
    for i in range(iterations):
        step = 1 << i
        num = np.zeros_like(c)
        den = np.zeros(c.shape[1:], dtype)
        sc = T(sigma_color) * T(2.0 ** -i)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                v = _views(c, dy * step, dx * step)
                if v is None:
                    continue
                (py, px), (qy, qx) = v
                e = np.zeros(c[0, py, px].shape, dtype)
                if sigma_color > 0:
                    e = e + ((c[:, py, px] - c[:, qy, qx]) ** 2).sum(0) / (sc * sc)
                if n is not None:
                    e = e + ((n[:, py, px] - n[:, qy, qx]) ** 2).sum(0) / (T(sigma_normal) * T(sigma_normal))
                if a is not None:
                    e = e + ((a[:, py, px] - a[:, qy, qx]) ** 2).sum(0) / (T(sigma_albedo) * T(sigma_albedo))
                if z is not None:
                    zp = z[py, px]
                    e = e + (zp - z[qy, qx]) ** 2 / (T(sigma_depth) * T(sigma_depth) * np.maximum(zp * zp, T(1e-12)))
                w = T(H[abs(dx)]) * T(H[abs(dy)]) * np.exp(-e)
                num[:, py, px] += w * c[:, qy, qx]
                den[py, px] += w
        c = (num / den).astype(dtype)
    return c


def synthetic(seed=5, w=W, h=HGT):
    """Two planes meeting at a normal / albedo / depth edge under a sky strip
    with zero guides; colour = a piecewise-constant signal + seeded noise.
    Returns dict(color, clean, normal, albedo, depth, left, right, sky), float32
    planes and boolean region masks."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    sky = yy < max(1, h // 5)
    left = ~sky & (xx < w // 2)
    right = ~sky & ~left
    clean = np.zeros((3, h, w))
    normal = np.zeros((3, h, w))
    albedo = np.zeros((3, h, w))
    depth = np.zeros((h, w))
    for m, sig, nrm, alb, z0 in ((left, (0.25, 0.2, 0.15), (0.0, 0.0, 1.0), (0.8, 0.3, 0.3), 4.0),
                                 (right, (0.6, 0.7, 0.65), (1.0, 0.0, 0.0), (0.3, 0.3, 0.8), 6.0)):
        for ch in range(3):
            clean[ch][m] = sig[ch]
            normal[ch][m] = nrm[ch]
            albedo[ch][m] = alb[ch]
        depth[m] = z0 + 0.01 * xx[m] + 0.02 * yy[m]
    clean[:, sky] = 1.0
    color = clean + rng.normal(0.0, NOISE_STD, clean.shape)
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)  # noqa: E731
    return dict(color=f(color), clean=f(clean), normal=f(normal), albedo=f(albedo), depth=f(depth), left=left,
                right=right, sky=sky)


def tolerance(kw):
    """(tol, f64 result): tol = 8 x max|f32 restatement - f64 restatement| for
    the filter arguments kw (the factor allows for expf and summation-order
    differences between numpy and the device)."""
    r64 = atrous(dtype=np.float64, **kw)
    r32 = atrous(dtype=np.float32, **kw)
    return 8.0 * float(np.abs(r32.astype(np.float64) - r64).max()), r64


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
