"""numpy restatement of the environment-map lookup (DESIGN.md §13,
include/spt.h spt_scene_set_envmap), written from the definition, not from the
kernels: float32, one rounded operation at a time, texels fetched from the
N x N image through the octahedral edge rule (no gutter array).

  e   = R d            e_x = (R00 d_x + R01 d_y) + R02 d_z, ...
  s   = (|e_x| + |e_y|) + |e_z|;  M = 0 unless 0 < s < inf
  a, b = e_x / s, e_y / s;  e_z < 0: (a, b) = ((1 - |b|) sgn a, (1 - |a|) sgn b)
  fx  = (a 0.5 + 0.5) N - 0.5, i0 = floor fx, wx = fx - i0   (fy, j0, wy likewise)
  top = (1 - wx) T(i0, j0) + wx T(i0 + 1, j0);  bot: row j0 + 1
  M   = (1 - wy) top + wy bot

and the expected per-sample contributions of a render under a map, from the
oracle's rays and throughputs (contributions): x_s = L_emit + T (env M(d)).
Also the float64 restatement of spt_envmap_from_latlong (from_latlong)."""
import ctypes

import numpy as np

import oracle as O

F = np.float32
EDGES = ("left", "right", "top", "bottom", "corner")


def wrap(n, i, j):
    """Texel indices in [-1, n] -> the texel in [0, n) they stand for: the column first, then the row."""
    i, j = np.array(i, np.int64), np.array(j, np.int64)
    lo, hi = i < 0, i >= n
    j = np.where(lo | hi, n - 1 - j, j)
    i = np.where(lo, 0, np.where(hi, n - 1, i))
    lo, hi = j < 0, j >= n
    i = np.where(lo | hi, n - 1 - i, i)
    j = np.where(lo, 0, np.where(hi, n - 1, j))
    return i, j


def fetch(tex, i, j, touched=None):
    """T(i, j) of the (N, N, 3) image tex[row j, column i]; touched counts the fetches outside it, by edge."""
    n = tex.shape[0]
    i, j = np.asarray(i), np.asarray(j)
    if touched is not None:
        oi, oj = (i < 0) | (i >= n), (j < 0) | (j >= n)
        for k, m in (("left", (i < 0) & ~oj), ("right", (i >= n) & ~oj), ("top", (j < 0) & ~oi),
                     ("bottom", (j >= n) & ~oi), ("corner", oi & oj)):
            touched[k] = touched.get(k, 0) + int(np.count_nonzero(m))
    wi, wj = wrap(n, i, j)
    return tex[wj, wi]


def sgn(x):
    return np.where(x < 0, F(-1), F(1)).astype(F)


def coords(n, rot, d):
    """(valid, fx, fy) of directions d (..., 3): the continuous texel coordinates of the lookup."""
    d = np.asarray(d, F)
    r = np.asarray(rot, F).reshape(3, 3)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    with np.errstate(all="ignore"):
        e = [((r[k, 0] * dx).astype(F) + (r[k, 1] * dy).astype(F)).astype(F) + (r[k, 2] * dz).astype(F) for k in range(3)]
        ex, ey, ez = (v.astype(F) for v in e)
        s = ((np.abs(ex) + np.abs(ey)).astype(F) + np.abs(ez)).astype(F)
        valid = (s > 0) & (s < np.inf)
        ss = np.where(valid, s, F(1))
        a, b = (ex / ss).astype(F), (ey / ss).astype(F)
        fa = ((F(1) - np.abs(b)).astype(F) * sgn(a)).astype(F)
        fb = ((F(1) - np.abs(a)).astype(F) * sgn(b)).astype(F)
        low = ez < 0
        a, b = np.where(low, fa, a), np.where(low, fb, b)
        fn = F(n)
        fx = (((a * F(0.5)).astype(F) + F(0.5)).astype(F) * fn).astype(F) - F(0.5)
        fy = (((b * F(0.5)).astype(F) + F(0.5)).astype(F) * fn).astype(F) - F(0.5)
    return valid, np.where(valid, fx, F(0)).astype(F), np.where(valid, fy, F(0)).astype(F)


def lookup(tex, rot, d, touched=None):
    """M(d) for directions d (..., 3) of any length: (..., 3) float32."""
    tex = np.asarray(tex, F)
    n = tex.shape[0]
    assert tex.shape == (n, n, 3)
    valid, fx, fy = coords(n, rot, d)
    fi, fj = np.floor(fx), np.floor(fy)
    wx, wy = (fx - fi).astype(F)[..., None], (fy - fj).astype(F)[..., None]
    i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
    assert i0.min() >= -1 and i0.max() <= n - 1 and j0.min() >= -1 and j0.max() <= n - 1
    tt = None
    if touched is not None:  # count only the fetches of valid lookups
        tt = {}
    t00, t10 = fetch(tex, i0, j0, tt), fetch(tex, i0 + 1, j0, tt)
    t01, t11 = fetch(tex, i0, j0 + 1, tt), fetch(tex, i0 + 1, j0 + 1, tt)
    if touched is not None:
        for k, v in tt.items():
            touched[k] = touched.get(k, 0) + v
    ux, uy = (F(1) - wx).astype(F), (F(1) - wy).astype(F)
    top = ((ux * t00).astype(F) + (wx * t10).astype(F)).astype(F)
    bot = ((ux * t01).astype(F) + (wx * t11).astype(F)).astype(F)
    m = ((uy * top).astype(F) + (wy * bot).astype(F)).astype(F)
    return np.where(valid[..., None], m, F(0)).astype(F)


def with_env(p, env):
    q = type(p).from_buffer_copy(p)
    q.env[:] = list(env)
    return q


def escapes(osc, p, rows=None):
    """Per (sample, row, column) of the oracle scene (built WITHOUT emission) under
    p: escaped (bool), the escaping ray's direction d (3) and the throughput T (3)
    at the escape (the sample's L3 under env = 1: 0 + T 1 = T exactly)."""
    rows = [int(r) for r in (range(p.height) if rows is None else rows)]
    p1 = with_env(p, (1.0, 1.0, 1.0))
    shape = (p.spp, len(rows), p.width)
    esc, d, T = np.zeros(shape, bool), np.zeros(shape + (3,), F), np.zeros(shape + (3,), F)
    rays, ids = np.zeros((p.max_depth, 6), F), np.zeros(p.max_depth, np.int32)
    tuv, L = np.zeros((p.max_depth, 3), F), np.zeros(3, F)
    for r, y in enumerate(rows):
        for px in range(p.width):
            for s in range(p.spp):
                n = O.lib.oracle_trace_sample(osc.h, ctypes.byref(p1), px, y, s, rays.ctypes.data, ids.ctypes.data,
                                              tuv.ctypes.data, L.ctypes.data)
                if n > 0 and ids[n - 1] == -1:
                    esc[s, r, px] = True
                    d[s, r, px] = rays[n - 1, 3:6]
                    T[s, r, px] = L
                else:
                    assert not L.any()
    return esc, d, T


def emitted(osc_emit, p, rows=None):
    """L_emit per (sample, 3, row, column): L3 of the scene with emission under env = 0."""
    import accum_ref
    return accum_ref.contributions(osc_emit, with_env(p, (0.0, 0.0, 0.0)), rows)


def contributions(osc, p, tex, rot, osc_emit=None, rows=None, touched=None):
    """x[s] = L_emit + T (env M(d)), 0 for a path that neither escaped nor met an
    emitter: (spp, 3, rows, width) float32.  osc: the scene without emission;
    osc_emit: the same scene with it (None: no emitters)."""
    esc, d, T = escapes(osc, p, rows)
    env = np.array(list(p.env), F)
    m = lookup(tex, rot, d, touched=None)
    if touched is not None:
        lookup(tex, rot, d[esc], touched=touched)
    E = (env * m).astype(F)
    x = np.where(esc[..., None], (T * E).astype(F), F(0)).astype(F)      # (spp, rows, width, 3)
    x = np.ascontiguousarray(np.moveaxis(x, -1, 1))
    if osc_emit is not None:
        x = (emitted(osc_emit, p, rows) + x).astype(F)
    return x


def identity():
    return np.eye(3, dtype=F)


def rotation(axis, degrees):
    """A float32 rotation matrix about `axis` (Rodrigues, computed in f64, rounded once)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)).astype(F)


def random_map(n, seed, bright=3):
    """Random positive HDR texels, `bright` of them near 1e3."""
    rng = np.random.default_rng(seed)
    tex = rng.uniform(0.05, 4.0, size=(n, n, 3)).astype(F)
    for _ in range(min(bright, n * n)):
        tex[rng.integers(n), rng.integers(n)] = rng.uniform(500.0, 1500.0, size=3).astype(F)
    return tex


def texel_direction(n, i, j):
    """The (un-normalised, |x| + |y| + |z| = 1) direction of texel centre (i, j) in float64: the lookup's inverse."""
    a = (np.asarray(i, np.float64) + 0.5) / n * 2.0 - 1.0
    b = (np.asarray(j, np.float64) + 0.5) / n * 2.0 - 1.0
    z = 1.0 - np.abs(a) - np.abs(b)
    x = np.where(z < 0, (1.0 - np.abs(b)) * np.where(a < 0, -1.0, 1.0), a)
    y = np.where(z < 0, (1.0 - np.abs(a)) * np.where(b < 0, -1.0, 1.0), b)
    return x, y, z


def from_latlong(img, n):
    """spt_envmap_from_latlong in float64, rounded once: (H, W, 3) -> (n, n, 3) float32."""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    x, y, z = texel_direction(n, i, j)
    ln = np.sqrt(x * x + y * y + z * z)
    theta = np.arccos(np.clip(z / ln, -1.0, 1.0))
    phi = np.arctan2(y, x)
    phi = np.where(phi < 0, phi + 2.0 * np.pi, phi)
    fx, fy = phi / (2.0 * np.pi) * w - 0.5, theta / np.pi * h - 0.5
    x0f, y0f = np.floor(fx), np.floor(fy)
    dx, dy = (fx - x0f)[..., None], (fy - y0f)[..., None]
    x0 = np.mod(x0f.astype(np.int64), w)
    x1 = np.mod(x0 + 1, w)
    y0 = np.clip(y0f.astype(np.int64), 0, h - 1)
    y1 = np.clip(y0f.astype(np.int64) + 1, 0, h - 1)
    top = (1.0 - dx) * img[y0, x0] + dx * img[y0, x1]
    bot = (1.0 - dx) * img[y1, x0] + dx * img[y1, x1]
    return ((1.0 - dy) * top + dy * bot).astype(F)
