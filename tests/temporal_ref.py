"""numpy restatement of spt_temporal_accumulate (include/spt.h: the temporal
accumulation of Schied et al. 2017), parametrised by dtype — float32 is the
contract, bit for bit; float64 the yardstick — and the analytic synthetic its
tests share.  Written from the header's steps 1-11, not from the kernel; the
camera constants C, C' are the library's own (spt_debug_camera_constants), so
the restatement starts from the numbers the device starts from.

Every operation below is one rounded operation in `dtype`, in the header's
order.  All pixels are evaluated at once; a tap that the definition does not
read is masked out (adding +0 to a sum that started at +0 leaves it as it is).
"""
import numpy as np

from sptamd import _lib, make_params

F = np.float32
SNAP = 1.0 / 64.0


def constants(camera: dict, width: int, height: int) -> dict:
    """The library's camera constants of a view (dict as sptamd.reference_camera)."""
    return _lib.camera_constants(make_params(width, height, 1, 1, camera=camera).camera, width, height)


def _v(t, T):
    return tuple(T(x) for x in t)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _to_local(C, w, T):
    return tuple(_dot(_v(C[k], T), w) for k in ("bx", "by", "bz"))


def _to_world(C, l, T):
    bx, by, bz = _v(C["bx"], T), _v(C["by"], T), _v(C["bz"], T)
    return tuple((bx[k] * l[0] + by[k] * l[1]) + bz[k] * l[2] for k in range(3))


def centre_dirs(C, width, height, dtype=F):
    """Step 2: camera_sample_dir(C, x, y, C.origin, 0.5, 0.5) for every pixel, three (H, W) arrays."""
    T = np.dtype(dtype).type
    px = np.broadcast_to(np.arange(width, dtype=dtype)[None, :], (height, width))
    py = np.broadcast_to(np.arange(height, dtype=dtype)[:, None], (height, width))
    o = _v(C["origin"], T)
    lens = _to_local(C, tuple(np.full((height, width), a - a, dtype) for a in o), T)
    ndc_x = (px + T(0.5)) / T(C["fw"])
    ndc_y = (py + T(0.5)) / T(C["fh"])
    fx = (T(0.5) - ndc_x) * (T(C["ratio"]) * T(C["film_y"]))
    fy = (T(0.5) - ndc_y) * T(C["film_y"])
    fz = T(C["dist_lens_to_film"])
    focal = ((T(C["focal_dist"]) * fx) / fz, (T(C["focal_dist"]) * fy) / fz, np.full((height, width), T(C["focal_z"]), dtype))
    v = tuple(focal[k] - lens[k] for k in range(3))
    inv = T(1) / np.sqrt(_dot(v, v))
    return _to_world(C, tuple(v[k] * inv for k in range(3)), T)


def accumulate(C, Cp, sum_, sum_sq, cur, prev=None, prev_guides=None, samples=1.0, max_history=64.0, sigma_depth=0.1,
               normal_min=0.9, dtype=F):
    """spt_temporal_accumulate.  C, Cp: constants() of the current and the
    previous view.  sum_, sum_sq: (3, H, W).  cur, prev_guides: dicts with
    "depth", "coverage" (H, W) and optionally "normal" (3, H, W).  prev: dict
    with "color", "moment2" (3, H, W) and "length" (H, W), or None.  Returns a
    dict with color, moment2, length, film, variance in `dtype`, and under
    "detail" what happened to each pixel: inside, snap_x, snap_y (bool), cand
    (taps read), valid, and the taps rejected by length / coverage / depth /
    normal (a tap is counted at the first test it fails, in the header's order)."""
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        return _accumulate(T, dtype, C, Cp, sum_, sum_sq, cur, prev, prev_guides, samples, max_history, sigma_depth,
                           normal_min)


def _accumulate(T, dtype, C, Cp, sum_, sum_sq, cur, prev, prev_guides, samples, max_history, sigma_depth, normal_min):
    s1 = np.asarray(sum_).astype(dtype)
    s2 = np.asarray(sum_sq).astype(dtype)
    H, W = s1.shape[1:]
    n = T(samples)
    assert (prev is None) == (prev_guides is None)
    zero = np.zeros((H, W), dtype)
    sw, hl = zero.copy(), zero.copy()
    hc, hm = np.zeros((3, H, W), dtype), np.zeros((3, H, W), dtype)
    detail = {k: np.zeros((H, W), np.int32) for k in ("cand", "valid", "rej_length", "rej_coverage", "rej_depth",
                                                         "rej_normal")}
    detail.update({k: np.zeros((H, W), bool) for k in ("inside", "snap_x", "snap_y", "surface")})
    if prev is not None:
        cov = np.asarray(cur["coverage"]).astype(dtype)
        dep = np.asarray(cur["depth"]).astype(dtype)
        surface = cov > 0                                                        # 1
        d = centre_dirs(C, W, H, dtype)                                          # 2
        o, op = _v(C["origin"], T), _v(Cp["origin"], T)
        z = dep / cov                                                            # 3
        X = tuple(o[k] + z * d[k] for k in range(3))
        vs = tuple(X[k] - op[k] for k in range(3))
        zexp = np.sqrt(_dot(vs, vs))
        v = tuple(np.where(surface, vs[k], d[k]) for k in range(3))
        l = _to_local(Cp, v, T)                                                  # 4
        dist = T(Cp["dist_lens_to_film"])
        fx = (l[0] * dist) / l[2]
        fy = (l[1] * dist) / l[2]
        ndx = T(0.5) - fx / (T(Cp["ratio"]) * T(Cp["film_y"]))
        ndy = T(0.5) - fy / T(Cp["film_y"])
        sx = ndx * T(W) - T(0.5)
        sy = ndy * T(H) - T(0.5)
        inside = (l[2] > 0) & np.isfinite(sx) & np.isfinite(sy) & (sx > -1) & (sx < T(W)) & (sy > -1) & (sy < T(H))
        rx, ry = np.rint(sx), np.rint(sy)                                        # 5
        snap_x = np.abs(sx - rx) <= T(SNAP)
        snap_y = np.abs(sy - ry) <= T(SNAP)
        sx = np.where(snap_x, rx, sx)
        sy = np.where(snap_y, ry, sy)
        x0, y0 = np.floor(sx), np.floor(sy)                                      # 6
        tx, ty = sx - x0, sy - y0
        ws = ((T(1) - tx) * (T(1) - ty), tx * (T(1) - ty), (T(1) - tx) * ty, tx * ty)
        x0i = np.where(inside, x0, 0).astype(np.int64)
        y0i = np.where(inside, y0, 0).astype(np.int64)
        pl = np.asarray(prev["length"]).astype(dtype)
        pc = np.asarray(prev["color"]).astype(dtype)
        pm = np.asarray(prev["moment2"]).astype(dtype)
        pcov = np.asarray(prev_guides["coverage"]).astype(dtype)
        pdep = np.asarray(prev_guides["depth"]).astype(dtype)
        normals = normal_min > -1 and cur.get("normal") is not None and prev_guides.get("normal") is not None
        if normals:
            cn = np.asarray(cur["normal"]).astype(dtype)
            pn = np.asarray(prev_guides["normal"]).astype(dtype)
            ncur = tuple(cn[k] / cov for k in range(3))
        for k in range(4):
            qx, qy = x0i + (k & 1), y0i + (k >> 1)
            w = ws[k]
            read = inside & (w != 0) & (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            jx, jy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            ln, cq = pl[jy, jx], pcov[jy, jx]                                    # 7
            ok_len = ln > 0
            ok_cov = np.where(surface, cq > 0, cq <= 0)
            ok_depth = np.ones((H, W), bool)
            ok_normal = np.ones((H, W), bool)
            if sigma_depth > 0:
                zq = pdep[jy, jx] / cq
                ok_depth = ~surface | (np.abs(zq - zexp) <= T(sigma_depth) * zexp)
            if normals:
                nq = tuple(pn[c][jy, jx] / cq for c in range(3))
                ok_normal = ~surface | (_dot(ncur, nq) >= T(normal_min))
            valid = read & ok_len & ok_cov & ok_depth & ok_normal
            detail["cand"] += read
            detail["valid"] += valid
            detail["rej_length"] += read & ~ok_len
            detail["rej_coverage"] += read & ok_len & ~ok_cov
            detail["rej_depth"] += read & ok_len & ok_cov & ~ok_depth
            detail["rej_normal"] += read & ok_len & ok_cov & ok_depth & ~ok_normal
            wv = np.where(valid, w, T(0))                                        # 8
            sw = sw + wv
            hl = hl + np.where(valid, w * ln, T(0))
            for c in range(3):
                hc[c] = hc[c] + np.where(valid, w * pc[c][jy, jx], T(0))
                hm[c] = hm[c] + np.where(valid, w * pm[c][jy, jx], T(0))
        detail.update(inside=inside, snap_x=inside & snap_x, snap_y=inside & snap_y, surface=surface)
    has = sw > 0
    hl = hl / sw
    hc = hc / sw
    hm = hm / sw
    m = s1 / n                                                                   # 9
    q = s2 / n
    Nh = np.where(has, np.fmin(hl, T(max_history)), T(0))                        # 10
    blend = Nh > 0
    N = np.where(blend, Nh + n, n)
    a = n / N
    color = np.where(blend, hc + a * (m - hc), m).astype(dtype)
    moment2 = np.where(blend, hm + a * (q - hm), q).astype(dtype)
    variance = np.where(N < 2, T(0), np.fmax(moment2 - color * color, T(0)) / (N - T(1))).astype(dtype)   # 11
    return {"color": color, "moment2": moment2, "length": N.astype(dtype), "film": color.copy(), "variance": variance,
            "detail": detail}


# ---------------------------------------------------------------- the synthetic
# A ground square, a box standing on it and a small sphere floating just in
# front of a wall, in front of the sky.  A camera that moves sideways uncovers
# ground far behind the box (another depth) and wall right behind the sphere's
# silhouette (the same depth within the tolerance, another normal).  From the
# pixel-centre rays of a camera: coverage, depth and normal as spt_render_aov
# writes them (premultiplied by a coverage of 1, 3/4 or 1/2 on the surfaces).
GROUND = 3.0                                     # the ground is y = 0, |x|, |z| <= GROUND
SPHERE = ((-0.8, 0.9, 0.0), 0.35)
BOXES = (((0.3, 0.0, -0.5), (1.3, 0.8, 0.5)), ((-1.8, 0.0, -0.6), (0.0, 1.6, -0.4)))   # the box, the wall
CAMERA_A = dict(look_from=(-1.0, 1.6, 5.0), look_at=(0.0, 0.7, 0.0), up=(0.0, 1.0, 0.0), lens_radius=0.0,
                focal_dist=1.0, fov_y=0.6981317, film_size_y=0.035)
CAMERA_B = dict(CAMERA_A, look_from=(1.0, 1.75, 4.8), look_at=(0.25, 0.6, 0.0))


def guides(camera: dict, width: int, height: int, seed: int = 0) -> dict:
    """The first-hit planes of the synthetic under `camera`: depth, coverage (H, W), normal (3, H, W), float32."""
    C = constants(camera, width, height)
    d = np.stack(centre_dirs(C, width, height, np.float64))
    o = np.array(C["origin"], np.float64)[:, None, None]
    t = np.full((height, width), np.inf)
    nrm = np.zeros((3, height, width))
    with np.errstate(all="ignore"):
        tg = -o[1] / d[1]                                                    # the ground
        p = o + tg * d
        hit = (tg > 0) & (np.abs(p[0]) <= GROUND) & (np.abs(p[2]) <= GROUND)
        t = np.where(hit, tg, t)
        nrm[1] = np.where(hit, 1.0, 0.0)
        c, r = np.array(SPHERE[0])[:, None, None], SPHERE[1]                 # the sphere
        oc = o - c
        b = (oc * d).sum(0)
        disc = b * b - ((oc * oc).sum(0) - r * r)
        ts = -b - np.sqrt(disc)
        hit = (disc > 0) & (ts > 0) & (ts < t)
        t = np.where(hit, ts, t)
        nrm = np.where(hit, ((o + ts * d) - c) / r, nrm)
        for blo, bhi in BOXES:                                               # the boxes (slabs)
            lo, hi = np.array(blo)[:, None, None], np.array(bhi)[:, None, None]
            t0, t1 = (lo - o) / d, (hi - o) / d
            tn, tf = np.minimum(t0, t1), np.maximum(t0, t1)
            tb, axis = tn.max(0), tn.argmax(0)
            hit = (tb < tf.min(0)) & (tb > 0) & (tb < t)
            t = np.where(hit, tb, t)
            bn = np.zeros_like(nrm)
            for k in range(3):
                bn[k] = np.where(axis == k, -np.sign(d[k]), 0.0)
            nrm = np.where(hit, bn, nrm)
    hit = np.isfinite(t)
    cov = np.where(hit, np.random.default_rng(seed).choice([1.0, 0.75, 0.5], size=t.shape), 0.0)
    return {"coverage": cov.astype(F), "depth": (np.where(hit, t, 0.0) * cov).astype(F),
            "normal": np.ascontiguousarray((nrm * cov).astype(F))}


def history(width: int, height: int, seed: int = 1) -> dict:
    """Random history planes: a colour in [0, 2), a second moment above its square, a length of 0 (one pixel in eight) .. 40."""
    rng = np.random.default_rng(seed)
    color = rng.random((3, height, width)) * 2.0
    moment2 = color * color + rng.random((3, height, width))
    length = np.where(rng.random((height, width)) < 0.125, 0.0, rng.integers(1, 41, (height, width)))
    return {"color": color.astype(F), "moment2": moment2.astype(F), "length": length.astype(F)}


def frame_sums(width: int, height: int, samples: int, seed: int = 2):
    """(sum, sum_sq) of `samples` random non-negative samples per pixel, float32, added in order."""
    rng = np.random.default_rng(seed)
    x = (rng.random((samples, 3, height, width)) * 1.5).astype(F)
    s, q = np.zeros(x.shape[1:], F), np.zeros(x.shape[1:], F)
    for k in range(samples):
        s = s + x[k]
        q = q + x[k] * x[k]
    return s, q


def synthetic(width: int, height: int, samples: int = 4, camera=None, prev_camera=None, seed: int = 0) -> dict:
    """Everything one moved-camera call needs: C, Cp, sum, sum_sq, cur, prev, prev_guides, samples."""
    camera = CAMERA_B if camera is None else camera
    prev_camera = CAMERA_A if prev_camera is None else prev_camera
    s, q = frame_sums(width, height, samples, seed + 2)
    return {"C": constants(camera, width, height), "Cp": constants(prev_camera, width, height), "sum": s, "sum_sq": q,
            "cur": guides(camera, width, height, seed), "prev": history(width, height, seed + 1),
            "prev_guides": guides(prev_camera, width, height, seed + 7), "samples": float(samples),
            "camera": camera, "prev_camera": prev_camera}


def call(d: dict, **kw) -> dict:
    """accumulate() on a synthetic()'s inputs; kw overrides parameters, prev=None drops the history."""
    args = dict(prev=d["prev"], prev_guides=d["prev_guides"], samples=d["samples"])
    args.update(kw)
    if args["prev"] is None:
        args["prev_guides"] = None
    return accumulate(d["C"], d["Cp"], d["sum"], d["sum_sq"], d["cur"], **args)


def classes(detail: dict) -> dict:
    """How many pixels fall in each class the moved-camera synthetic must hold."""
    D = detail
    surf, sky, cand = D["surface"], ~D["surface"], D["cand"]
    return {
        "snapped": int((D["snap_x"] | D["snap_y"]).sum()),
        "four_valid": int((D["valid"] == 4).sum()),
        "some_rejected": int(((D["valid"] > 0) & (D["valid"] < cand)).sum()),
        "all_rejected_by_depth": int((surf & (cand > 0) & (D["rej_depth"] == cand)).sum()),
        "all_rejected_by_normal": int((surf & (cand > 0) & (D["rej_normal"] == cand)).sum()),
        "off_screen": int((~D["inside"]).sum()),
        "sky_onto_sky": int((sky & (D["valid"] > 0)).sum()),
        "sky_onto_surface_rejected": int((sky & (D["rej_coverage"] > 0)).sum()),
    }
