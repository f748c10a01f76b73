"""Multiple importance sampling without a GPU: the restatement
(tests/mis_ref.py) with the switch off is nee_ref and sky_ref bit for bit on their
own test scenes; the two weights of a direction both strategies can produce sum
to 1 within 4 ulp on 2 x 10^4 random configurations, and every degenerate case
gives its documented value; the restated estimator of a floor point under a
rectangular emitter converges to the form factor, and next to the emitter its
sample variance is below the light sampler's; the host program
tests/native/mis_check.cpp under ASan + UBSan — the SPT_HD weight functions and
the factored cx bit for bit against the restatement; the refusals that need no
device."""
import os
import shutil
import subprocess

import numpy as np

import envmap_ref as E
import mis_ref as M
import nee_ref as R
import oracle as O
import sky_ref as S
import sptamd
from sptamd import _lib, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallpt-enoki-optix_amd", "csrc")
F = np.float32
INV = _lib.SPT_ERR_INVALID
ULP = 2.0 ** -23
W, H, SPP, DEPTH = 37, 19, 8, 5
ROWS = (3, 9, 15)           # three rows of the GPU tests' render: every kind of vertex, a third of a second each
ROT = E.rotation((0.4, 1.0, -0.3), 63.0)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---- mis = False is nee_ref and sky_ref

def cornell():
    m = scenes.cornell_spheres(0.05)
    kd, ke = scenes.smallpt_materials(m)
    return m, kd, ke


def test_switch_off_reproduces_nee_ref_and_sky_ref():
    m, kd, ke = cornell()
    cam = scenes.cornell_camera()
    tex_n = E.random_map(8, seed=21)            # test_gpu_nee.py's map
    tex_s = E.random_map(8, 21, bright=0)       # test_gpu_sky.py's, with its sun
    tex_s[5, 5] = (1000.0, 800.0, 600.0)
    for env, sky in (((0.0, 0.0, 0.0), None), ((0.3, 0.7, 1.0), None), ((0.3, 0.7, 1.0), (tex_n, ROT))):
        p = O.reference_params(W, H, SPP, DEPTH, camera=cam, env=env, rr_start_depth=2)
        ca, cb = {}, {}
        a = R.contributions(m, p, kd, ke, sky=sky, rows=ROWS, count=ca)
        b = M.contributions(m, p, kd, ke, sky=sky, nee=True, rows=ROWS, count=cb)
        assert np.array_equal(bits(a), bits(b)) and ca["shadow_casts"] == cb["shadow_casts"] > 0, (env, sky is None)
        on = M.contributions(m, p, kd, ke, sky=sky, nee=True, mis=True, rows=ROWS, count=cb)
        assert not np.array_equal(on, a) and cb["weighted_hits"] > 0 and np.isfinite(on).all()
        off = M.contributions(m, p, kd, ke, sky=sky, rows=ROWS)
        assert np.array_equal(bits(off), bits(R.contributions(m, p, kd, ke, sky=sky, rows=ROWS, on=False)))
    p = O.reference_params(W, H, SPP, DEPTH, camera=cam, env=(1.0, 1.0, 1.0), rr_start_depth=2)
    for emission, nee, share in ((np.zeros_like(ke), False, 0.5), (ke, True, 0.5), (ke, True, 0.25), (ke, False, 0.5)):
        ca, cb = {}, {}
        a = S.contributions(m, p, kd, emission, (tex_s, ROT), nee=nee, share=share, rows=ROWS, count=ca)
        b = M.contributions(m, p, kd, emission, sky=(tex_s, ROT), nee=nee, sky_on=True, share=share, rows=ROWS, count=cb)
        assert np.array_equal(bits(a), bits(b)) and ca["shadow_casts"] == cb["shadow_casts"] > 0, (nee, share)
        on = M.contributions(m, p, kd, emission, sky=(tex_s, ROT), nee=nee, sky_on=True, share=share, mis=True, rows=ROWS,
                             count=cb)
        assert not np.array_equal(on, a) and cb["weighted_escapes"] > 0 and np.isfinite(on).all()
        assert (cb["weighted_hits"] > 0) == nee
    # mis with neither sampler: nothing to weigh
    a = M.contributions(m, p, kd, ke, sky=(tex_s, ROT), rows=ROWS)
    b = M.contributions(m, p, kd, ke, sky=(tex_s, ROT), mis=True, rows=ROWS)
    assert np.array_equal(bits(a), bits(b))


# ---- the two weights sum to 1

def random_normals(rng, n):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * rng.uniform(0.5, 1.0, size=(n, 1))).astype(F)       # shading normals of length 0.5 - 1


def test_the_two_weights_sum_to_one():
    """A configuration (x, n, light, d) or (n, d, sky) both strategies can produce: the shadow
    ray computes cx and c* at the vertex (r2 = 1 / rl^2), the bounce ray along the same d
    computes cb, and cl from its hit (t = 1, r2 = (t t)(d . d)): |w_shadow + w_bounce - 1| <= 4
    ulp(1) over 3 x 10^4 triangle and 2 x 10^4 sky configurations, normals of length 0.5 - 1, s = 1,
    1/4 and 3/4.

    A real bounce ray has another length, k d with t = 1 / k, rounded again, so its cb and cl
    differ from the vertex's by their own rounding; near grazing cx is a difference of
    products whose relative error has no bound in ulp.  That sum is printed, not asserted
    (seen: 7 ulp on the triangles, 105 ulp on the sky's grazing directions, 1e-5 relative)."""
    rng = np.random.default_rng(16)
    n = 10000
    soup = rng.uniform(-1, 1, size=(40, 9)).astype(F)
    table = R.light_table(soup, rng.integers(0, 2, size=40), np.array([[0, 0, 0], [3, 1, 2]], F))
    ids, cdf, pdf, tv, ng, le = table
    assert len(ids) > 10
    worst = scaled = 0.0
    for s in (F(1), F(0.25), (F(1) - F(0.25)).astype(F)):
        i = rng.integers(0, len(ids), size=n)
        b = rng.dirichlet((1, 1, 1), size=n)
        y = (b[:, :1] * tv[i, 0:3] + b[:, 1:2] * tv[i, 3:6] + b[:, 2:] * tv[i, 6:9]).astype(F)
        x = rng.uniform(-2, 2, size=(n, 3)).astype(F)
        nh = random_normals(rng, n)
        d = (y - x).astype(F)
        rl = M.inv_len(d)
        cx = M.bounce_cx(nh, d, rl)
        cy = (np.abs(R.dot(ng[i], d)) * rl).astype(F)
        ok = (cx > 0) & (cy > 0)                      # what the light sampler accepts
        assert ok.sum() > n // 4
        ws = M.shadow_weight(cx, (s * M.light_cl(pdf[i], (F(1) / (rl * rl).astype(F)).astype(F), cy)).astype(F))
        wb = M.light_hit_weight(cx, s, ng[i], pdf[i], d, np.ones(n, F))
        err = np.abs((ws.astype(np.float64) + wb.astype(np.float64)) - 1.0)[ok]
        worst = max(worst, err.max() / ULP)
        assert np.all((ws[ok] > 0) & (ws[ok] < 1) & (wb[ok] > 0) & (wb[ok] < 1))
        # and what it refuses counts in full at the hit where the refusal is the edge-on test
        assert np.all(wb[~(cy > 0)] == 1)
        k = rng.uniform(0.5, 2.0, size=n).astype(F)
        db = (d * k[:, None]).astype(F)
        wk = M.light_hit_weight(M.bounce_cx(nh, db, M.inv_len(db)), s, ng[i], pdf[i], db, (F(1) / k).astype(F))
        scaled = max(scaled, (np.abs((ws.astype(np.float64) + wk.astype(np.float64)) - 1.0)[ok]).max() / ULP)
    print(f"triangles: worst |w_shadow + w_bounce - 1| = {worst:.2f} ulp, with a rescaled bounce ray {scaled:.2f} ulp")
    assert worst <= 4.0
    tex = E.random_map(8, 3)
    rot = E.rotation((0.3, 1.0, -0.2), 37.0)
    stab = S.sky_table(tex)
    worst = scaled = 0.0
    for s in (F(1), F(0.25)):
        d = rng.normal(size=(n, 3)).astype(F)
        nh = random_normals(rng, n)
        cx = M.bounce_cx(nh, d, M.inv_len(d))
        pdfs = S.sky_pdf(stab, rot, d)
        ok = (cx > 0) & (pdfs > 0)
        assert ok.sum() > n // 4
        ws = M.shadow_weight(cx, (s * (M.PI * pdfs).astype(F)).astype(F))
        wb = M.escape_weight(cx, s, pdfs)
        err = np.abs((ws.astype(np.float64) + wb.astype(np.float64)) - 1.0)[ok]
        worst = max(worst, err.max() / ULP)
        assert np.all((ws[ok] > 0) & (ws[ok] < 1) & (wb[ok] > 0) & (wb[ok] < 1))
        k = rng.uniform(0.5, 2.0, size=n).astype(F)
        db = (d * k[:, None]).astype(F)
        pdfb = S.sky_pdf(stab, rot, db)
        sel = ok & (np.abs(pdfb.astype(np.float64) / np.where(ok, pdfs, 1) - 1) < 1e-5)   # (k d may round into the next cell)
        assert sel.sum() > 0.95 * ok.sum()
        wk = M.escape_weight(M.bounce_cx(nh, db, M.inv_len(db)), s, pdfb)
        scaled = max(scaled, (np.abs((ws.astype(np.float64) + wk.astype(np.float64)) - 1.0)[sel]).max() / ULP)
    print(f"sky: worst |w_shadow + w_bounce - 1| = {worst:.2f} ulp, with a rescaled bounce ray {scaled:.2f} ulp")
    assert worst <= 4.0


def test_degenerate_weights_are_the_documented_values():
    inf, nan = F(np.inf), F(np.nan)
    one, zero = F(1), F(0)
    ng, d, t = np.array([0, 1, 0], F), np.array([0.3, 0.8, -0.1], F), F(2)
    # cb = 0, negative, NaN: the shadow sampler refuses cx <= 0 — the hit counts in full
    for cb in (zero, F(-0.5), nan):
        assert M.bounce_weight(cb, F(2)) == 1 and M.shadow_weight(cb, F(2)) == 0
        assert M.light_hit_weight(cb, one, ng, F(3), d, t) == 1 and M.escape_weight(cb, one, F(0.2)) == 1
    # the sampler's density zero, negative or NaN: it cannot produce the direction
    for sb in (zero, F(-1), nan):
        assert M.bounce_weight(F(0.5), sb) == 1 and M.shadow_weight(F(0.5), sb) == 0
        assert M.shadow_factor(F(0.5), sb) == inf                   # "g < inf" fails: no shadow ray
    assert M.escape_weight(F(0.5), one, zero) == 1 and M.escape_weight(F(0.5), F(0.25), nan) == 1
    # pdfA = 0 (a member of weight 0) and cy = 0 (edge-on, or a member without a normal)
    assert M.light_hit_weight(F(0.5), one, ng, zero, d, t) == 1
    assert M.light_hit_weight(F(0.5), one, ng, F(3), np.array([1, 0, 0], F), t) == 1
    assert M.light_hit_weight(F(0.5), one, np.zeros(3, F), zero, d, t) == 1
    assert M.light_hit_weight(F(0.5), one, np.zeros(3, F), F(3), d, t) == 1
    # a sum that is not finite: the sampler's weight is 1, the hit's 0, the shadow factor 0 (c = 0: not traced)
    for c, sb in ((F(0.5), inf), (F(3e38), F(3e38))):
        assert M.bounce_weight(c, sb) == 0 and M.shadow_weight(c, sb) == 1 and M.shadow_factor(c, sb) == 0
    assert M.light_hit_weight(F(0.5), one, ng, F(3e38), d, F(1e10)) == 0
    assert M.light_cl(F(3), F(4), zero) == inf and np.isnan(M.light_cl(zero, F(4), zero))
    # an ordinary pair, and s = 1 against s = 1/4
    assert M.bounce_weight(F(1), F(3)) == F(0.25) and M.shadow_weight(F(1), F(3)) == F(0.75) and M.shadow_factor(F(1), F(3)) == F(0.25)
    assert M.escape_weight(F(0.5), F(0.25), F(0.2)) > M.escape_weight(F(0.5), one, F(0.2))


# ---- the closed form

def quad(y, x0, x1, z0, z1):
    return np.array([[x0, y, z0, x1, y, z0, x1, y, z1], [x0, y, z0, x1, y, z1, x0, y, z1]], F)


def form_factor(h, x0, x1, z0, z1):
    def corner(a, b):
        X, Y = abs(a) / h, abs(b) / h
        f = (X / np.sqrt(1 + X * X) * np.arctan(Y / np.sqrt(1 + X * X))
             + Y / np.sqrt(1 + Y * Y) * np.arctan(X / np.sqrt(1 + Y * Y))) / (2 * np.pi)
        return f * np.sign(a) * np.sign(b)
    return corner(x1, z1) - corner(x0, z1) - corner(x1, z0) + corner(x0, z0)


def estimators(h, seed):
    """Per sample, red channel: (the light sampler's c, the MIS estimator's shadow part + bounce part)
    of the floor point 0 under the rectangle at height h, Le = 12."""
    x0, x1, z0, z1 = -0.3, 0.5, -0.2, 0.45
    le = np.array([[0, 0, 0], [12, 6, 3]], F)
    table = R.light_table(quad(h, x0, x1, z0, z1), np.array([1, 1]), le)
    n = 1 << 16
    rng = np.random.default_rng(seed)
    xi = rng.random((3, n)).astype(F)
    x = np.zeros((n, 3), F)
    nh = np.tile(np.array([0, 1, 0], F), (n, 1))
    one = np.ones((n, 3), F)
    plain = R.light_sample(table, x, nh, one, *xi)[4][:, 0].astype(np.float64)
    shadow = M.light_sample(table, x, nh, one, *xi, F(1))[4][:, 0].astype(np.float64)
    # the bounce ray: cosine-distributed about +y, met by the plane y = h
    u1, u2 = rng.random(n), rng.random(n)
    r, ph = np.sqrt(u1), 2 * np.pi * u2
    d = np.stack([r * np.cos(ph), np.sqrt(1 - u1), r * np.sin(ph)], axis=1).astype(F)
    with np.errstate(all="ignore"):
        t = (F(h) / d[:, 1]).astype(F)
    px, pz = t * d[:, 0], t * d[:, 2]
    hit = (d[:, 1] > 0) & (px >= x0) & (px <= x1) & (pz >= z0) & (pz <= z1)
    cb = M.bounce_cx(nh, d, M.inv_len(d))
    w = M.light_hit_weight(cb, F(1), np.tile(table[4][0], (n, 1)), np.full(n, table[2][0], F), d, t)
    bounce = np.where(hit, 12.0 * w.astype(np.float64), 0.0)
    return plain, shadow + bounce, 12.0 * form_factor(h, x0, x1, z0, z1), hit.mean()


def test_restated_mis_estimator_converges_to_the_form_factor():
    for h in (0.8, 0.05):
        plain, mis, want, hits = estimators(h, 11)
        n = len(mis)
        z = (mis.mean() - want) / (mis.std(ddof=1) / np.sqrt(n))
        zp = (plain.mean() - want) / (plain.std(ddof=1) / np.sqrt(n))
        print(f"h = {h}: Le F = {want:.5f}, MIS mean {mis.mean():.5f} z {z:+.2f} variance {mis.var(ddof=1):.4g}; light sampling "
              f"alone mean {plain.mean():.5f} z {zp:+.2f} variance {plain.var(ddof=1):.4g}; {hits:.3f} of the bounce rays hit")
        assert abs(z) <= 4
        if h == 0.05:       # the near light: the area sampler's weight is unbounded, the balance heuristic's is not
            assert mis.var(ddof=1) < plain.var(ddof=1)
            assert mis.max() <= 2 * 12.0 * (1 + 1e-6) < plain.max()     # each of the two parts is at most Le


# ---- the host program under the sanitizers

def _build(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "mis_check"
    root = os.environ.get("ROCM_PATH", "/opt/rocm")   # spt_math.h includes the HIP runtime header for its markers
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(root, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "mis_check.cpp")], check=True, capture_output=True)
    return exe


def _run(exe, mode, rows, tmp_path):
    path = tmp_path / (mode + ".f32")
    np.ascontiguousarray(rows, F).tofile(path)
    run = subprocess.run([str(exe), mode, str(path)], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    out = np.array([[int(v, 16) for v in line.split()] for line in run.stdout.strip().split("\n")], np.uint32)
    assert len(out) == len(rows)
    return out.view(F)


def test_host_program_equals_the_restatement(tmp_path):
    exe = _build(tmp_path)
    rng = np.random.default_rng(7)
    n = 2000
    special = np.array([0, -0.0, 1, -1, 0.5, 3e38, 1e-38, 1e-45, np.inf, -np.inf, np.nan, 3.4028235e38], F)
    # cx: random normals of every length, axis-aligned ones (the frame's sign branch), zero vectors
    nh = np.concatenate([random_normals(rng, n), np.array([[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, -1], [0, 0, 0], [0, -0.0, 1]], F)])
    d = np.concatenate([(rng.normal(size=(n, 3)) * rng.uniform(0.01, 30, size=(n, 1))).astype(F),
                        np.array([[0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 0, 0], [1, 1, 1], [1e-20, 0, 0]], F)])
    got = _run(exe, "cx", np.concatenate([nh, d], axis=1), tmp_path)[:, 0]
    assert same_bits(got, M.bounce_cx(nh, d, M.inv_len(d)))
    # and the factored helper is the expression nee_ref / sky_ref restate
    ok = np.isfinite(got)
    assert ok.sum() > n
    # pairs and cl: random positive values over many binades, and every pair of special values
    sp = np.array([(a, b) for a in special for b in special], F)
    pairs = np.concatenate([np.exp(rng.uniform(-60, 60, size=(n, 2))).astype(F), sp])
    got = _run(exe, "pair", pairs, tmp_path)
    assert same_bits(got[:, 0], M.shadow_factor(pairs[:, 0], pairs[:, 1]))
    assert same_bits(got[:, 1], M.bounce_weight(pairs[:, 0], pairs[:, 1]))
    assert not np.isnan(got[:, 1]).any()                        # a weight is a number whatever comes in
    sp3 = np.array([(a, b, c) for a in special for b in special for c in special], F)
    cl = np.concatenate([np.exp(rng.uniform(-30, 30, size=(n, 3))).astype(F), sp3])
    assert same_bits(_run(exe, "cl", cl, tmp_path)[:, 0], M.light_cl(cl[:, 0], cl[:, 1], cl[:, 2]))
    got = _run(exe, "escape", cl, tmp_path)[:, 0]
    assert same_bits(got, M.escape_weight(cl[:, 0], cl[:, 1], cl[:, 2])) and not np.isnan(got).any()
    # hits: cb s ng pdfA d t, with special values in every scalar column
    m = n + len(special) * 4
    rows = np.zeros((m, 10), F)
    rows[:, 0] = np.exp(rng.uniform(-20, 5, size=m))
    rows[:, 1] = rng.choice(np.array([1, 0.25, 0.75, 0.5], F), size=m)
    v = rng.normal(size=(m, 3))
    rows[:, 2:5] = v / np.linalg.norm(v, axis=1, keepdims=True)
    rows[:, 5] = np.exp(rng.uniform(-10, 10, size=m))
    rows[:, 6:9] = rng.normal(size=(m, 3)) * rng.uniform(0.1, 10, size=(m, 1))
    rows[:, 9] = np.exp(rng.uniform(-8, 8, size=m))
    for c, col in enumerate((0, 1, 5, 9)):
        rows[n + c * len(special): n + (c + 1) * len(special), col] = special
    rows[5, 2:5] = 0                                            # a member without a normal
    rows[6, 6:9] = np.cross(rows[6, 2:5], [1, 0, 0])            # nearly edge-on
    got = _run(exe, "hit", rows, tmp_path)[:, 0]
    want = M.light_hit_weight(rows[:, 0], rows[:, 1], rows[:, 2:5], rows[:, 5], rows[:, 6:9], rows[:, 9])
    assert same_bits(got, want) and not np.isnan(got).any()
    assert np.all((got >= 0) & (got <= 1))


# ---- the refusals that need no device

def test_refusals_need_no_device():
    L = _lib.lib
    for name in ("spt_scene_set_mis", "spt_scene_get_mis"):
        assert name in _lib.EXPORTED and hasattr(L, name), name
    assert L.spt_scene_set_mis(None, 1) == INV and b"NULL scene" in L.spt_last_error()
    fake = 0x1000    # never dereferenced: refused first
    assert L.spt_scene_set_mis(fake, 2) == INV and b"on = 2" in L.spt_last_error()
    assert L.spt_scene_get_mis(None, None) == INV
    assert callable(sptamd.HipBackend.set_mis) and callable(sptamd.HipBackend.mis)
