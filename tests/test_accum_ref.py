"""The CPU restatements behind the progressive-render tests, checked on their
own: accum_ref.moments over the oracle's per-sample contributions reproduces
oracle_render's film bit for bit (so sums and second moments can be held to the
oracle), its variance is a real signal and agrees with the f64 unbiased
variance of the mean; denoise_var_ref.atrous_var's f32 / f64 gap keeps the GPU
gate (8 x that gap) below 1e-3 x max|color| on heteroscedastic images, the
variance-guided filter beats the plain one at default sigmas there, and the
filtered variance never exceeds the input's."""
import numpy as np
import pytest

import accum_ref as A
import denoise_ref as R
import denoise_var_ref as V
import oracle as O
from sptamd import _lib, scenes

W, H, SPP, DEPTH = 12, 8, 6, 4
KW = dict(rr_start_depth=2, env=(0.3, 0.7, 1.0))
ALBEDO = np.array([[1.0, 1.0, 1.0], [0.8, 0.6, 0.4], [0.9, 0.3, 0.2], [0.2, 0.2, 0.8], [0.9, 0.9, 0.3],
                   [0.4, 0.4, 0.4]], np.float32)


def mode_scene(mode, mesh=None):
    """(mesh, albedo, emission) of a path mode: unit (every albedo 1), albedo, emit."""
    m = scenes.mitsuba_synth(detail=0.25) if mesh is None else mesh
    albedo = ALBEDO[: len(m["kd"])]
    if mode == "unit":
        return m, None, None
    if mode == "albedo":
        return m, albedo, None
    emi = np.zeros((len(albedo), 3), np.float32)
    emi[1] = (1.5, 0.5, 0.25)
    return m, albedo, emi


@pytest.mark.parametrize("mode", ["unit", "albedo", "emit"])
def test_moments_restatement_reproduces_the_oracle_film(mode):
    m, albedo, emi = mode_scene(mode)
    osc = O.OracleScene(m, albedo=albedo, emission=emi)
    p = O.reference_params(W, H, SPP, DEPTH, **KW)
    x = A.contributions(osc, p)
    s, q, film, var = A.moments(x)
    ref, _ = osc.render(p)
    np.testing.assert_array_equal(film, ref)
    # the variance is a signal, not zeros: on more than a quarter of the pixels
    # with albedos / emitters, and somewhere in unit mode (a pixel's samples all
    # escape or all do not, mostly)
    nz = int((var.max(axis=0) > 0).sum())
    print(f"{mode}: variance non-zero on {nz} of {W * H} pixels, max {float(var.max()):.4g}")
    assert nz >= 1 if mode == "unit" else nz > W * H // 4
    # and it is the unbiased variance of the mean, to f32 rounding of sums of magnitude q
    v64 = A.variance_f64(x)
    gap = float(np.abs(var.astype(np.float64) - v64).max())
    bound = 8.0 * np.finfo(np.float32).eps * float((q / np.float32(SPP)).max()) / (SPP - 1)
    print(f"{mode}: max |variance - f64| {gap:.3g} (bound {bound:.3g}), max variance {float(v64.max()):.4g}")
    assert gap <= bound
    # any split point gives the same sums (the running sum is just carried)
    s2, q2 = s * 0, q * 0
    for k in range(SPP):
        s2 = (s2 + x[k]).astype(np.float32)
        q2 = (q2 + (x[k] * x[k]).astype(np.float32)).astype(np.float32)
    np.testing.assert_array_equal(s2, s)
    np.testing.assert_array_equal(q2, q)


def test_moments_of_one_sample_have_zero_variance():
    x = np.full((1, 3, 2, 2), 0.5, np.float32)
    s, q, film, var = A.moments(x)
    assert np.all(var == 0) and np.all(film == 0.5) and np.all(q == 0.25)


def default_sigmas():
    p = _lib.default_denoise_var_params()
    return dict(sigma_variance=p.sigma_variance, sigma_normal=p.sigma_normal, sigma_albedo=p.sigma_albedo,
                sigma_depth=p.sigma_depth)


def filter_kw(d, iterations, **sig):
    return dict(color=d["color"], variance=d["variance"], normal=d["normal"], albedo=d["albedo"], depth=d["depth"],
                iterations=iterations, **dict(default_sigmas(), **sig))


SIZES = [(37, 19), (1, 1), (3, 70), (70, 3), (64, 48)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("iterations", [1, 2, 5, 8])
def test_filter_f32_gap_and_variance_bound(w, h, iterations):
    d = V.synthetic(seed=5, w=w, h=h)
    (tol_c, tol_v), (c64, v64) = V.tolerance(filter_kw(d, iterations))
    cap = 1e-3 * float(np.abs(d["color"]).max())
    print(f"{w} x {h} x {iterations}: colour gate {tol_c:.3e} (cap {cap:.3e}), variance gate {tol_v:.3e}")
    assert tol_c < cap
    v_in = V.v0(d["variance"])
    assert float(v64.max()) <= float(v_in.max())
    assert tol_v < 1e-3 * max(float(v_in.max()), 1e-30)
    assert np.isfinite(c64).all() and np.isfinite(v64).all()


@pytest.mark.parametrize("w,h", [(37, 19), (64, 48)])
def test_variance_guided_beats_plain_filter(w, h):
    d = V.synthetic(seed=5, w=w, h=h)
    guided, v = V.atrous_var(**filter_kw(d, 5))
    pd = _lib.default_denoise_params()
    plain = R.atrous(color=d["color"], normal=d["normal"], albedo=d["albedo"], depth=d["depth"], iterations=5,
                     sigma_color=pd.sigma_color, sigma_normal=pd.sigma_normal, sigma_albedo=pd.sigma_albedo,
                     sigma_depth=pd.sigma_depth)
    noisy, rp, rg = R.rmse(d["color"], d["clean"]), R.rmse(plain, d["clean"]), R.rmse(guided, d["clean"])
    print(f"{w} x {h}: rmse noisy {noisy:.4f}, plain {rp:.4f}, variance-guided {rg:.4f}")
    assert rg < rp < noisy
    # the converged sky stays exactly as it was, and the estimate of what is left shrank
    np.testing.assert_array_equal(guided[:, d["sky"]], d["clean"].astype(np.float64)[:, d["sky"]])
    assert float(v.max()) < float(V.v0(d["variance"]).max())


def test_zero_iterations_and_colour_term_off():
    d = V.synthetic(seed=5)
    c, v = V.atrous_var(**filter_kw(d, 0))
    np.testing.assert_array_equal(c, d["color"].astype(np.float64))
    np.testing.assert_array_equal(v, V.v0(d["variance"]))
    # sigma_variance <= 0: the colour term is off, the variance is still propagated
    c_off, v_off = V.atrous_var(**filter_kw(d, 3, sigma_variance=0.0))
    c_on, _ = V.atrous_var(**filter_kw(d, 3))
    assert not np.array_equal(c_off, c_on)
    assert float(v_off.max()) < float(V.v0(d["variance"]).max())
