"""spt_denoise_var (csrc/denoise.hip) against the numpy restatement of the
filter (tests/denoise_var_ref.py): |gpu - f64 restatement| <= tol with tol =
8 x max|f32 restatement - f64 restatement| for the colour and for the variance
plane, computed here from the restatement alone (test_accum_ref.py bounds the
colour's by 1e-3 x max|color|); iterations = 0, image borders, tiny and thin
images, each guide NULL in turn, the colour term switched off, writes outside
the outputs, aliasing, and one end-to-end progressive render -> render_aov ->
denoise_var."""
import ctypes

import numpy as np
import pytest
import torch

import denoise_ref as R
import denoise_var_ref as V
import sptamd
from sptamd import _lib, scenes

pytestmark = pytest.mark.gpu
GUIDES = ("normal", "albedo", "depth")


def default_sigmas():
    p = _lib.default_denoise_var_params()
    return dict(sigma_variance=p.sigma_variance, sigma_normal=p.sigma_normal, sigma_albedo=p.sigma_albedo,
                sigma_depth=p.sigma_depth)


@pytest.fixture(scope="module")
def data():
    return V.synthetic()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def gpu(d, iterations, guides=GUIDES, **sig):
    aov = {k: dev(d[k]) for k in guides}
    out, vout = sptamd.denoise_var(dev(d["color"]), dev(d["variance"]), aov, iterations=iterations,
                                   return_variance=True, **sig)
    torch.cuda.synchronize()
    return out.cpu().numpy(), vout.cpu().numpy()


def check(d, iterations, guides=GUIDES, **sig):
    kw = dict(color=d["color"], variance=d["variance"], iterations=iterations, **dict(default_sigmas(), **sig))
    kw.update({k: d[k] for k in guides})
    (tol_c, tol_v), (c64, v64) = V.tolerance(kw)
    assert tol_c <= 1e-3 * float(np.abs(d["color"]).max())
    got, vgot = gpu(d, iterations, guides, **sig)
    err_c = float(np.abs(got.astype(np.float64) - c64).max())
    err_v = float(np.abs(vgot.astype(np.float64) - v64).max())
    print(f"{d['color'].shape[1:]} x {iterations} iterations, guides {guides}: colour max |gpu - f64| {err_c:.3e} "
          f"(tol {tol_c:.3e}), variance {err_v:.3e} (tol {tol_v:.3e})")
    assert err_c <= tol_c, (err_c, tol_c)
    assert err_v <= tol_v, (err_v, tol_v)
    return got, vgot, c64, v64


@pytest.mark.parametrize("iterations", [1, 2, 5, 8])
def test_matches_the_restatement(data, iterations):
    got, vgot, _, _ = check(data, iterations)
    assert float(vgot.max()) <= float(V.v0(data["variance"], np.float32).max())
    if iterations == 5:   # and it denoises, better than the plain filter does at its default sigmas
        plain = sptamd.denoise(dev(data["color"]), {k: dev(data[k]) for k in GUIDES})
        torch.cuda.synchronize()
        noisy, rp, rg = (R.rmse(x, data["clean"]) for x in (data["color"], plain.cpu().numpy(), got))
        print(f"rmse: noisy {noisy:.4f}, plain {rp:.4f}, variance-guided {rg:.4f}")
        assert rg < rp < noisy
        np.testing.assert_array_equal(got[:, data["sky"]], data["clean"][:, data["sky"]])   # converged: untouched


def test_zero_iterations_copies_bit_for_bit(data):
    got, vgot = gpu(data, 0)
    np.testing.assert_array_equal(got, data["color"])
    np.testing.assert_array_equal(vgot, V.v0(data["variance"], np.float32))
    neg = dict(data, variance=-data["variance"])          # v_0 clamps at 0
    _, vneg = gpu(neg, 0)
    assert (vneg == 0).all()


@pytest.mark.parametrize("w,h", [(1, 1), (3, 70), (70, 3), (64, 48)])
def test_tiny_thin_and_multi_block_images(w, h):
    check(V.synthetic(seed=9, w=w, h=h), 5)


@pytest.mark.parametrize("missing", GUIDES)
def test_null_guide_disables_its_term(data, missing):
    guides = tuple(g for g in GUIDES if g != missing)
    got, _, _, _ = check(data, 3, guides)
    # ... which is the restatement with that sigma switched off
    off, _ = V.atrous_var(**{k: data[k] for k in ("color", "variance") + GUIDES}, iterations=3,
                          **dict(default_sigmas(), **{"sigma_" + missing: 0.0}))
    (tol, _), _ = V.tolerance(dict(color=data["color"], variance=data["variance"], iterations=3,
                                   **{k: data[k] for k in guides}, **default_sigmas()))
    assert float(np.abs(got - off).max()) <= tol


def test_colour_term_off_and_other_switches(data):
    _, vgot, _, _ = check(data, 3, sigma_variance=0.0)          # the variance is still propagated
    assert float(vgot.max()) < float(V.v0(data["variance"], np.float32).max())
    check(data, 3, sigma_variance=-1.0, guides=())
    check(data, 3, guides=())
    check(data, 2, sigma_normal=-1.0, sigma_depth=0.0)
    check(data, 2, sigma_variance=1.0)


def test_writes_only_the_outputs(data):
    h, w = data["color"].shape[1:]
    pad, n = 64, 3 * h * w
    buf = torch.full((pad + n + pad + h * w + pad,), -7.0, dtype=torch.float32, device="cuda")
    out = buf[pad:pad + n].view(3, h, w)
    vout = buf[pad + n + pad:pad + n + pad + h * w]
    aov = {k: dev(data[k]) for k in GUIDES}
    color, var = dev(data["color"]), dev(data["variance"])
    scratch = torch.empty(_lib.lib.spt_denoise_var_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    guides = sptamd.aov_struct(aov)
    for iterations in (0, 1, 4):
        for want_v in (True, False):
            buf.fill_(-7.0)
            p = _lib.default_denoise_var_params()
            p.width, p.height, p.iterations = w, h, iterations
            _lib.check(_lib.lib.spt_denoise_var(ctypes.byref(p), color.data_ptr(), var.data_ptr(), ctypes.byref(guides),
                                                out.data_ptr(), vout.data_ptr() if want_v else None,
                                                scratch.data_ptr(), None), "spt_denoise_var")
            torch.cuda.synchronize()
            guard = torch.cat([buf[:pad], buf[pad + n:pad + n + pad], buf[-pad:]])
            assert torch.all(guard == -7.0), (iterations, want_v)
            assert torch.all(out != -7.0)
            assert torch.all(vout != -7.0) if want_v else torch.all(vout == -7.0)


def test_out_must_not_alias_an_input(data):
    c, v = dev(data["color"]), dev(data["variance"])
    with pytest.raises(sptamd.SptError):
        sptamd.denoise_var(c, v, None, out=c)
    with pytest.raises(sptamd.SptError):
        sptamd.denoise_var(c, v, None, out=v)
    torch.cuda.synchronize()


def test_progressive_render_aov_denoise_var_end_to_end():
    """mitsuba_synth 64 x 48, 8 spp as two passes of 4, 4 casts: denoise_var of
    the accumulated film with the accumulator's variance is nearer a 256-spp
    render than the film is; the plain denoise is printed beside it, not gated.
    (Checked on the CPU first through the oracle's per-sample contributions and
    the f64 restatement, with depth and albedo guides: rmse 0.0496 -> 0.0229 at
    sigma_variance 4; 0.0437 / 0.0288 / 0.0228 at 1 / 2 / 8; the plain filter 0.0244.)"""
    s = sptamd.Scene()
    s.add_arrays(scenes.mitsuba_synth(detail=0.25))
    s.commit(0)
    p = sptamd.make_params(64, 48, 8, 4)
    acc = s.accumulator(p)
    acc.add(4)
    acc.add(4)
    aov = s.render_aov(p)
    clean, vout = sptamd.denoise_var(acc.film, acc.variance, aov, return_variance=True)
    plain = sptamd.denoise(acc.film, aov)
    ref, _ = s.render(sptamd.make_params(64, 48, 256, 4))
    film8, _ = s.render(p)
    torch.cuda.synchronize()
    film = acc.film.cpu().numpy()
    np.testing.assert_array_equal(film, film8.cpu().numpy())
    ref = ref.cpu().numpy()
    noisy, den, pl = R.rmse(film, ref), R.rmse(clean.cpu().numpy(), ref), R.rmse(plain.cpu().numpy(), ref)
    print(f"rmse to 256 spp: 8 spp {noisy:.4f}, denoise_var {den:.4f}, plain denoise {pl:.4f}")
    assert den < noisy
    # the device's filter of the device's planes is the restatement's, to the same gate
    kw = dict(color=film, variance=acc.variance.cpu().numpy(), normal=aov["normal"].cpu().numpy(),
              albedo=aov["albedo"].cpu().numpy(), depth=aov["depth"].cpu().numpy(), iterations=5, **default_sigmas())
    (tol_c, tol_v), (c64, v64) = V.tolerance(kw)
    assert float(np.abs(clean.cpu().numpy() - c64).max()) <= tol_c
    assert float(np.abs(vout.cpu().numpy() - v64).max()) <= tol_v
