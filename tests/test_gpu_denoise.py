"""spt_denoise (csrc/denoise.hip) against the numpy restatement of the filter
(tests/denoise_ref.py): |gpu - f64 restatement| <= tol with tol = 8 x
max|f32 restatement - f64 restatement|, computed here from the restatement
alone (test_denoise_ref.py bounds it by 1e-3 x max(color)); iterations = 0,
image borders (the step of 16 reaches past a 37 x 19 image), tiny and thin
images, each guide NULL in turn, writes outside `out`, and one end-to-end
render -> render_aov -> denoise."""
import ctypes

import numpy as np
import pytest
import torch

import denoise_ref as R
import sptamd
from sptamd import _lib, scenes

pytestmark = pytest.mark.gpu


def default_sigmas():
    p = _lib.default_denoise_params()
    return dict(sigma_color=p.sigma_color, sigma_normal=p.sigma_normal, sigma_albedo=p.sigma_albedo,
                sigma_depth=p.sigma_depth)


@pytest.fixture(scope="module")
def data():
    return R.synthetic()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def gpu(d, iterations, guides=("normal", "albedo", "depth"), **sig):
    aov = {k: dev(d[k]) for k in guides}
    out = sptamd.denoise(dev(d["color"]), aov, iterations=iterations, **sig)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(d, iterations, guides=("normal", "albedo", "depth"), **sig):
    kw = dict(color=d["color"], iterations=iterations, **dict(default_sigmas(), **sig))
    kw.update({k: d[k] for k in guides})
    tol, r64 = R.tolerance(kw)
    assert tol <= 1e-3 * float(np.abs(d["color"]).max())
    got = gpu(d, iterations, guides, **sig)
    err = float(np.abs(got.astype(np.float64) - r64).max())
    print(f"{d['color'].shape[1:]} x {iterations} iterations, guides {guides}: max |gpu - f64| {err:.3e}, tol {tol:.3e}")
    assert err <= tol, (err, tol)
    return got, r64


@pytest.mark.parametrize("iterations", [1, 2, 5, 8])
def test_matches_the_restatement(data, iterations):
    got, r64 = check(data, iterations)
    if iterations == 5:   # and it denoises: the restatement's own property, here on the device's output
        assert R.rmse(got, data["clean"]) < R.rmse(data["color"], data["clean"])


def test_zero_iterations_copies_bit_for_bit(data):
    np.testing.assert_array_equal(gpu(data, 0), data["color"])


@pytest.mark.parametrize("w,h", [(1, 1), (3, 70), (70, 3)])
def test_tiny_and_thin_images(w, h):
    check(R.synthetic(seed=9, w=w, h=h), 5)


@pytest.mark.parametrize("missing", ["normal", "albedo", "depth"])
def test_null_guide_disables_its_term(data, missing):
    guides = tuple(g for g in ("normal", "albedo", "depth") if g != missing)
    got, _ = check(data, 3, guides)
    # ... which is the restatement with that sigma switched off, and not the full filter
    off = R.atrous(**{k: data[k] for k in ("color", "normal", "albedo", "depth")}, iterations=3,
                   **dict(default_sigmas(), **{"sigma_" + missing: 0.0}))
    tol, _ = R.tolerance(dict(color=data["color"], iterations=3, **{k: data[k] for k in guides}, **default_sigmas()))
    assert float(np.abs(got - off).max()) <= tol


def test_no_guides_and_disabled_sigmas(data):
    check(data, 3, guides=())
    check(data, 3, sigma_color=0.0)
    check(data, 2, sigma_normal=-1.0, sigma_depth=0.0)


def test_writes_only_the_image(data):
    h, w = data["color"].shape[1:]
    pad = 64
    buf = torch.full((pad + 3 * h * w + pad,), -7.0, dtype=torch.float32, device="cuda")
    out = buf[pad:pad + 3 * h * w].view(3, h, w)
    aov = {k: dev(data[k]) for k in ("normal", "albedo", "depth")}
    for iterations in (0, 1, 4):
        buf.fill_(-7.0)
        res = sptamd.denoise(dev(data["color"]), aov, iterations=iterations, out=out)
        torch.cuda.synchronize()
        assert res.data_ptr() == out.data_ptr()
        assert torch.all(buf[:pad] == -7.0) and torch.all(buf[-pad:] == -7.0), iterations
        assert torch.all(out != -7.0)


def test_out_must_not_alias_color(data):
    c = dev(data["color"])
    with pytest.raises(sptamd.SptError):
        sptamd.denoise(c, None, out=c)
    torch.cuda.synchronize()


def test_render_aov_denoise_end_to_end():
    """mitsuba_synth 64 x 48 at 4 spp, 4 casts: the denoised film is nearer a
    256-spp render than the 4-spp film is.  (Checked on the CPU first, oracle
    renders through the f64 restatement: 0.0673 -> 0.0374.)"""
    s = sptamd.Scene()
    s.add_arrays(scenes.mitsuba_synth(detail=0.25))
    s.commit(0)
    p = sptamd.make_params(64, 48, 4, 4)
    film, _ = s.render(p)
    aov = s.render_aov(p)
    clean = sptamd.denoise(film, aov)
    ref, _ = s.render(sptamd.make_params(64, 48, 256, 4))
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    noisy, den = R.rmse(film.cpu().numpy(), ref), R.rmse(clean.cpu().numpy(), ref)
    print(f"rmse to 256 spp: 4 spp {noisy:.4f}, denoised {den:.4f}")
    assert den < noisy
    # the device's filter of the device's planes is the restatement's, to the same gate
    kw = dict(color=film.cpu().numpy(), normal=aov["normal"].cpu().numpy(), albedo=aov["albedo"].cpu().numpy(),
              depth=aov["depth"].cpu().numpy(), iterations=5, **default_sigmas())
    tol, r64 = R.tolerance(kw)
    assert float(np.abs(clean.cpu().numpy() - r64).max()) <= tol
