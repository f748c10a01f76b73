"""The numpy restatement of spt_denoise's filter (tests/denoise_ref.py) on its
own, on the CPU: identity, constants, noise removal and edge preservation with
the library's default sigmas, and the f32-vs-f64 tolerance the GPU test
(test_gpu_denoise.py) gates on."""
import numpy as np
import pytest

import denoise_ref as R
from sptamd import _lib


def default_sigmas():
    p = _lib.default_denoise_params()
    return dict(sigma_color=p.sigma_color, sigma_normal=p.sigma_normal, sigma_albedo=p.sigma_albedo,
                sigma_depth=p.sigma_depth)


@pytest.fixture(scope="module")
def data():
    return R.synthetic()


def guided(d, **kw):
    return dict(color=d["color"], normal=d["normal"], albedo=d["albedo"], depth=d["depth"], **kw)


def test_inputs_are_what_they_claim(data):
    assert data["color"].shape == (3, R.HGT, R.W) == (3, 19, 37)
    assert data["sky"].any() and data["left"].any() and data["right"].any()
    for k in ("normal", "albedo"):
        assert np.all(data[k][:, data["sky"]] == 0)
    assert np.all(data["depth"][data["sky"]] == 0) and np.all(data["depth"][~data["sky"]] > 0)
    noise = data["color"].astype(np.float64) - data["clean"]
    assert 0.8 * R.NOISE_STD < noise.std() < 1.2 * R.NOISE_STD


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_iterations_is_the_identity(data, dtype):
    out = R.atrous(**guided(data, iterations=0, **default_sigmas()), dtype=dtype)
    np.testing.assert_array_equal(out, data["color"].astype(dtype))


def test_constant_colour_stays_constant(data):
    c = np.empty_like(data["color"])
    c[0], c[1], c[2] = 0.25, 0.5, 0.7
    out = R.atrous(**dict(guided(data, iterations=5, **default_sigmas()), color=c), dtype=np.float64)
    np.testing.assert_allclose(out, c.astype(np.float64), rtol=0, atol=1e-15)


def test_default_sigmas_remove_noise_and_keep_the_edge(data):
    out = R.atrous(**guided(data, iterations=5, **default_sigmas()), dtype=np.float64)
    noisy, clean = R.rmse(data["color"], data["clean"]), R.rmse(out, data["clean"])
    print(f"rmse to the clean signal: input {noisy:.5f}, filtered {clean:.5f}")
    assert clean < noisy
    # no bleeding: a side's mean moves toward the other side's by less than the
    # noise's standard error of that mean (per channel)
    for a, b in (("left", "right"), ("right", "left")):
        m, o = data[a], data[b]
        toward = np.sign(data["clean"][:, o].mean(1) - data["clean"][:, m].mean(1))
        move = (out[:, m].mean(1) - data["color"][:, m].astype(np.float64).mean(1)) * toward
        se = R.NOISE_STD / np.sqrt(m.sum())
        print(f"{a}: moved toward {b} by {move}, standard error {se:.5f}")
        assert np.all(move < se), (a, move, se)


@pytest.mark.parametrize("iterations", [1, 5])
def test_f32_restatement_is_well_conditioned(data, iterations):
    """tol = 8 x max|f32 - f64| must stay below 1e-3 x max(color): the inputs
    are such that the GPU gate cannot be widened by ill-conditioning."""
    tol, _ = R.tolerance(guided(data, iterations=iterations, **default_sigmas()))
    print(f"iterations {iterations}: tol {tol:.3e}")
    assert 0 < tol <= 1e-3 * float(data["color"].max())


def test_disabled_terms_and_missing_guides_agree(data):
    s = default_sigmas()
    a = R.atrous(data["color"], None, data["albedo"], data["depth"], 3, **s)
    b = R.atrous(data["color"], data["normal"], data["albedo"], data["depth"], 3, **dict(s, sigma_normal=0.0))
    np.testing.assert_array_equal(a, b)
    full = R.atrous(**guided(data, iterations=3, **s))
    assert not np.array_equal(a, full)
