"""Properties of the numpy restatement of spt_temporal_accumulate alone
(tests/temporal_ref.py; no GPU): what the definition of include/spt.h promises
whatever computes it, and that the moved-camera synthetic the GPU comparison
uses holds every class of pixel, so that comparison cannot be vacuous."""
import numpy as np
import pytest

import temporal_ref as R

F = np.float32
INF = float("inf")
SIZES = [(64, 48), (70, 50)]


@pytest.mark.parametrize("w,h", SIZES + [(1, 1), (3, 70), (1920, 1080)])
def test_identity_camera_reads_exactly_its_own_pixel(w, h):
    d = R.synthetic(w, h, camera=R.CAMERA_A, prev_camera=R.CAMERA_A)
    d["prev_guides"] = d["cur"]          # the same view saw the same surfaces
    r = R.call(d, max_history=INF)
    D = r["detail"]
    assert D["inside"].all() and D["snap_x"].all() and D["snap_y"].all()
    assert (D["cand"] == 1).all()        # one tap of weight 1: the pixel itself
    has = d["prev"]["length"] > 0
    np.testing.assert_array_equal(D["valid"] == 1, has)
    n = F(d["samples"])
    np.testing.assert_array_equal(r["length"], np.where(has, d["prev"]["length"] + n, n))
    # weight 1 on itself: hc is the pixel's own history, bit for bit
    m = d["sum"] / n
    a = n / r["length"]
    hc = d["prev"]["color"]
    np.testing.assert_array_equal(r["color"], np.where(has, hc + a * (m - hc), m))


def test_still_camera_accumulates_every_frame():
    w, h, n, K = 70, 50, 4, 6
    C = R.constants(R.CAMERA_A, w, h)
    g = R.guides(R.CAMERA_A, w, h)
    sums = [R.frame_sums(w, h, n, seed=100 + k) for k in range(K)]
    out = {}
    for dtype in (np.float32, np.float64):
        prev = None
        for s, q in sums:
            prev = R.accumulate(C, C, s, q, g, prev=prev, prev_guides=None if prev is None else g, samples=n,
                                max_history=INF, dtype=dtype)
        out[dtype] = prev
    f32, f64 = out[np.float32], out[np.float64]
    assert f32["color"].dtype == np.float32
    np.testing.assert_array_equal(f32["length"], np.full((h, w), K * n, F))
    mean = sum(s.astype(np.float64) for s, _ in sums) / (K * n)
    np.testing.assert_allclose(f64["film"], mean, rtol=0, atol=1e-13)
    tol = 8.0 * float(np.abs(f32["film"].astype(np.float64) - f64["film"]).max())   # denoise_ref.tolerance's factor
    assert 0 < tol < 1e-5
    assert float(np.abs(f32["film"].astype(np.float64) - mean).max()) <= tol
    # the second moment is the mean of the frames' too, and the variance follows spt_render_accum's formula
    mean_q = sum(q.astype(np.float64) for _, q in sums) / (K * n)
    np.testing.assert_allclose(f64["moment2"], mean_q, rtol=0, atol=1e-12)
    np.testing.assert_allclose(f64["variance"], np.maximum(mean_q - mean * mean, 0) / (K * n - 1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("w,h", SIZES)
def test_no_history_returns_the_frames_own_samples(w, h):
    d = R.synthetic(w, h)
    n = F(d["samples"])
    m, q = d["sum"] / n, d["sum_sq"] / n
    for r in (R.call(d, max_history=0.0), R.call(d, prev=None)):
        np.testing.assert_array_equal(r["color"], m)
        np.testing.assert_array_equal(r["film"], m)
        np.testing.assert_array_equal(r["moment2"], q)
        np.testing.assert_array_equal(r["length"], np.full((h, w), n, F))
        np.testing.assert_array_equal(r["variance"], np.maximum(q - m * m, F(0)) / (n - F(1)))
    # one sample per pixel: no variance estimate
    s1, q1 = R.frame_sums(w, h, 1)
    r = R.accumulate(d["C"], d["Cp"], s1, q1, d["cur"], samples=1.0)
    assert not r["variance"].any() and (r["length"] == 1).all()


def test_camera_turned_away_leaves_no_history():
    w, h = 64, 48
    back = dict(R.CAMERA_A, look_at=(-0.3, 1.9, 10.0))       # more than 90 degrees from CAMERA_A's direction
    d = R.synthetic(w, h, camera=back, prev_camera=R.CAMERA_A)
    r = R.call(d, sigma_depth=0.0, normal_min=-1.0, max_history=INF)
    assert not r["detail"]["inside"].any() and not r["detail"]["valid"].any()
    np.testing.assert_array_equal(r["length"], np.full((h, w), F(d["samples"]), F))
    np.testing.assert_array_equal(r["color"], d["sum"] / F(d["samples"]))


@pytest.mark.parametrize("w,h", SIZES)
def test_moved_camera_synthetic_holds_every_class(w, h):
    d = R.synthetic(w, h)
    r = R.call(d)
    c = R.classes(r["detail"])
    print(w, h, c)
    assert set(c) == {"snapped", "four_valid", "some_rejected", "all_rejected_by_depth", "all_rejected_by_normal",
                      "off_screen", "sky_onto_sky", "sky_onto_surface_rejected"}
    for name, count in c.items():
        assert count >= 1, name
    # and the guides themselves: surfaces and sky, fractional coverage, history holes
    cov = d["cur"]["coverage"]
    assert (cov == 0).any() and (cov == 1).any() and ((cov > 0) & (cov < 1)).any()
    assert (d["prev"]["length"] == 0).any() and (d["prev"]["length"] > 0).any()
    # with a history the result differs from the frame's own samples where taps were valid, only there
    own = d["sum"] / F(d["samples"])
    changed = (r["color"] != own).any(0)
    assert changed[r["detail"]["valid"] > 0].all() and not changed[r["detail"]["valid"] == 0].any()
    # the cap: no history length above max_history + n
    assert float(R.call(d, max_history=8.0)["length"].max()) <= 8.0 + d["samples"]


def test_tests_switch_off():
    d = R.synthetic(70, 50)
    base = R.call(d)["detail"]
    no_depth = R.call(d, sigma_depth=0.0)["detail"]
    no_normal = R.call(d, normal_min=-1.0)["detail"]
    assert no_depth["rej_depth"].sum() == 0 < base["rej_depth"].sum()
    assert no_normal["rej_normal"].sum() == 0 < base["rej_normal"].sum()
    flat = dict(d, cur={k: v for k, v in d["cur"].items() if k != "normal"})
    assert R.call(flat)["detail"]["rej_normal"].sum() == 0     # one side without normals: the test does not run
    assert no_depth["valid"].sum() > base["valid"].sum() and no_normal["valid"].sum() > base["valid"].sum()
