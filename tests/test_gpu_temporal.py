"""spt_temporal_accumulate on the GPU: bit for bit against the float32
restatement (tests/temporal_ref.py), the planes it may write, and the
TemporalAccumulator end to end under a still and an orbiting camera."""
import math

import numpy as np
import pytest
import torch

import sptamd
from sptamd import scenes

import temporal_ref as R

pytestmark = pytest.mark.gpu

# the kernels of namespace spt_temporal in libspt.so, all launched below
# (tests/test_temporal_host.py holds the built library to this list)
KERNELS = ["_ZN12spt_temporal15temporal_kernelENS_12TemporalArgsE"]

F = np.float32
INF = float("inf")
OUTPUTS = ("color", "moment2", "length", "film", "variance")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F)).cuda()


def dev_dict(d, drop=()):
    return None if d is None else {k: dev(v) for k, v in d.items() if k not in drop}


_SYNTH = {}


def synth(w, h):
    """temporal_ref.synthetic(w, h) and its device copies, made once and left unchanged."""
    if (w, h) not in _SYNTH:
        d = R.synthetic(w, h)
        d["dev"] = {k: dev_dict(d[k]) for k in ("cur", "prev", "prev_guides")}
        d["dev"]["sum"], d["dev"]["sum_sq"] = dev(d["sum"]), dev(d["sum_sq"])
        _SYNTH[(w, h)] = d
    return _SYNTH[(w, h)]


def run_device(d, prev=True, normals=(True, True), camera=None, **kw):
    g = d["dev"]
    cur = {k: v for k, v in g["cur"].items() if normals[0] or k != "normal"}
    pg = {k: v for k, v in g["prev_guides"].items() if normals[1] or k != "normal"}
    res = sptamd.temporal_accumulate(g["sum"], g["sum_sq"], cur, d["camera"] if camera is None else camera,
                                     prev=g["prev"] if prev else None, prev_aov=pg if prev else None,
                                     prev_camera=d["prev_camera"] if prev else None, samples=d["samples"], **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def run_ref(d, prev=True, normals=(True, True), **kw):
    cur = {k: v for k, v in d["cur"].items() if normals[0] or k != "normal"}
    pg = {k: v for k, v in d["prev_guides"].items() if normals[1] or k != "normal"}
    return R.accumulate(d["C"], d["Cp"], d["sum"], d["sum_sq"], cur, prev=d["prev"] if prev else None,
                        prev_guides=pg if prev else None, samples=d["samples"], **kw)


def assert_same(got, want):
    for k in OUTPUTS:
        assert got[k].dtype == np.float32 and want[k].dtype == np.float32
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


PARAMS = [{}, {"sigma_depth": 0.0}, {"sigma_depth": -1.0, "normal_min": -1.0}, {"normal_min": -1.0}, {"normal_min": -2.0},
          {"max_history": 0.0}, {"max_history": 8.0}, {"max_history": INF}, {"max_history": INF, "sigma_depth": 0.3}]


@pytest.mark.parametrize("w,h", [(64, 48), (70, 50)])
@pytest.mark.parametrize("kw", PARAMS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "defaults")
def test_bit_exact_against_the_f32_restatement(w, h, kw):
    d = synth(w, h)
    want = run_ref(d, **kw)
    assert (want["detail"]["valid"] > 0).any() or kw.get("max_history") == 0.0
    assert_same(run_device(d, **kw), want)


@pytest.mark.parametrize("w,h", [(1, 1), (3, 70), (70, 3)])
def test_bit_exact_at_degenerate_sizes(w, h):
    d = synth(w, h)
    for kw in ({}, {"max_history": INF, "sigma_depth": 0.0, "normal_min": -1.0}):
        assert_same(run_device(d, **kw), run_ref(d, **kw))


@pytest.mark.parametrize("w,h", [(64, 48), (70, 50)])
@pytest.mark.parametrize("normals", [(False, False), (True, False), (False, True)])
def test_bit_exact_without_normal_planes(w, h, normals):
    d = synth(w, h)
    want = run_ref(d, normals=normals)
    assert want["detail"]["rej_normal"].sum() == 0       # the normal test runs only with both sides' planes
    assert_same(run_device(d, normals=normals), want)


@pytest.mark.parametrize("w,h", [(64, 48), (70, 50), (1, 1)])
def test_first_frame_has_no_history(w, h):
    d = synth(w, h)
    got = run_device(d, prev=False)
    assert_same(got, run_ref(d, prev=False))
    np.testing.assert_array_equal(got["length"], np.full((h, w), F(d["samples"])))
    np.testing.assert_array_equal(got["film"], d["sum"] / F(d["samples"]))


@pytest.mark.parametrize("w,h", [(64, 48), (70, 50)])
def test_thin_lens_is_treated_as_its_centre(w, h):
    d = synth(w, h)
    lens = dict(d["camera"], lens_radius=0.07, focal_dist=4.0)
    # focal_dist scales the centre ray before it is normalised: same direction up to rounding, so the
    # restatement is given the lens camera's constants too; the radius alone must change nothing at all
    radius_only = dict(d["camera"], lens_radius=0.07)
    assert_same(run_device(d, camera=radius_only), run_device(d))
    d2 = dict(d, C=R.constants(lens, w, h))
    assert_same(run_device(d, camera=lens), run_ref(d2))


def test_identity_camera_on_the_device():
    w, h = 70, 50
    d = dict(synth(w, h))
    d["camera"], d["C"] = d["prev_camera"], d["Cp"]
    want = run_ref(d, max_history=INF)
    assert want["detail"]["snap_x"].all() and want["detail"]["snap_y"].all()
    assert_same(run_device(d, max_history=INF), want)


GUARD = -7.0


@pytest.mark.parametrize("skip", [None, "film", "variance"])
def test_writes_only_its_outputs(skip):
    w, h = 70, 50
    d = synth(w, h)
    g = d["dev"]
    P = w * h
    sizes = {"color": 3 * P, "moment2": 3 * P, "length": P, "film": 3 * P, "variance": 3 * P}
    pad = 4096
    # one arena, every output between guard bands; inputs cloned to see they stay as they were
    arena = torch.full((sum(sizes.values()) + pad * (len(sizes) + 1),), GUARD, dtype=torch.float32, device="cuda")
    out, at, spans = {}, pad, {}
    for name, n in sizes.items():
        shape = (h, w) if name == "length" else (3, h, w)
        out[name] = arena[at:at + n].view(shape)
        spans[name] = (at, at + n)
        at += n + pad
    before = {k: {n: t.clone() for n, t in g[k].items()} for k in ("cur", "prev", "prev_guides")}
    res = sptamd.temporal_accumulate(g["sum"], g["sum_sq"], g["cur"], d["camera"], prev=g["prev"], prev_aov=g["prev_guides"],
                                     prev_camera=d["prev_camera"], samples=d["samples"], out=out,
                                     want_film=skip != "film", want_variance=skip != "variance")
    torch.cuda.synchronize()
    assert res[skip] is None if skip else all(res[k] is not None for k in OUTPUTS)
    want = run_ref(d)
    host = arena.cpu().numpy()
    mask = np.ones(host.shape, bool)
    for name, (a, b) in spans.items():
        if name == skip:
            continue                      # not asked for: its span must still hold the guard value
        mask[a:b] = False
        np.testing.assert_array_equal(host[a:b].reshape(want[name].shape), want[name], err_msg=name)
    assert (host[mask] == GUARD).all()
    for k, planes in before.items():
        for n, t in planes.items():
            assert torch.equal(t, g[k][n]), (k, n)


def test_overlapping_out_and_prev_raises():
    d = synth(64, 48)
    g = d["dev"]
    kw = dict(prev=g["prev"], prev_aov=g["prev_guides"], prev_camera=d["prev_camera"], samples=d["samples"])
    for out in ({"color": g["prev"]["color"]}, {"length": g["prev"]["length"]}, {"film": g["prev"]["moment2"]},
                {"variance": g["sum"]}, {"moment2": g["cur"]["normal"]}, {"length": g["prev_guides"]["depth"]}):
        keep = {k: v.clone() for k, v in out.items()}
        with pytest.raises(sptamd.SptError) as e:
            sptamd.temporal_accumulate(g["sum"], g["sum_sq"], g["cur"], d["camera"], out=out, **kw)
        assert e.value.code == sptamd._lib.SPT_ERR_INVALID and "overlaps" in str(e.value)
        torch.cuda.synchronize()
        for k, v in out.items():
            assert torch.equal(v, keep[k])        # refused before any device work
    with pytest.raises(ValueError):
        sptamd.temporal_accumulate(g["sum"], g["sum_sq"], g["cur"], d["camera"], prev=g["prev"], samples=4)


# ------------------------------------------------------------- end to end
W, H, CASTS, SPP, FRAMES = 64, 48, 4, 4, 6


@pytest.fixture(scope="module")
def scene():
    mesh = scenes.mitsuba_synth(detail=0.25)
    sc = sptamd.Scene()
    sc.add_arrays(mesh)
    sc.commit(0)
    return sc


def orbit(camera, degrees):
    """`camera` turned `degrees` about its up axis through look_at."""
    f, a, u = (np.array(camera[k], np.float64) for k in ("look_from", "look_at", "up"))
    u = u / np.linalg.norm(u)
    v, t = f - a, math.radians(degrees)
    v = v * math.cos(t) + np.cross(u, v) * math.sin(t) + u * np.dot(u, v) * (1 - math.cos(t))
    return dict(camera, look_from=tuple(float(x) for x in (a + v).astype(F)))


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def host(t):
    return {k: v.cpu().numpy() for k, v in t.items()} if isinstance(t, dict) else t.cpu().numpy()


@pytest.mark.parametrize("normal_min", [-1.0, None], ids=["normal_test_off", "default_normal_min"])
def test_still_camera_end_to_end(scene, normal_min):
    """Six frames of 4 spp of one view with max_history = inf: every pixel's
    history is 24 samples long, the film is the mean of the six frames' sums,
    and it is nearer the 256-spp render than one 4-spp frame is.

    With the normal test off every pixel reads itself and keeps its history.
    With the default normal_min = 0.9 the definition compares the pixel's
    averaged first-hit normal n / cov with itself: at a pixel whose samples
    straddle an edge that mean is shorter than 1, and where its squared length
    is below 0.9 the pixel fails its own normal test and restarts every frame
    (include/spt.h, Limits).  Measured on an MI355X: 103 of the 3072 pixels of
    this scene; exactly the pixels the restatement names, and the only ones."""
    params = sptamd.make_params(W, H, SPP, CASTS)
    t = sptamd.TemporalAccumulator(scene, params, max_history=INF, normal_min=normal_min)
    sums, sqs, first = [], [], None
    for k in range(FRAMES):
        t.frame(SPP)
        torch.cuda.synchronize()
        sums.append(t.sum.cpu().numpy())
        sqs.append(t.sum_sq.cpu().numpy())
        if k == 0:
            first = t.film.cpu().numpy()
    assert t.samples == FRAMES * SPP
    length = t.length.cpu().numpy()
    g = host(t.aov)
    with np.errstate(all="ignore"):
        nn = g["normal"] / g["coverage"]
        self_dot = (nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]
    own = (g["coverage"] > 0) & ~(self_dot >= F(0.9))          # pixels that fail the default normal test on themselves
    if normal_min is None:
        print(f"still camera, normal_min 0.9: {int(own.sum())} of {own.size} pixels restart every frame")
        assert 0 < own.sum() < 0.1 * own.size
        np.testing.assert_array_equal(length, np.where(own, F(SPP), F(FRAMES * SPP)))
    else:
        np.testing.assert_array_equal(length, np.full((H, W), FRAMES * SPP, F))
    # successive frames drew new samples
    assert all((sums[k] != sums[0]).any() for k in range(1, FRAMES))
    # the restatement in f32 and f64 over the device's own sums and guides: the tolerance, and the exact bits
    C = R.constants(sptamd.reference_camera(), W, H)
    kept = length == FRAMES * SPP
    out = {}
    for dtype in (np.float32, np.float64):
        prev = None
        for s, q in zip(sums, sqs):
            prev = R.accumulate(C, C, s, q, g, prev=prev, prev_guides=None if prev is None else g, samples=SPP,
                                max_history=INF, normal_min=0.9 if normal_min is None else normal_min, dtype=dtype)
        out[dtype] = prev
    film = t.film.cpu().numpy()
    np.testing.assert_array_equal(film, out[np.float32]["film"])
    np.testing.assert_array_equal(t.variance.cpu().numpy(), out[np.float32]["variance"])
    mean = sum(s.astype(np.float64) for s in sums) / (FRAMES * SPP)
    kept = kept & (out[np.float64]["length"] == FRAMES * SPP)       # (f64 may decide a pixel at the threshold otherwise)
    tol = 8.0 * float(np.abs(out[np.float32]["film"].astype(np.float64) - out[np.float64]["film"])[:, kept].max())
    err = float(np.abs(film.astype(np.float64) - mean)[:, kept].max())
    print(f"still camera: max |film - f64 mean| {err:.3g}, tolerance {tol:.3g}")
    assert 0 < tol < 1e-4 and err <= tol
    # the 24 samples are samples 0..23 of the pixel: the film is the 24-spp render up to summation order
    ref24, _ = scene.render(sptamd.make_params(W, H, FRAMES * SPP, CASTS))
    assert float(np.abs(film - ref24.cpu().numpy())[:, kept].max()) <= 1e-5
    ref, _ = scene.render(sptamd.make_params(W, H, 256, CASTS))
    ref = ref.cpu().numpy()
    e_t, e_1 = rmse(film, ref), rmse(first, ref)
    print(f"still camera: rmse to 256 spp: one 4-spp frame {e_1:.4f}, six frames accumulated {e_t:.4f}")
    assert e_t < e_1
    # reset: the next frame stands alone again
    t.reset()
    t.frame(SPP)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(t.length.cpu().numpy(), np.full((H, W), SPP, F))
    np.testing.assert_array_equal(t.film.cpu().numpy(), t.sum.cpu().numpy() / F(SPP))


def test_orbit_end_to_end(scene):
    """Six frames of 4 spp, the camera turned 1 degree per frame about its up
    axis, default parameters: the last frame's temporal film is nearer a 256-spp
    render of the last view than that frame's own 4 spp, and denoise_var of it
    (depth guide, the temporal variance) is nearer still.  (Checked on the CPU
    first through the oracle's per-sample contributions, first hits and the f32
    restatements, with depth and coverage guides: rmse to 256 spp 0.0733 for the
    frame's own 4 spp, 0.0211 temporal, 0.0172 temporal + denoise_var; denoise_var
    of the 4 spp alone 0.0237; mean history length after six frames 23.85 of 24.
    Measured on an MI355X with the normal guide on, as here: 0.0733, 0.0318, 0.0196
    with the depth guide, 0.0202 with every guide; mean history length 23.20.)
    The device result of every frame is the f32 restatement's over the device's
    own planes, bit for bit."""
    base = sptamd.reference_camera()
    params = sptamd.make_params(W, H, SPP, CASTS)
    t = sptamd.TemporalAccumulator(scene, params)
    prev = prev_g = prev_C = None
    for k in range(FRAMES):
        cam = orbit(base, 1.0 * k)
        t.frame(SPP, camera=cam)
        torch.cuda.synchronize()
        C = R.constants(cam, W, H)
        s, q, g = t.sum.cpu().numpy(), t.sum_sq.cpu().numpy(), host(t.aov)
        want = R.accumulate(C, C if prev is None else prev_C, s, q, g, prev=prev, prev_guides=prev_g, samples=SPP)
        got = {"color": t.color, "moment2": t.moment2, "length": t.length, "film": t.film, "variance": t.variance}
        assert_same(host(got), want)
        if k:
            D = want["detail"]
            assert (D["valid"] > 0).mean() > 0.9 and not (D["snap_x"] & D["snap_y"]).all()   # moved, and found its history
        prev, prev_g, prev_C = {k2: want[k2] for k2 in ("color", "moment2", "length")}, g, C
    own = s / F(SPP)
    film = t.film.cpu().numpy()
    ref, _ = scene.render(sptamd.make_params(W, H, 256, CASTS, camera=cam))
    clean = sptamd.denoise_var(t.film, t.variance, {"depth": t.aov["depth"]})
    full = sptamd.denoise_var(t.film, t.variance, t.aov)
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    e_own, e_t, e_d, e_f = rmse(own, ref), rmse(film, ref), rmse(clean.cpu().numpy(), ref), rmse(full.cpu().numpy(), ref)
    print(f"orbit: rmse to 256 spp of the last view: own 4 spp {e_own:.4f}, temporal {e_t:.4f}, "
          f"+ denoise_var (depth guide) {e_d:.4f}, + denoise_var (all guides, not gated) {e_f:.4f}; "
          f"mean history length {float(t.length.mean()):.2f}")
    assert e_t < e_own
    assert e_d < e_t
    # a gathered length is a rounded weighted mean of four: a few ulps above the samples drawn at the most
    assert float(t.length.max()) <= FRAMES * SPP * (1 + 1e-5) and float(t.length.mean()) > 0.9 * FRAMES * SPP
