"""The CPU restatement of the environment-map lookup (tests/envmap_ref.py),
checked on its own before the GPU is held to it: a constant map, a smooth
function of direction across the octahedral edges and corners, where the poles
and axes land, scale invariance, the edge rule itself, and the contributions
built from the oracle reproducing the oracle's own film under a constant sky."""
import numpy as np
import pytest

import accum_ref as A
import envmap_ref as E
import oracle as O
from test_accum_ref import mode_scene

F = np.float32


def test_constant_map_gives_the_constant_for_any_length():
    rng = np.random.default_rng(3)
    d = (rng.normal(size=(4000, 3)) * np.exp(rng.uniform(-20, 20, size=(4000, 1)))).astype(F)
    for n in (1, 2, 5, 8):
        tex = np.empty((n, n, 3), F)
        tex[...] = (0.25, 3.0, 1000.0)
        got = E.lookup(tex, E.rotation((1, 2, 3), 40.0), d)
        # fl(1 - w) + w rounds to 1 for every w in [0, 1), so a power of two comes back
        # exactly ((1 - w) c and w c are exact); any other constant within an ulp per blend
        np.testing.assert_array_equal(got[:, 0], F(0.25))
        np.testing.assert_allclose(got, np.broadcast_to(tex[0, 0], got.shape), rtol=2 * np.finfo(F).eps)
    ones = np.ones((1, 1, 3), F)
    np.testing.assert_array_equal(E.lookup(ones, E.identity(), d), np.ones_like(d))
    # a zero, infinite or NaN direction has no sky
    bad = np.array([[0, 0, 0], [np.inf, 0, 0], [np.nan, 1, 0], [3e38, 3e38, 3e38]], F)
    np.testing.assert_array_equal(E.lookup(ones, E.identity(), bad), np.zeros((4, 3), F))


def smooth(x, y, z):
    ln = np.sqrt(x * x + y * y + z * z)
    x, y, z = x / ln, y / ln, z / ln
    return np.stack([1.5 + x + 0.5 * y * z, 2.0 + np.sin(2.0 * y) + 0.3 * x, 1.2 + z * z + 0.4 * x * y], -1)


def test_smooth_function_is_reproduced_across_edges_and_corners():
    """A smooth f with f(x, y, z) = f(y, x, -z).  Under that symmetry the texel grid
    about the -z pole (the corners, continued through the gutter) is the grid about
    the +z pole (the centre), and the cells across an edge are the cells across the
    a = 0 / b = 0 lines, so at the same positions inside a cell the lookups that
    touch the gutter must show the interior's interpolation error and no more."""
    n = 64
    f = lambda x, y, z: smooth(x, y, z) + smooth(y, x, -z)
    j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    tex = f(*E.texel_direction(n, i, j)).astype(F)
    # the whole image, fx and fy in (-1/2, N - 1/2), on a lattice at odd sixteenths inside
    # every cell (a set the mirror w -> 1 - w keeps); the outermost half cells are the gutter's
    c = -0.5 + (np.arange(8 * n) + 0.5) / 8.0
    fy, fx = np.meshgrid(c, c, indexing="ij")
    x, y, z = E.texel_direction(n, fx.reshape(-1), fy.reshape(-1))
    d = np.stack([x, y, z], -1).astype(F)
    touched = {}
    got = E.lookup(tex, E.identity(), d, touched=touched).astype(np.float64)
    dd = d.astype(np.float64)
    err = np.abs(got - f(dd[:, 0], dd[:, 1], dd[:, 2])).max(axis=1)
    valid, gx, gy = E.coords(n, E.identity(), d)
    assert valid.all() and np.abs(gx - fx.reshape(-1)).max() < 1e-3 and np.abs(gy - fy.reshape(-1)).max() < 1e-3
    gutter = (gx < 0) | (gx >= n - 1) | (gy < 0) | (gy >= n - 1)
    assert all(touched.get(k, 0) > 0 for k in E.EDGES), touched
    inner, outer = float(err[~gutter].max()), float(err[gutter].max())
    print(f"N = {n}: max interpolation error interior {inner:.6e}, touching the gutter {outer:.6e} "
          f"({int(gutter.sum())} of {gutter.size} lookups, {touched})")
    assert gutter.sum() == (8 * n) ** 2 - (8 * n - 8) ** 2
    # equal up to f32 rounding of the texels and the blend (values of magnitude < 8)
    assert outer <= inner + 16 * 8 * float(np.finfo(F).eps)
    # a wrong edge rule (clamping instead of the mirror) is far outside: the check has teeth
    ci = np.clip(np.floor(gx).astype(int) + 1, 0, n - 1)
    cj = np.clip(np.floor(gy).astype(int) + 1, 0, n - 1)
    far = np.abs(tex[cj, ci].astype(np.float64) - f(dd[:, 0], dd[:, 1], dd[:, 2])).max(axis=1)[gutter].max()
    assert far > 4 * inner


def test_edge_rule():
    n = 8
    for k in range(-1, n + 1):
        assert tuple(int(v) for v in E.wrap(n, -1, k)) == ((0, n - 1 - k) if 0 <= k < n else (n - 1, n - 1 if k < 0 else 0))
    assert tuple(int(v) for v in E.wrap(n, n, 3)) == (n - 1, n - 1 - 3)
    assert tuple(int(v) for v in E.wrap(n, 3, -1)) == (n - 1 - 3, 0)
    assert tuple(int(v) for v in E.wrap(n, 3, n)) == (n - 1 - 3, n - 1)
    # a corner's diagonal neighbour is the opposite corner
    assert tuple(int(v) for v in E.wrap(n, -1, -1)) == (n - 1, n - 1)
    assert tuple(int(v) for v in E.wrap(n, n, n)) == (0, 0)
    assert tuple(int(v) for v in E.wrap(n, -1, n)) == (n - 1, 0)
    assert tuple(int(v) for v in E.wrap(n, n, -1)) == (0, n - 1)
    assert tuple(int(v) for v in E.wrap(n, 2, 5)) == (2, 5)
    # N = 1: everything is the one texel
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            assert tuple(int(v) for v in E.wrap(1, i, j)) == (0, 0)


def test_poles_and_axes_land_where_the_definition_says():
    n = 8
    c = (n - 1) / 2.0   # fx of a = 0: (0.5) n - 0.5
    dirs = {"+z": (0, 0, 1), "+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0), "-z": (0, 0, -1)}
    want = {"+z": (c, c), "+x": (n - 0.5, c), "-x": (-0.5, c), "+y": (c, n - 0.5), "-y": (c, -0.5),
            "-z": (n - 0.5, n - 0.5)}   # sgn(0) = +1: the -z pole folds to the (+, +) corner
    for k, d in dirs.items():
        valid, fx, fy = E.coords(n, E.identity(), np.array(d, F) * F(7.5))
        assert valid and (float(fx), float(fy)) == want[k], (k, fx, fy)
    # the four corners are one point: the -z pole reads the mean of the four corner texels
    tex = E.random_map(n, 2, bright=0)
    got = E.lookup(tex, E.identity(), np.array([0, 0, -1], F))
    corners = np.stack([tex[0, 0], tex[0, n - 1], tex[n - 1, 0], tex[n - 1, n - 1]]).astype(np.float64).mean(0)
    np.testing.assert_allclose(got, corners, rtol=1e-6)
    # the +z pole reads the mean of the four central texels
    got = E.lookup(tex, E.identity(), np.array([0, 0, 2], F))
    mid = tex[n // 2 - 1: n // 2 + 1, n // 2 - 1: n // 2 + 1].astype(np.float64).mean((0, 1))
    np.testing.assert_allclose(got, mid, rtol=1e-6)
    # a rotation that takes world +y to the map's +z
    r = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], F)
    np.testing.assert_array_equal(E.lookup(tex, r, np.array([0, 3, 0], F)), E.lookup(tex, E.identity(), np.array([0, 0, 3], F)))


def test_power_of_two_scale_gives_the_same_bits():
    rng = np.random.default_rng(9)
    d = rng.normal(size=(5000, 3)).astype(F)
    tex = E.random_map(8, 4)
    r = E.rotation((0.3, 1.0, -0.2), 77.0)
    base = E.lookup(tex, r, d)
    for k in (-40, -3, 1, 10, 60):
        np.testing.assert_array_equal(E.lookup(tex, r, d * F(2.0 ** k)), base, err_msg=f"2^{k}")
    assert not np.array_equal(E.lookup(tex, r, d * F(3.0)), base)    # (and not for any scale: rounding differs)


W, H, SPP, DEPTH = 12, 8, 6, 4
KW = dict(rr_start_depth=2, env=(0.3, 0.7, 1.0))


@pytest.mark.parametrize("mode", ["unit", "albedo", "emit"])
def test_contributions_under_a_unit_map_are_the_oracles(mode):
    """N = 1, texel (1, 1, 1): M = 1 exactly, so x_s is the oracle's own sample and the film its film."""
    m, albedo, emi = mode_scene(mode)
    osc = O.OracleScene(m, albedo=albedo)
    osc_e = O.OracleScene(m, albedo=albedo, emission=emi) if emi is not None else None
    p = O.reference_params(W, H, SPP, DEPTH, **KW)
    x = E.contributions(osc, p, np.ones((1, 1, 3), F), E.identity(), osc_emit=osc_e)
    full = osc_e if osc_e is not None else osc
    np.testing.assert_array_equal(x, A.contributions(full, p))
    np.testing.assert_array_equal(A.moments(x)[2], full.render(p)[0])
    assert x.max() > 0


def test_contributions_follow_the_map():
    m, albedo, _ = mode_scene("albedo")
    osc = O.OracleScene(m, albedo=albedo)
    p = O.reference_params(W, H, SPP, DEPTH, **KW)
    tex = E.random_map(8, 1)
    touched = {}
    x = E.contributions(osc, p, tex, E.rotation((1, 1, 0), 30.0), touched=touched)
    esc, d, T = E.escapes(osc, p)
    assert esc.any() and not esc.all()
    assert not x[~np.broadcast_to(esc[:, None], x.shape)].any()
    assert x.max() > 10.0     # a bright texel was seen
    x2 = E.contributions(osc, p, (tex * F(2)).astype(F), E.rotation((1, 1, 0), 30.0))
    np.testing.assert_array_equal(x2, (x * F(2)).astype(F))   # linear in the map (a power of two: exact)
