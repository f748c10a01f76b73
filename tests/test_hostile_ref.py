"""The reference on the hostile families of tests/hostile.py, without a GPU:
what tests/test_gpu_hostile.py compares the kernels with is checked here on
its own.  For every family the brute-force oracle (no tree) equals the
oracle's BVH bit for bit; every aimed ray has a hit no later than its target
(an arithmetic mistake shared by both cannot hide as an agreed miss); every
closest-hit record is a real point of its triangle in float64; and the
coincident stacks answer with their smallest triangle id.  The host builders
run on every family under AddressSanitizer + UBSan in a stand-alone program
(tests/native/soup_build.cpp).

Measured here and kept in CLOSEST_RESIDUAL (the closest hits) and
REF_RESIDUAL (every crossing along the rays): the float64 residual |o + t d
- (w p0 + u p1 + v p2)| over the triangle's longest edge, the largest per
family.  The share of aimed rays that hit is 1.0 in every family; the latest
aimed hit is at t = 1.0000005, among slivers' needles at t = 1.0004853."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import hostile
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallpt-enoki-optix_amd", "csrc")

# The largest residual of the brute-force oracle's closest hits per family,
# rounded up to two digits: a measurement of the reference, not of a kernel.
# (near, through): the near sets (aimed, interval, surface, degenerate) start
# within a few triangle sizes of what they hit; the through rays start 1e3 scene
# diameters away, where the float32 rounding of t alone moves the point by 1e-4
# diameters, many lengths of a small triangle (the chain's and the far cloud's
# most of all), so they are kept apart.  A needle's record is loose along the
# needle: slivers' near figure is in units of a longest edge 1e5 widths long.
CLOSEST_RESIDUAL = {
    "mixed_scale": (1.5e-06, 0.0014),      # measured 1.415e-06, 0.001347
    "corner_chain": (1.7e-06, 7.9),        # measured 1.665e-06, 7.813
    "far_small": (9.7e-07, 48),            # measured 9.679e-07, 47.69 (8 hits)
    "coincident": (8.1e-07, 0.00031),      # measured 8.005e-07, 0.0003025
    "slivers": (0.0084, 0.002),            # measured 0.008359, 0.001962
    "flat_axes": (1.7e-06, 0.0053),        # measured 1.619e-06, 0.005298
    "nonfinite": (2.8e-06, 0.0013),        # measured 2.797e-06, 0.001259
}
# The same over every crossing the reference finds along the rays (crossings():
# each ray cast again from just behind its hit until it leaves the scene; the
# closest hits are the first crossings).  An any-hit query may stop at any of
# these triangles, and where sizes span ten binades the closest hits alone say
# little about them: a through ray of mixed_scale crosses up to 506 triangles,
# and the reference's own record of a small one far down the ray is 4000 times
# worse than that of any closest hit.  This is the REF_RESIDUAL the any-hit
# records of tests/test_gpu_hostile.py are held to (4 x).  All 20 000 rays of
# every family, measured with crossings(name, 1); mixed_scale and nonfinite
# take a minute each that way, so the test below walks the first 48 crossings
# of every 16th of their rays.
REF_RESIDUAL = {
    "mixed_scale": (3.3e-05, 6.0),         # measured 3.236e-05, 5.922 (2 785 561 crossings)
    "corner_chain": (1.7e-06, 23),         # measured 1.665e-06, 22.1
    "far_small": (9.7e-07, 48),            # measured 9.679e-07, 47.69
    "coincident": (1.1e-06, 0.00035),      # measured 1.051e-06, 0.0003456
    "slivers": (0.0084, 0.002),            # measured 0.008359, 0.001962
    "flat_axes": (2.9e-06, 0.0057),        # measured 2.814e-06, 0.005694
    "nonfinite": (3.5e-05, 1.1),           # measured 3.426e-05, 1.056 (3 531 233 crossings)
}
NEAR_SETS = ("aimed", "interval", "surface", "degenerate")


def ref_residual(name, ray_set):
    return REF_RESIDUAL[name][1 if ray_set == "through" else 0]


def crossings(name, stride, passes=1 << 30):
    """The largest residual (near, through) over every crossing (the first
    `passes` of them) of every stride-th ray: the oracle's closest hit (its
    BVH: test_tree_independence), then again from the next float behind that
    hit, until nothing is hit."""
    (o, d, tmin, tmax), spans = hostile.all_rays(name)
    mesh = hostile.family(name)
    sc = O.OracleScene(mesh, use_bvh=True)
    act = np.arange(0, o.shape[1], stride)
    worst, cur = np.zeros(o.shape[1]), np.array(tmin)
    while len(act) and passes > 0:
        passes -= 1
        oo, dd = np.ascontiguousarray(o[:, act]), np.ascontiguousarray(d[:, act])
        r = sc.intersect(oo, dd, cur[act], tmax[act])
        h = r[0] >= 0
        act = act[h]
        worst[act] = np.maximum(worst[act], hostile.residual(mesh, oo, dd, *r)[h])
        cur[act] = np.nextafter(r[1][h], np.float32(np.inf))
    return max(worst[spans[s]].max() for s in NEAR_SETS), worst[spans["through"]].max()


@functools.lru_cache(maxsize=None)
def brute(name):
    """The brute-force oracle's closest hits over all_rays(name): (tri, t, u, v), read-only."""
    (o, d, tmin, tmax), _ = hostile.all_rays(name)
    out = O.OracleScene(hostile.family(name), use_bvh=False).intersect(o, d, tmin, tmax)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def residuals(name):
    (o, d, _, _), spans = hostile.all_rays(name)
    r = hostile.residual(hostile.family(name), o, d, *brute(name))
    return {s: r[sl] for s, sl in spans.items()}


@pytest.mark.parametrize("name", hostile.FAMILIES)
def test_tree_independence(name):
    (o, d, tmin, tmax), spans = hostile.all_rays(name)
    assert 19000 <= o.shape[1] <= 21000
    tree = O.OracleScene(hostile.family(name), use_bvh=True).intersect(o, d, tmin, tmax)
    ref = brute(name)
    np.testing.assert_array_equal(tree[0], ref[0])
    hit = ref[0] >= 0
    for k in (1, 2, 3):
        np.testing.assert_array_equal(tree[k][hit], ref[k][hit])
    bad = np.flatnonzero(~hostile.finite_tris(hostile.family(name)))
    assert not np.isin(ref[0], bad).any()                 # a non-finite triangle is never hit
    deg = ref[0][spans["degenerate"]]
    assert (deg[3::6] == -1).all() and (deg[5::6] == -1).all()   # zero and NaN directions miss


@pytest.mark.parametrize("name", hostile.FAMILIES)
def test_no_missed_hits(name):
    _, spans = hostile.all_rays(name)
    tri, t, _, _ = brute(name)
    a = spans["aimed"]
    share = (tri[a] >= 0).mean()
    print(name, "aimed hit share", share, "latest t", t[a].max())
    assert share == 1.0
    assert t[a].max() <= 1.0 + 1e-3 and t[a].min() >= 0.0
    iv = spans["interval"]                                # the same rays, cut to their intervals
    (_, _, tmin, tmax), _ = hostile.all_rays(name)
    h = tri[iv] >= 0
    assert h.any() and not h.all()                        # the intervals cut some hits away and keep some
    assert (t[iv][h] >= tmin[iv][h]).all() and (t[iv][h] <= tmax[iv][h]).all()
    inside = (t[a] >= tmin[iv]) & (t[a] <= tmax[iv])      # the unbounded hit lies in the interval: it is the hit
    np.testing.assert_array_equal(tri[iv][inside], tri[a][inside])


@pytest.mark.parametrize("name", hostile.FAMILIES)
def test_records_are_points_of_their_triangles(name):
    res = residuals(name)
    tri = brute(name)[0]
    _, spans = hostile.all_rays(name)
    for s in hostile.RAY_SETS:
        h = tri[spans[s]] >= 0
        worst = float(np.max(res[s][h])) if h.any() else 0.0
        print(f'    ("{name}", "{s}"): {worst:.2g},   # {int(h.sum())} hits')
        assert np.isfinite(res[s][h]).all()
        assert worst <= CLOSEST_RESIDUAL[name][1 if s == "through" else 0], (name, s, worst)
    # within a few sizes of the triangle a record is sharp: a few float32 ulps of the distances
    assert CLOSEST_RESIDUAL[name][0] <= (1e-2 if name == "slivers" else 1e-5)


@pytest.mark.parametrize("name", hostile.FAMILIES)
def test_every_crossing_is_a_point_of_its_triangle(name):
    full = name not in ("mixed_scale", "nonfinite")
    near, through = crossings(name, 1) if full else crossings(name, 16, 48)
    print(f'    "{name}": crossings near {near:.4g} through {through:.4g}')
    assert CLOSEST_RESIDUAL[name][0] <= REF_RESIDUAL[name][0] and CLOSEST_RESIDUAL[name][1] <= REF_RESIDUAL[name][1]
    assert near <= REF_RESIDUAL[name][0] and through <= REF_RESIDUAL[name][1]
    if full:                                              # the recorded figure is the measured one, rounded up
        assert near > REF_RESIDUAL[name][0] / 1.1 and through > REF_RESIDUAL[name][1] / 1.1


def test_tie_rule_on_coincident_stacks():
    mesh = hostile.family("coincident")
    first = hostile.stack_ids(mesh)
    assert len(np.unique(first)) == 4 and np.bincount(first).max() == 600
    tri = brute("coincident")[0]
    hit = tri >= 0
    np.testing.assert_array_equal(tri[hit], first[tri[hit]])
    assert len(np.unique(tri[hit])) == 4                  # every stack is reached, from one side or the other


def test_host_builders_under_sanitizers(tmp_path):
    """tests/native/soup_build.cpp on every family and on the two soups whose
    subnormal centroid extents indexed the SAH bins at INT_MIN."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    files = []
    for name in hostile.FAMILIES:
        files.append(str(tmp_path / f"{name}.f32"))
        hostile.tri_soup(hostile.family(name)).tofile(files[-1])
    x = np.exp2(np.arange(-120, 120, dtype=np.float64))[:, None]
    files.append(str(tmp_path / "subnormal_chain.f32"))
    (x * np.array([[1, 0, 0, 1.001, 0, 0, 1, 0.001, 0]])).astype(np.float32).tofile(files[-1])
    rng = np.random.default_rng(10)
    files.append(str(tmp_path / "mixed_1e37.f32"))
    (rng.normal(size=(300, 9)) * np.exp(rng.uniform(-85, 85, size=(300, 1)))).astype(np.float32).tofile(files[-1])
    exe = tmp_path / "soup_build"
    srcs = [os.path.join(ROOT, "tests", "native", "soup_build.cpp"), os.path.join(CSRC, "bvh_build.cpp"),
            os.path.join(CSRC, "bvh8_build.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, "-o", str(exe), *srcs, "-lpthread"],
                   check=True, capture_output=True)
    # (the leak check needs ptrace, which a sandboxed test run may not have; it is not what this looks for)
    run = subprocess.run([str(exe), *files], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    lines = run.stdout.strip().split("\n")
    assert len(lines) == len(files)
    print(run.stdout)
