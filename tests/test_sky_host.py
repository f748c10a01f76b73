"""Sky sampling without a GPU: spt_sky_table_build against the
float64 restatement (tests/sky_ref.py) on the awkward images; the densities
integrating to 1 over the sphere; a stratified count of drawn cells against
their probabilities; the restated estimator of a plane's irradiance against a
float64 quadrature; the host program tests/native/sky_check.cpp under ASan +
UBSan — sky_uniform, the unfold and the density bit for bit against the
restatement, the builder on n = 1, 2, 4096 and hostile images; and the
refusals that need no device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

import envmap_ref as E
import sky_ref as S
import sptamd
from sptamd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallpt-enoki-optix_amd", "csrc")
F = np.float32
INV, LIM = _lib.SPT_ERR_INVALID, _lib.SPT_ERR_LIMIT


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the table

def table_cases():
    cases = {"n1": np.full((1, 1, 3), 2.5, F), "random8": E.random_map(8, 3), "odd5": E.random_map(5, 4)}
    hot = np.zeros((8, 8, 3), F)
    hot[0, 0] = (1000.0, 10.0, 1.0)            # a corner: its stencil crosses two octahedral edges
    cases["hot_corner"] = hot
    zr = E.random_map(8, 6)
    zr[2:6] = 0                                 # rows 2 and 5 keep weight through the stencil, rows 3 and 4 have
                                                # none (an edge mirrors row j onto row 7 - j: the band is symmetric)
    cases["zero_row"] = zr
    tail = np.zeros((8, 8, 3), F)               # an interior block: the stencil spills one texel around it and
    tail[2:4, 2:4] = E.random_map(2, 7)         # reaches no edge, so rows and columns 5 .. 7 carry no weight
    cases["zero_tail"] = tail
    cases["empty_zero"] = np.zeros((4, 4, 3), F)
    neg = -E.random_map(6, 8)
    neg[1, 2] = (-3.0, 0.5, -900.0)
    cases["negative"] = neg
    return cases


def test_table_matches_the_restatement():
    for name, tex in table_cases().items():
        marg, cond, pdf = sptamd.sky_table_build(tex)
        ref = S.sky_table(tex)
        if name.startswith("empty"):
            assert ref is None and marg.size == 0 and cond.size == 0 and pdf.size == 0, name
            continue
        n = tex.shape[0]
        rm, rc, rp, P = ref
        d = max(int(np.abs(bits(a).astype(np.int64) - bits(b)).max()) for a, b in ((marg, rm), (cond, rc), (pdf, rp)))
        print(f"{name}: n = {n}, worst difference {d} ulp, sum P = {P.sum()!r}")
        assert d == 0, name                                     # the same float64 operations in the same order
        assert marg[-1] == 1 and np.all(np.diff(marg) >= 0) and np.all(cond[:, -1] == 1) and np.all(np.diff(cond, axis=1) >= 0)
        assert np.all(np.isfinite(pdf)) and np.all(pdf >= 0) and abs(P.sum() - 1) < 1e-12
    marg, cond, pdf = sptamd.sky_table_build(table_cases()["zero_row"])
    assert marg[4] == marg[3] == marg[2] and not pdf[3:5].any() and pdf[2].all() and pdf[5].all()    # flat: never drawn
    assert np.array_equal(cond[3], np.array([0] * 7 + [1], F)) and np.array_equal(cond[4], cond[3])
    marg, cond, pdf = sptamd.sky_table_build(table_cases()["zero_tail"])
    assert marg[4] == 1.0 and marg[3] < 1.0 and not pdf[5:].any()      # no number reaches the weightless last rows
    assert np.all(cond[1:5, 4] == 1.0) and np.all(cond[1:5, 3] < 1.0)  # (row and column 4 hold the stencil's spill)
    marg, cond, pdf = sptamd.sky_table_build(table_cases()["hot_corner"])
    # the corner texel lies in the stencils of its own 2 x 2 block, of two cells across each of the
    # two edges that meet there (mirrored: the far end of row 0 and of column 0) and of the opposite corner
    lit = {(0, 0), (0, 1), (1, 0), (1, 1), (0, 7), (0, 6), (7, 0), (6, 0), (7, 7)}
    assert {(int(r), int(c)) for r, c in zip(*np.nonzero(pdf))} == lit
    marg, cond, pdf = sptamd.sky_table_build(table_cases()["n1"])
    assert marg.tolist() == [1.0] and cond.tolist() == [[1.0]] and pdf[0, 0] == F(0.25)   # 4 pi / 4 pi over a square of area 4
    a, b, c = sptamd.sky_table_build(table_cases()["negative"])
    a2, b2, c2 = sptamd.sky_table_build(-table_cases()["negative"])
    assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(c, c2)      # |.|: the sign does not matter


def test_densities_integrate_to_one_over_the_sphere():
    """sum over a fine grid of the octahedral square of sky_pdf(R^T p) dw, dw = da db / |p|^3 (the
    measure of the parametrisation; its own sum is 4 pi), through the rotation and back."""
    rot = E.rotation((0.3, 1.0, -0.2), 37.0)

    def grid(m):
        x, y, z = E.texel_direction(m, *np.meshgrid(np.arange(m), np.arange(m), indexing="xy"))
        dw = (2.0 / m) ** 2 / np.sqrt(x * x + y * y + z * z) ** 3
        p = np.stack([x, y, z], axis=-1).reshape(-1, 3)
        return (p @ rot.astype(np.float64)).astype(F), dw.ravel()            # R^T p

    assert abs(grid(512)[1].sum() - 4 * np.pi) < 1e-3
    for name in ("random8", "odd5", "hot_corner", "zero_row", "n1"):
        tex = table_cases()[name]
        tab = S.sky_table(tex)
        d, dw = grid(64 * tex.shape[0])      # 64 x 64 points inside every cell, none on an edge
        total = float((S.sky_pdf(tab, rot, d).astype(np.float64) * dw).sum())
        # the density is constant over a cell in (a, b), so the only error is f32 and the grid
        # points that R^T and R move across a cell edge (the nearest is 1/128 of a cell from one)
        print(f"{name}: integral of the density {total:.7f}")
        assert abs(total - 1) < 1e-5, name
    d = grid(512)[0]
    d2 = (d * F(37.5)).astype(F)                               # any length: the density is of the direction
    np.testing.assert_allclose(S.sky_pdf(S.sky_table(table_cases()["random8"]), rot, d2[::97]),
                               S.sky_pdf(S.sky_table(table_cases()["random8"]), rot, d[::97]), rtol=2e-6)


def test_stratified_draws_count_the_cells():
    """1024 x 1024 stratified (xi0, xi1): a cell's count is (numbers choosing row j) x
    (numbers choosing column i of it), each within 1 of 1024 x its f32 cdf step."""
    m = 1024
    xi = ((np.arange(m) + 0.5) / m).astype(F)
    for name in ("random8", "zero_row", "hot_corner", "odd5"):
        tex = table_cases()[name]
        marg, cond, pdf, P = S.sky_table(tex)
        n = len(marg)
        j = S.search(np.broadcast_to(marg, (m, n)), xi)
        rows = np.bincount(j, minlength=n)
        counts = np.zeros((n, n), np.int64)
        for r in range(n):
            counts[r] = rows[r] * np.bincount(S.search(np.broadcast_to(cond[r], (m, n)), xi), minlength=n)
        pm = np.diff(np.concatenate([[0.0], marg.astype(np.float64)]))
        pc = np.diff(np.concatenate([np.zeros((n, 1)), cond.astype(np.float64)], axis=1), axis=1)
        bound = m * (pm[:, None] + pc) + 1 + m * m * 2e-7
        err = np.abs(counts - m * m * P)
        print(f"{name}: worst count error {err.max():.1f} of {m * m}, bound there {bound.ravel()[err.argmax()]:.1f}")
        assert counts.sum() == m * m and np.all(err <= bound), name
        assert not counts[P == 0].any(), name                  # a cell without weight is never drawn


def test_restated_estimator_matches_the_quadrature():
    """The irradiance of a tilted plane under the n = 8 map: the mean of pi c at 2^16
    samples against sum M(d) cos dw over a 1024^2 grid of the octahedral square."""
    tex, rot = E.random_map(8, 3), E.rotation((0.3, 1.0, -0.2), 37.0)
    tab = S.sky_table(tex)
    # tilted 40-odd degrees away from the brightest cell
    jb, ib = np.unravel_index(np.argmax(tab[3]), tab[3].shape)
    sun = np.array(E.texel_direction(8, ib, jb)) @ rot.astype(np.float64)
    nrm = sun / np.linalg.norm(sun) + 0.8 * np.array([0.3, 0.9, 0.2]) / np.linalg.norm([0.3, 0.9, 0.2])
    nrm = (nrm / np.linalg.norm(nrm)).astype(F)
    n = 1 << 16
    xi = np.random.default_rng(21).random((4, n)).astype(F)
    traced, d, tmin, c = S.sky_sample(tab, tex, rot, np.ones(3, F), np.tile(nrm, (n, 1)), np.ones((n, 3), F), *xi)
    assert 0.3 < traced.mean() < 0.95 and np.all(tmin[traced] > 0)
    est = c.astype(np.float64) * np.pi
    mean, se = est.mean(axis=0), est.std(axis=0, ddof=1) / np.sqrt(n)
    m = 1024
    x, y, z = E.texel_direction(m, *np.meshgrid(np.arange(m), np.arange(m), indexing="xy"))
    ln = np.sqrt(x * x + y * y + z * z)
    p = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    dq = p @ rot.astype(np.float64)
    cos = np.maximum((dq @ nrm.astype(np.float64)) / ln.ravel(), 0.0)
    M = E.lookup(tex, rot, dq.astype(F)).astype(np.float64)
    quad = (M * (cos * (2.0 / m) ** 2 / ln.ravel() ** 3)[:, None]).sum(axis=0)
    zs = (mean - quad) / se
    print("quadrature", quad, "mean", mean, "se", se, "z", zs)
    assert np.all(np.abs(zs) <= 5)
    # against cosine sampling of the same integral: the variance is lower
    rng = np.random.default_rng(22)
    u1, u2 = rng.random(n), rng.random(n)
    r, ph = np.sqrt(u1), 2 * np.pi * u2
    t = np.cross(nrm, [1.0, 0, 0])
    t /= np.linalg.norm(t)
    bt = np.cross(nrm, t)
    dc = (r * np.cos(ph))[:, None] * t + (r * np.sin(ph))[:, None] * bt + np.sqrt(1 - u1)[:, None] * nrm
    cosest = E.lookup(tex, rot, dc.astype(F)).astype(np.float64) * np.pi
    print("cosine-sampled mean", cosest.mean(axis=0), "variance ratio", cosest.var(axis=0) / est.var(axis=0))
    assert np.all(est.var(axis=0) < cosest.var(axis=0))


def test_refusals_need_no_device():
    L = _lib.lib
    for name in ("spt_scene_set_sky_sampling", "spt_scene_get_sky_sampling", "spt_sky_table_build"):
        assert name in _lib.EXPORTED and hasattr(L, name), name
    assert L.spt_scene_set_sky_sampling(None, 1, 0.5) == INV and b"NULL scene" in L.spt_last_error()
    fake = 0x1000    # never dereferenced: refused first
    assert L.spt_scene_set_sky_sampling(fake, 2, 0.5) == INV and b"on = 2" in L.spt_last_error()
    for share in (0.0, 1.0, -0.25, 1.5, float("nan"), float("inf")):
        for on in (0, 1):
            assert L.spt_scene_set_sky_sampling(fake, on, share) == INV and b"share" in L.spt_last_error(), share
    assert L.spt_scene_get_sky_sampling(None, None, None, None) == INV
    one = np.ones((1, 1, 3), F)
    n = ctypes.c_uint32(7)
    assert L.spt_sky_table_build(one.ctypes.data, 1, None, None, None, None) == INV
    assert L.spt_sky_table_build(None, 1, None, None, None, ctypes.byref(n)) == INV
    assert L.spt_sky_table_build(one.ctypes.data, 0, None, None, None, ctypes.byref(n)) == INV
    assert L.spt_sky_table_build(one.ctypes.data, 4097, None, None, None, ctypes.byref(n)) == LIM
    assert L.spt_sky_table_build(one.ctypes.data, 1, None, None, None, ctypes.byref(n)) == 0 and n.value == 1
    assert callable(sptamd.HipBackend.set_sky_sampling) and "sky_table_build" in sptamd.__all__
    assert ctypes.sizeof(_lib.RenderStats) == 288


# ---- the host program under the sanitizers

def _build(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "sky_check"
    root = os.environ.get("ROCM_PATH", "/opt/rocm")   # spt_math.h includes the HIP runtime header for its markers
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(root, "include"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "sky_check.cpp")], check=True, capture_output=True)
    return exe


def _run(exe, args, text=""):
    run = subprocess.run([str(exe), *args], input=text, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    return run.stdout.strip().split("\n")


def test_host_program_hash_unfold_density_and_builder(tmp_path):
    exe = _build(tmp_path)
    rng = np.random.default_rng(3)
    rows = [(0, 0, 0, k) for k in range(5)] + [(702, 7, 4, 1), (0xffffffff, (1 << 24) - 1, 63, 4)]
    rows += [tuple(int(v) for v in r) for r in
             np.stack([rng.integers(0, 1 << 32, 300), rng.integers(0, 1 << 24, 300), rng.integers(0, 64, 300),
                       rng.integers(0, 5, 300)], axis=1)]
    got = _run(exe, ["hash"], "".join("%d %d %d %d\n" % r for r in rows))
    a = np.array(rows, np.uint64)
    for k in range(5):
        sel = a[:, 3] == k
        want = bits(S.sky_uniform(a[sel, 0], a[sel, 1], a[sel, 2], k))
        assert [int(g, 16) for g, s in zip(got, sel) if s] == list(want)
    u = np.array([int(g, 16) for g in got], np.uint32).view(F)
    assert u.min() >= 0 and u.max() < 1 and len(set(got)) > 295      # numbers in [0, 1), no stuck stream
    # the five keys of one cast are not keys of the next, nor light_uniform's numbers
    import nee_ref
    k0 = [S.sky_uniform(5, 9, dd, kk) for dd in (3, 4) for kk in range(5)]
    assert len({float(v) for v in k0}) == 10
    assert all(float(S.sky_uniform(5, 9, 3, kk)) != float(nee_ref.light_uniform(5, 9, 3, kk)) for kk in range(3))
    ab = np.concatenate([rng.uniform(-1, 1, (400, 2)).astype(F),
                         np.array([[0, 0], [1, 0], [0, -1], [0.5, 0.5], [-0.5, 0.5], [1, 1], [-1, 1], [-1, -1], [0.25, -0.75],
                                   [0.99999994, 0.99999994], [-0.0, 0.7]], F)])
    got = _run(exe, ["unfold"], "".join("%08x %08x\n" % (x, y) for x, y in bits(ab)))
    p = S.unfold(ab[:, 0], ab[:, 1])
    assert [tuple(int(v, 16) for v in g.split()) for g in got] == [tuple(r) for r in bits(p)]
    l1 = np.abs(p.astype(np.float64)).sum(axis=1)
    assert np.all(np.abs(l1 - 1) < 3e-7)                            # on the octahedron
    inside = np.abs(ab[:, 0].astype(np.float64)) + np.abs(ab[:, 1]) <= 1
    assert np.all(p[inside, 2] >= 0) and np.all(p[~inside, 2] <= 0)
    # the unfold inverts the lookup's fold: the lookup's coordinates of p are (a, b) again
    valid, fx, fy = E.coords(8, E.identity(), p[:400])
    back = np.stack([(fx + 0.5) / 8 * 2 - 1, (fy + 0.5) / 8 * 2 - 1], axis=1)
    assert valid.all() and np.abs(back - ab[:400]).max() < 2e-6
    tex, rot = E.random_map(8, 3), E.rotation((0.3, 1.0, -0.2), 37.0)
    tab = S.sky_table(tex)
    d = np.concatenate([rng.normal(size=(500, 3)).astype(F), np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [0, 0, 0],
                                                                       [1e-30, 0, 0], [3e38, 3e38, 0]], F)])
    path = tmp_path / "pdf.f32"
    np.concatenate([[F(8)], rot.reshape(9), tab[2].reshape(-1), d.reshape(-1)]).astype(F).tofile(path)
    got = _run(exe, ["pdf", str(path)])
    assert [int(g, 16) for g in got] == list(bits(S.sky_pdf(tab, rot, d)))
    lines = _run(exe, ["build"])
    print("\n".join(lines))
    seen = {}
    for line in lines:
        name, n, cells, bad = line.split()
        assert int(bad) == 0, line
        seen[name] = (int(n), int(cells))
    assert seen["one"] == (1, 1) and seen["two"] == (2, 4) and seen["large"] == (4096, 4096 * 4096)
    assert seen["one_zero"][1] == 0 and seen["all_nan"][1] == 0 and seen["hostile"][1] == 49
    assert seen["negative"][1] == 49 and seen["zero_tail"][1] == 49 and seen["subnormal"][1] == 49
