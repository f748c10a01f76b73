"""Light sampling without a GPU: spt_light_table_build against
the float64 restatement (tests/nee_ref.py) on the awkward tables; the host
program tests/native/light_check.cpp under ASan + UBSan — light_uniform and
the triangle map bit for bit against the restatement, the table builder on the
hostile families' soups; the refusals that need no device; the triangle map's
area preservation; and the restated estimator against the closed-form form
factor of a rectangle."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

import hostile
import nee_ref as R
import sptamd
from sptamd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smallpt-enoki-optix_amd", "csrc")
F = np.float32
INV, LIM = _lib.SPT_ERR_INVALID, _lib.SPT_ERR_LIMIT


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the table

def quad(y, x0, x1, z0, z1):
    return np.array([[x0, y, z0, x1, y, z0, x1, y, z1], [x0, y, z0, x1, y, z1, x0, y, z1]], F)


def table_cases():
    rng = np.random.default_rng(5)
    soup = rng.uniform(-1, 1, size=(40, 9)).astype(F)
    mats = rng.integers(0, 4, size=40)
    emi = np.array([[0, 0, 0], [3, 1, 2], [0, 0, 0], [0.5, 9, 0.1]], F)
    cases = {"mixed": (soup, mats, emi)}
    deg = soup.copy()
    deg[3, 3:6] = deg[3, 0:3]                  # a zero-area member in the middle ...
    deg[39, 6:9] = deg[39, 3:6]                # ... and one at the end
    mats_deg = mats.copy()
    mats_deg[[3, 39]] = 1
    cases["degenerate"] = (deg, mats_deg, emi)
    nan = soup.copy()
    nan[7, 4] = np.nan
    nan[11, 0] = np.inf
    mats_nan = mats.copy()
    mats_nan[[7, 11]] = 3
    cases["nan"] = (nan, mats_nan, emi)
    cases["single"] = (soup, np.where(np.arange(40) == 17, 1, 0), emi)
    cases["empty_no_emitter"] = (soup, mats, np.zeros((4, 3), F))
    cases["empty_zero_area"] = (np.repeat(soup[:, 0:3], 3, axis=1).reshape(40, 9), mats, emi)
    cases["unused_material"] = (soup, np.where(mats == 3, 2, mats), emi)   # material 3 emits, no triangle has it
    cases["non_monotone_mats"] = (soup, np.array([3, 1, 0, 2] * 10), emi)
    cases["mat_out_of_range"] = (soup, mats - 1 + 2 * (np.arange(40) % 3 == 0) * 3, emi)
    cases["no_mat_ids"] = (soup, None, np.array([[1, 1, 1]], F))
    cases["negative_emission"] = (soup, mats, np.array([[0, 0, 0], [-1, -2, -3], [0, 0, 0], [1, 1, 1]], F))
    return cases


def test_table_matches_the_restatement():
    worst = 0
    for name, (tv, mat, emi) in table_cases().items():
        ids, cdf, pdf = sptamd.light_table_build(tv, mat, emi)
        rid, rcdf, rpdf = R.light_table(tv, mat, emi)[:3]
        np.testing.assert_array_equal(ids, rid, err_msg=name)
        if name.startswith("empty"):
            assert len(ids) == 0, name
            continue
        assert len(ids) > 0 and cdf[-1] == 1.0 and np.all(np.diff(cdf) >= 0), name
        # measured: bit-equal in every case (the same float64 operations in the same order)
        d = max(int(np.abs(bits(cdf).astype(np.int64) - bits(rcdf)).max()),
                int(np.abs(bits(pdf).astype(np.int64) - bits(rpdf)).max()))
        worst = max(worst, d)
        print(f"{name}: {len(ids)} lights, worst difference {d} ulp")
        assert d == 0, name
    ids, cdf, pdf = sptamd.light_table_build(*table_cases()["degenerate"])
    k = list(ids).index(3)
    assert pdf[k] == 0 and cdf[k] == cdf[k - 1]            # a member, never chosen
    assert pdf[-1] == 0 and cdf[-1] == 1.0 and cdf[-2] == 1.0
    ids, cdf, pdf = sptamd.light_table_build(*table_cases()["nan"])
    for t in (7, 11):
        assert pdf[list(ids).index(t)] == 0
    assert np.all(np.isfinite(cdf)) and np.all(np.isfinite(pdf))
    ids, cdf, pdf = sptamd.light_table_build(*table_cases()["single"])
    assert list(ids) == [17] and cdf[0] == 1.0
    area = 0.5 * np.linalg.norm(np.cross(*(table_cases()["single"][0][17].astype(np.float64).reshape(3, 3)[1:] -
                                           table_cases()["single"][0][17].astype(np.float64).reshape(3, 3)[0])))
    assert pdf[0] == F(1.0 / area)


def test_table_abi_refusals_and_two_call_protocol():
    L = _lib.lib
    tv = np.ascontiguousarray(table_cases()["mixed"][0])
    emi = np.ones((1, 3), F)
    n = ctypes.c_uint32(77)
    assert L.spt_light_table_build(tv.ctypes.data, None, 40, emi.ctypes.data, 1, None, None, None, 0, None) == INV
    assert L.spt_light_table_build(None, None, 40, emi.ctypes.data, 1, None, None, None, 0, ctypes.byref(n)) == INV
    assert L.spt_light_table_build(tv.ctypes.data, None, 40, None, 1, None, None, None, 0, ctypes.byref(n)) == INV
    assert L.spt_light_table_build(tv.ctypes.data, None, 1 << 28, emi.ctypes.data, 1, None, None, None, 0,
                                   ctypes.byref(n)) == LIM
    assert L.spt_light_table_build(tv.ctypes.data, None, 40, emi.ctypes.data, 1, None, None, None, 0, ctypes.byref(n)) == 0
    assert n.value == 40
    cdf = np.zeros(40, F)
    assert L.spt_light_table_build(tv.ctypes.data, None, 40, emi.ctypes.data, 1, None, cdf.ctypes.data, None, 39,
                                   ctypes.byref(n)) == INV and b"capacity" in L.spt_last_error()
    assert not cdf.any()
    assert L.spt_light_table_build(tv.ctypes.data, None, 40, emi.ctypes.data, 1, None, cdf.ctypes.data, None, 40,
                                   ctypes.byref(n)) == 0 and cdf[-1] == 1.0
    assert L.spt_light_table_build(None, None, 0, None, 0, None, None, None, 0, ctypes.byref(n)) == 0 and n.value == 0


def test_setter_refusals_need_no_device():
    L = _lib.lib
    for name in ("spt_scene_set_light_sampling", "spt_scene_get_light_sampling", "spt_light_table_build",
                 "spt_scene_get_shadow_casts"):
        assert name in _lib.EXPORTED and hasattr(L, name), name
    assert L.spt_scene_set_light_sampling(None, 1) == INV and b"NULL scene" in L.spt_last_error()
    fake = 0x1000    # never dereferenced: refused first
    assert L.spt_scene_set_light_sampling(fake, 2) == INV and b"on = 2" in L.spt_last_error()
    assert L.spt_scene_get_light_sampling(None, None, None) == INV
    assert callable(sptamd.HipBackend.set_light_sampling) and "light_table_build" in sptamd.__all__
    assert L.spt_scene_get_shadow_casts(None, None) == INV and L.spt_scene_get_shadow_casts(fake, None) == INV
    assert ctypes.sizeof(_lib.RenderStats) == 288              # the counter has a call of its own


# ---- the host program under the sanitizers

def _build(tmp_path, name, extra=()):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / name
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + CSRC, *extra, "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", name + ".cpp")], check=True, capture_output=True)
    return exe


def _run(exe, args, text=""):
    run = subprocess.run([str(exe), *args], input=text, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, run.stderr[-2000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    return run.stdout.strip().split("\n")


def _hip_include():
    # spt_math.h includes the HIP runtime header for its __host__ __device__ markers
    root = os.environ.get("ROCM_PATH", "/opt/rocm")
    return ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(root, "include")]


def test_host_program_hash_map_and_hostile_tables(tmp_path):
    exe = _build(tmp_path, "light_check", _hip_include())
    rng = np.random.default_rng(3)
    rows = [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 0, 2), (702, 7, 4, 1), (0xffffffff, (1 << 24) - 1, 63, 2)]
    rows += [tuple(int(v) for v in r) for r in
             np.stack([rng.integers(0, 1 << 32, 200), rng.integers(0, 1 << 24, 200), rng.integers(0, 64, 200),
                       rng.integers(0, 3, 200)], axis=1)]
    got = _run(exe, ["hash"], "".join("%d %d %d %d\n" % r for r in rows))
    a = np.array(rows, np.uint64)
    for k in range(3):
        sel = a[:, 3] == k
        want = bits(R.light_uniform(a[sel, 0], a[sel, 1], a[sel, 2], k))
        assert [int(g, 16) for g, s in zip(got, sel) if s] == list(want)
    u = np.array([int(g, 16) for g in got], np.uint32).view(F)
    assert u.min() >= 0 and u.max() < 1 and len(set(got)) > 195      # numbers in [0, 1), no stuck stream
    xi = np.concatenate([rng.random((300, 2)).astype(F), np.array([[0, 0], [0.5, 0.5], [0.99999994, 0], [0, 0.99999994],
                                                                   [0.25, 0.75], [0.75, 0.25]], F)])
    got = _run(exe, ["map"], "".join("%08x %08x\n" % (x, y) for x, y in bits(xi)))
    b1, b2 = R.tri_map(xi[:, 0], xi[:, 1])
    assert [tuple(int(v, 16) for v in g.split()) for g in got] == list(zip(bits(b1), bits(b2)))
    assert np.all(b1 >= 0) and np.all(b2 >= 0) and np.all(b1.astype(np.float64) + b2 <= 1)
    files = []
    for name in hostile.FAMILIES:
        files.append(str(tmp_path / f"{name}.f32"))
        hostile.tri_soup(hostile.family(name)).tofile(files[-1])
    x = np.exp2(np.arange(-120, 120, dtype=np.float64))[:, None]
    files.append(str(tmp_path / "subnormal_chain.f32"))
    (x * np.array([[1, 0, 0, 1.001, 0, 0, 1, 0.001, 0]])).astype(F).tofile(files[-1])
    files.append(str(tmp_path / "mixed_1e37.f32"))
    (rng.normal(size=(300, 9)) * np.exp(rng.uniform(-85, 85, size=(300, 1)))).astype(F).tofile(files[-1])
    lines = _run(exe, ["soup", *files])
    assert len(lines) == len(files)
    for line in lines:
        name, ntri, lights, chosen_flat, non_monotone = line.split()
        assert int(chosen_flat) == 0 and int(non_monotone) == 0, line
        assert int(lights) in (0, int(ntri)), line
    print("\n".join(lines))


# ---- the triangle map preserves area

def test_triangle_map_is_area_preserving():
    """2^16 stratified points (the centres of a 256 x 256 grid of the unit square)
    binned into the 4 x 4 grid of (b1, b2): six whole cells of the triangle hold
    1/8 of it each, the four cells the hypotenuse cuts 1/16 each.  The map is
    linear with Jacobian 1/2 on either side of xi1 = xi2, so a grid cell whose
    image lies inside one bin gives that bin one point for exactly its area: a
    count can be off only by the cells whose image meets the bin's boundary,
    counted here per bin from the cells' corners (at most 2 x perimeter x 256 of them)."""
    n = 256
    c = ((np.arange(n) + 0.5) / n).astype(F)
    x1, x2 = np.meshgrid(c, c, indexing="ij")
    b1, b2 = R.tri_map(x1.ravel(), x2.ravel())
    assert np.all(b1 >= 0) and np.all(b2 >= 0) and np.all(b1.astype(np.float64) + b2 <= 1)
    bins = np.minimum((b1 * 4).astype(int), 3) * 4 + np.minimum((b2 * 4).astype(int), 3)
    counts = np.bincount(bins, minlength=16).reshape(4, 4)
    # cells meeting a bin's boundary, from the images of the cells' corners (and, for the
    # cells xi1 = xi2 cuts, of the diagonal's ends — the same corners) in float64
    e = np.arange(n + 1) / n
    g1, g2 = np.meshgrid(e, e, indexing="ij")
    up = g2 > g1
    c1 = np.where(up, g1 / 2, g1 - g2 / 2)
    c2 = np.where(up, g2 - g1 / 2, g2 / 2)
    eps = 1e-12                                    # a corner on a bin edge belongs to both sides
    lo = np.minimum(np.floor(c1 * 4 - eps), 3) * 4 + np.minimum(np.floor(c2 * 4 - eps), 3)
    hi = np.minimum(np.floor(c1 * 4 + eps), 3) * 4 + np.minimum(np.floor(c2 * 4 + eps), 3)
    touch = np.zeros((16, n, n), bool)
    for arr in (lo, hi):
        for di in (0, 1):
            for dj in (0, 1):
                b = arr[di:di + n, dj:dj + n].astype(int)
                touch[b, np.arange(n)[:, None], np.arange(n)[None, :]] = True
    straddle = touch.sum(axis=0) > 1
    for i in range(4):
        for j in range(4):
            want = 0 if i + j > 3 else (n * n / 16 if i + j == 3 else n * n / 8)
            bound = int((straddle & touch[i * 4 + j]).sum())
            print(f"bin ({i}, {j}): {counts[i, j]} points, exact {want:.0f}, cells on its boundary {bound}")
            assert bound <= 2 * 4 * n
            assert abs(counts[i, j] - want) <= bound, (i, j)
    assert counts.sum() == n * n


# ---- the restated estimator converges to the form factor

def test_restatement_converges_to_the_form_factor():
    """A floor point under a parallel rectangular light: E[c] = Le F with
    F = sum over the four corner rectangles of
    1/(2 pi) (X/sqrt(1+X^2) atan(Y/sqrt(1+X^2)) + Y/sqrt(1+Y^2) atan(X/sqrt(1+Y^2)))."""
    h, x0, x1, z0, z1 = 0.8, -0.3, 0.5, -0.2, 0.45
    tv = quad(h, x0, x1, z0, z1)
    le = np.array([[0, 0, 0], [12, 6, 3]], F)
    table = R.light_table(tv, np.array([1, 1]), le)
    np.testing.assert_allclose(table[2], 1.0 / ((x1 - x0) * (z1 - z0)), rtol=1e-6)
    n = 1 << 16
    rng = np.random.default_rng(11)
    xi = rng.random((3, n)).astype(F)
    x = np.zeros((n, 3), F)
    nh = np.tile(np.array([0, 1, 0], F), (n, 1))
    traced, d, tmin, tmax, c, lid = R.light_sample(table, x, nh, np.ones((n, 3), F), *xi)
    assert traced.all() and np.all(tmin > 0) and np.all(tmax > 1) and set(lid) == {0, 1}

    def corner(a, b):
        X, Y = abs(a) / h, abs(b) / h
        f = (X / np.sqrt(1 + X * X) * np.arctan(Y / np.sqrt(1 + X * X))
             + Y / np.sqrt(1 + Y * Y) * np.arctan(X / np.sqrt(1 + Y * Y))) / (2 * np.pi)
        return f * np.sign(a) * np.sign(b)

    ff = corner(x1, z1) - corner(x0, z1) - corner(x1, z0) + corner(x0, z0)
    c64 = c.astype(np.float64)
    mean, se = c64.mean(axis=0), c64.std(axis=0, ddof=1) / np.sqrt(n)
    print("form factor", ff, "mean / Le", mean / le[1], "z", (mean - le[1] * ff) / se)
    assert 0.05 < ff < 0.5
    assert np.all(np.abs(mean - le[1].astype(np.float64) * ff) <= 5 * se)
    # the two triangles are chosen by area: both halves of the rectangle are lit
    assert abs(np.mean(xi[0] < table[1][0]) - 0.5) < 0.01
