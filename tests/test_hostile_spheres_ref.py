"""The reference on the hostile sphere families of tests/hostile_spheres.py,
without a GPU: what tests/test_gpu_hostile_spheres.py compares the kernels
with is checked here on its own.

The oracle (closest and any-hit, its BVH and brute force) equals, bit for bit,
the numpy float32 restatement of sphere_t and of the loop over the spheres
applied to the oracle's own triangles-only answer, on every family and ray
set, BEYOND's included.  Against float64 (hostile_spheres.sphere_f64, one
(ray, sphere) pair at a time, the sphere each ray was built about): on the
families inside the envelope every decidable pair agrees on hit or miss and
on which root is taken; the error of t in units of E_t is measured and kept
in T_RESIDUAL; every finite t the reference reports, decidable or not, lies
within GENUINE units of a float64 root of its pair; the share of pairs left
out as undecidable is capped.  The guard G = 8 selects the pairs that are
compared; every figure of T_RESIDUAL is below it.

BEYOND_MEASURED holds what the same measurements give outside the envelope;
ENVELOPE the two figures DESIGN.md §2 and include/spt.h quote."""
import functools

import numpy as np
import pytest

import hostile_spheres as S
import oracle as O

# max |t32 - t64| / E_t over the decidable hits of a family, per ray set
# (aimed, interval, inside, surface, grazing), rounded up to two digits.
T_RESIDUAL = {
    "unit256": (2.5, 2.6, 1.8, 1.8, 1.6),       # measured 2.485, 2.548, 1.794, 1.722, 1.599
    "walls_1e2": (1.9, 2.8, 2.0, 1.9, 1.7),     # measured 1.881, 2.725, 1.918, 1.896, 1.641
    "walls_1e3": (2.5, 2.4, 1.7, 1.8, 1.4),     # measured 2.49, 2.312, 1.604, 1.775, 1.395
    "walls_1e4": (2.0, 2.7, 1.9, 2.3, 1.3),     # measured 1.995, 2.649, 1.832, 2.256, 1.246
    "small_far": (3.2, 3.2, 2.0, 1.6, 1.4),     # measured 3.103, 3.103, 1.93, 1.564, 1.322
    "outside": (3.0, 3.8, 1.9, 1.8, 1.5),       # measured 2.92, 3.748, 1.891, 1.752, 1.407
}
# max over every finite t the restatement reports (decidable or not) of its
# distance to the nearer float64 root, in E_t, per family, rounded up to two digits
# (the undecidable pairs, whose E_t has error_model's floor, stay below the decidable ones)
GENUINE = {
    "unit256": 2.6,       # measured 2.548
    "walls_1e2": 2.8,     # measured 2.725
    "walls_1e3": 2.5,     # measured 2.49
    "walls_1e4": 2.7,     # measured 2.649
    "small_far": 3.2,     # measured 3.103
    "outside": 3.8,       # measured 3.748
}
# the largest undecidable share of the pairs a set may have, in every family.  Measured: aimed, interval, inside
# and surface at most 0.0057 (small_far), grazing 0.095 (small_far) to 0.1485 (outside).  The grazing share is set
# by the guard: |det| <= G E_det is an impact parameter within 8 eps (D / r)^2 = 4.8e-7 (D / r)^2 of r, D the
# origin's distance from the centre: 13.6 % of 10^U(-7, -2) at D = r, which is why those origins are near.
CAPS = {"aimed": 0.03, "interval": 0.03, "inside": 0.03, "surface": 0.03, "grazing": 0.15}
# BEYOND: per family and set, beyond_figures(): (undecidable share, share of all pairs answered unlike float64,
# worst |t32 - t64| |d| where both take the same root, decidable or not), measured
BEYOND_MEASURED = {
    ("walls_1e5", "aimed"): (0.0592, 0.0000, 1.28),
    ("walls_1e5", "interval"): (0.0002, 0.0000, 0.0612),
    ("walls_1e5", "inside"): (0.0000, 0.0000, 0.0345),
    ("walls_1e5", "surface"): (0.5980, 0.0000, 0.0343),
    ("walls_1e5", "grazing"): (0.1420, 0.0015, 13.2),
    ("small_far_1e-3", "aimed"): (0.9582, 0.0458, 0.0598),
    ("small_far_1e-3", "interval"): (0.9585, 0.0265, 0.0598),
    ("small_far_1e-3", "grazing"): (0.0125, 0.0005, 9.99e-06),
    ("small_far_3e-4", "aimed"): (1.0000, 0.2755, 0.0502),
    ("small_far_3e-4", "interval"): (1.0000, 0.1573, 0.0428),
    ("small_far_3e-4", "grazing"): (0.0040, 0.0000, 1.69e-06),
    ("surface_1e3", "surface"): (0.8100, 0.0108, 0.0207),
}
# the envelope in the caller's terms (include/spt.h): the smallest r / distance of SMALL_SWEEP and the
# largest x = (|c - o| + r) / |d| of SURFACE_SWEEP whose undecidable share is within CAPS; the next point of each
# sweep is beyond them.  No decidable pair of either sweep is answered unlike float64.
ENVELOPE = {"r_over_distance": 1e-2, "surface_x": 163.0}
# r / distance: (undecidable share, share answered unlike float64) of the aimed pairs, measured
SMALL_SWEEP = {
    1e-1: (0.0, 0.0), 3e-2: (0.0007, 0.0), 1e-2: (0.0112, 0.0007), 3e-3: (0.1210, 0.0050), 1e-3: (0.9568, 0.0435),
    3e-4: (1.0, 0.2842),
}
# wall radius R: (undecidable share, share answered unlike float64) of the surface pairs, measured; |d| is within
# exp(+-1), so x runs from 0.74 R to 5.44 R
SURFACE_SWEEP = {
    1e1: (0.0036, 0.0004), 3e1: (0.0188, 0.0), 1e2: (0.0568, 0.0008), 3e2: (0.2688, 0.0052), 1e3: (0.8008, 0.0108),
    1e4: (1.0, 0.0),
}


@functools.lru_cache(maxsize=None)
def oracle_hits(name, use_bvh, closest):
    (o, d, tmin, tmax), _ = S.all_rays(name)
    out = O.OracleScene(S.family(name), use_bvh=use_bvh).intersect(o, d, tmin, tmax, closest=closest)
    for a in out:
        a.setflags(write=False)
    return out


def reference(name):
    """What the GPU tests compare with: the brute-force oracle's closest hits."""
    return oracle_hits(name, False, True)


@functools.lru_cache(maxsize=None)
def pairs(name, ray_set):
    """(t32, root32, f64 dict, decidable) of a set's rays against the spheres they were built about."""
    sets, which = S.rays(name)
    sph = S.family(name)["spheres"]
    t, root = S.sphere_records(sph, *sets[ray_set], which[ray_set])
    ref = S.sphere_f64(sph, *sets[ray_set], which[ray_set])
    return t, root, ref, S.decidable(ref)


@pytest.mark.parametrize("name", S.FAMILIES + S.BEYOND)
def test_restatement_equals_oracle(name):
    mesh = S.family(name)
    (o, d, tmin, tmax), spans = S.all_rays(name)
    assert 19000 <= o.shape[1] <= 21000
    assert (name == "alone") == (len(mesh["pos_tri"]) == 0)
    for use_bvh in (True, False):
        tris = O.OracleScene(S.without_spheres(mesh), use_bvh=use_bvh)
        for closest in (True, False):
            held = tris.intersect(o, d, tmin, tmax, closest=closest)
            want = S.trace_spheres(mesh["spheres"], o, d, tmin, tmax, held=held, anyhit=not closest)
            got = oracle_hits(name, use_bvh, closest)
            np.testing.assert_array_equal(got[0], want[0], err_msg=f"{name} bvh {use_bvh} closest {closest}")
            h = want[0] != -1
            for k in (1, 2, 3):
                np.testing.assert_array_equal(got[k][h], want[k][h], err_msg=f"{name} record {k}")
            sp = got[0] < -1
            assert sp.sum() > 2000 and (got[0] >= -1 - len(mesh["spheres"])).all()
            assert (got[2][sp] == 0).all() and (got[3][sp] == 0).all()
            assert np.isfinite(got[1][h]).all()               # a report is finite; a miss is id -1
            if closest and use_bvh:                           # the tree does not matter
                for a, b in zip(got, oracle_hits(name, False, True)):
                    np.testing.assert_array_equal(a, b)
    deg = reference(name)[0][spans["degenerate"]]
    assert (deg[3::6] == -1).all() and (deg[5::6] == -1).all()   # zero and NaN directions miss
    # one sphere alone, through sphere_records: the reported t is that sphere's own
    ids, t = reference(name)[:2]
    sp = np.flatnonzero(ids < -1)
    one, _ = S.sphere_records(mesh["spheres"], o[:, sp], d[:, sp], tmin[sp], tmax[sp], -2 - ids[sp])
    np.testing.assert_array_equal(one, t[sp])


@pytest.mark.parametrize("name", S.F64_FAMILIES)
def test_hit_or_miss_and_root_against_float64(name):
    for st in S.F64_SETS:
        t, root, ref, dec = pairs(name, st)
        share = 1.0 - dec.mean()
        print(f'    ("{name}", "{st}"): undecidable {share:.4f}, hits {int((root[dec] >= 0).sum())}, '
              f'misses {int((root[dec] < 0).sum())}')
        np.testing.assert_array_equal(root[dec], ref["root"][dec], err_msg=f"{name} {st}")
        assert share <= CAPS[st], (name, st, share)
        assert (root[dec] >= 0).sum() > 100, (name, st)
    # the sets do exercise both answers and both roots
    roots = np.concatenate([pairs(name, st)[1][pairs(name, st)[3]] for st in S.F64_SETS])
    assert (roots == -1).sum() > 200 and (roots == 0).sum() > 200 and (roots == 1).sum() > 200


def t_residual(name, st):
    t, root, ref, dec = pairs(name, st)
    h = dec & (root >= 0)
    _, e_t = S.error_model(ref)
    return float(np.max(np.abs(t[h].astype(np.float64) - ref["t"][h]) / e_t[h]))


@pytest.mark.parametrize("name", S.F64_FAMILIES)
def test_t_error_in_units_of_the_model(name):
    got = tuple(t_residual(name, st) for st in S.F64_SETS)
    print(f'    "{name}": (' + ", ".join(f"{x:.3g}" for x in got) + "),")
    for st, x, rec in zip(S.F64_SETS, got, T_RESIDUAL[name]):
        assert rec <= S.G, "the guard is too small for this figure: raise G"
        assert x <= rec and x > rec / 1.1, (name, st, x, rec)


def genuine(name):
    worst = 0.0
    for st in S.F64_SETS:
        t, root, ref, _ = pairs(name, st)
        h = np.isfinite(t)
        _, e_t = S.error_model(ref)
        with np.errstate(all="ignore"):
            mid = ref["b"] / ref["a"]                         # without real roots: where they would meet
            lo, hi = np.where(np.isnan(ref["lo"]), mid, ref["lo"]), np.where(np.isnan(ref["hi"]), mid, ref["hi"])
            t64 = t.astype(np.float64)
            off = np.minimum(np.abs(t64 - lo), np.abs(t64 - hi)) / e_t
        assert np.isfinite(off[h]).all()
        worst = max(worst, float(off[h].max()))
    return worst


@pytest.mark.parametrize("name", S.F64_FAMILIES)
def test_every_reported_hit_is_a_root_of_its_pair(name):
    x = genuine(name)
    print(f'    "{name}": genuine {x:.3g}')
    rec = GENUINE[name]
    assert x <= rec and x > rec / 1.1, (name, x, rec)


def beyond_figures(name, st):
    """(undecidable share, share of all pairs whose float32 answer takes another
    root than float64 or a hit for a miss, worst |t32 - t64| |d| over the pairs
    where both take the same root: a length, in the scene's units)."""
    t, root, ref, dec = pairs(name, st)
    wrong = root != ref["root"]
    same = (root >= 0) & ~wrong
    worst = float(np.max(np.abs(t[same].astype(np.float64) - ref["t"][same]) * ref["dlen"][same])) if same.any() else 0.0
    return 1.0 - dec.mean(), wrong.mean(), worst


def close_to(got, rec):
    return all(abs(x - r) <= 0.1 * abs(r) + 1e-3 * (r < 1) for x, r in zip(got, rec))


@pytest.mark.parametrize("name", S.BEYOND)
def test_beyond_the_envelope_is_measured(name):
    ids, t = reference(name)[:2]
    assert np.isfinite(t[ids != -1]).all()
    for st in S.F64_SETS:
        tt, root, _, _ = pairs(name, st)
        assert (np.isfinite(tt) | (tt == np.inf)).all() and ((root >= 0) == np.isfinite(tt)).all()
    sets = {"walls_1e5": S.F64_SETS, "surface_1e3": ("surface",)}.get(name, ("aimed", "interval", "grazing"))
    for st in sets:
        got = beyond_figures(name, st)
        print(f'    ("{name}", "{st}"): ({got[0]:.3f}, {got[1]:.4f}, {got[2]:.3g}),')
        assert close_to(got, BEYOND_MEASURED[(name, st)]), (name, st, got)


@pytest.mark.parametrize("ratio", sorted(SMALL_SWEEP, reverse=True))
def test_envelope_of_small_spheres(ratio):
    """Aimed rays from about the origin at spheres 100 away of r / distance = ratio."""
    got = beyond_figures(f"small_far_{ratio:g}", "aimed")[:2]
    print(f'    {ratio:g}: ({got[0]:.4f}, {got[1]:.4f}),')
    assert close_to(got, SMALL_SWEEP[ratio]), (ratio, got)
    _, root, ref, dec = pairs(f"small_far_{ratio:g}", "aimed")
    np.testing.assert_array_equal(root[dec], ref["root"][dec])
    assert (got[0] <= CAPS["aimed"]) == (ratio >= ENVELOPE["r_over_distance"])


def surface_sweep(R):
    t, root, ref, dec = pairs(f"surface_{R:g}", "surface")
    x = (np.sqrt(ref["op2"]) + ref["r"]) / ref["dlen"]
    np.testing.assert_array_equal(root[dec], ref["root"][dec])
    return 1.0 - dec.mean(), (root != ref["root"]).mean(), float(x.min()), float(x.max())


@pytest.mark.parametrize("R", sorted(SURFACE_SWEEP))
def test_envelope_of_rays_leaving_a_surface(R):
    """Rays from a float32 point of a wall of radius R, tmin = 1e-3, |d| over
    exp(+-1): x = (|c - o| + r) / |d| is 2 R / |d|."""
    und, wrong, lo, hi = surface_sweep(R)
    print(f'    {R:g}: ({und:.4f}, {wrong:.4f}),   # x from {lo:.3g} to {hi:.3g}')
    assert close_to((und, wrong), SURFACE_SWEEP[R]), (R, und, wrong)
    assert (und <= CAPS["surface"]) == (hi <= ENVELOPE["surface_x"] * 1.001)


def test_tie_rules():
    mesh = S.family("tie")
    (o, d, _, _), spans = S.all_rays("tie")
    a = spans["aimed"]
    np.testing.assert_array_equal(o[:, a][:, :5].T, S.TIE_RAYS[0])
    np.testing.assert_array_equal(d[:, a][:, :5].T, S.TIE_RAYS[1])
    ids, t = (x[a][:5] for x in reference("tie")[:2])
    for i, (want_id, want_t) in enumerate(S.TIE_EXPECT):
        assert ids[i] == want_id and t[i] == np.float32(want_t), (i, ids[i], t[i])
    # the ties are ties: the sphere alone and the triangle alone report the same float
    tri = O.OracleScene(S.without_spheres(mesh), use_bvh=False).intersect(S.TIE_RAYS[0].T, S.TIE_RAYS[1].T,
                                                                           np.zeros(5, np.float32), np.full(5, 1e20, np.float32))
    alone, _ = S.sphere_records(mesh["spheres"], S.TIE_RAYS[0].T, S.TIE_RAYS[1].T, np.zeros(5, np.float32),
                                np.full(5, 1e20, np.float32), [0, 1, 2, 0, 1])
    assert tri[0][0] == 0 and tri[1][0] == alone[0] == 4.0
    assert tri[0][1] == 1 and tri[1][1] == np.nextafter(np.float32(4.0), np.float32(5.0)) and alone[1] == 4.0
    assert tri[0][2] == -1 and alone[2] == 4.0
    assert tri[1][3] == alone[3] == 2.0 and tri[1][4] > alone[4] == 2.0
    # any-hit: the triangle pass's answer stands wherever it has one
    anyh = oracle_hits("tie", False, False)[0][a][:5]
    assert anyh[0] == 0 and anyh[1] == 1 and anyh[2] == -4


def test_identical_spheres_answer_with_the_lower_index():
    for name in ("unit256", "alone"):
        sph = S.family(name)["spheres"]
        ids = reference(name)[0]
        for lo, hi in S.IDENTICAL:
            np.testing.assert_array_equal(sph[lo], sph[hi])
            assert (ids == -2 - lo).sum() > 20 and not (ids == -2 - hi).any(), (name, lo, hi)
        # the nest: every shell is reached, the inner ones by the rays that start inside the outer
        assert all((ids == -2 - k).any() for k in (40, 41, 42, 43))
