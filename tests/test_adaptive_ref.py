"""tests/adaptive_ref.py checked on its own: the float32 restatement of
spt_adapt_select's rule against a float64 one on inputs away from the
threshold, and the properties an adaptive schedule must have whatever the
kernels do — count is a prefix length, the sky converges at min_spp, max_spp is
a hard cap, a NaN pixel runs to max_spp, sample_base 0 selects every pixel."""
import functools

import numpy as np
import pytest

import accum_ref as A
import adaptive_ref as R
import oracle as O
from test_accum_ref import mode_scene

W, H, N, DEPTH = 12, 8, 16, 4
KW = dict(rr_start_depth=2, env=(0.3, 0.7, 1.0))
PASSES = [2, 2, 4, 8]
RULE = dict(min_spp=2, max_spp=16, tolerance=0.1, floor=0.03)


@functools.lru_cache(maxsize=None)
def samples(mode):
    m, albedo, emi = mode_scene(mode)
    x = A.contributions(O.OracleScene(m, albedo=albedo, emission=emi), O.reference_params(W, H, N, DEPTH, **KW))
    x.setflags(write=False)
    return x


def prefix_moments(x, n):
    s, q, _, _ = A.moments(x[:n])
    return s, q


@pytest.mark.parametrize("mode", ["unit", "albedo", "emit"])
@pytest.mark.parametrize("n", [2, 3, 8, 15])
def test_f32_rule_agrees_with_f64_away_from_the_threshold(mode, n):
    s, q = prefix_moments(samples(mode), n)
    for tol in (0.02, 0.1, 0.3):
        got = R.converged(s, q, n, tol, 0.03)
        want, v, t2 = R.converged_f64(s, q, n, tol, 0.03)
        # f32 against f64: t^2 is off by a few ulp of itself; v by a few ulp of
        # itself plus, where q - m m cancels, a few ulp of q / (n - 1).  64 ulp
        # of their sum is far above both (about a dozen rounded operations)
        qn = np.asarray(q, np.float64).reshape(3, -1).sum(axis=0) / n / (n - 1)
        far = np.abs(v - t2) > 64 * np.finfo(np.float32).eps * (qn + v + t2)
        assert far.sum() > far.size // 2, "most pixels must be testable"
        np.testing.assert_array_equal(got[far], want[far])


@pytest.mark.parametrize("mode", ["unit", "albedo", "emit"])
def test_schedule_properties(mode):
    x = samples(mode)
    s, q, count, actives = R.schedule(x, PASSES, **RULE)
    # the first pass takes every pixel (sample_base 0), whatever count holds
    assert actives[0].all()
    assert R.active(None, None, np.full(5, 77), 0, **RULE).all()
    # count is a prefix length: one of the pass boundaries, and the sums are that prefix's
    bounds = np.cumsum(PASSES)
    assert np.isin(count, bounds).all() and count.min() >= RULE["min_spp"] and count.max() <= RULE["max_spp"]
    for b in bounds:
        sb, qb = prefix_moments(x, int(b))
        sel = count == b
        np.testing.assert_array_equal(s[:, sel], sb[:, sel])
        np.testing.assert_array_equal(q[:, sel], qb[:, sel])
    # a pixel that left the list never comes back: the actives are nested
    for a, b in zip(actives[1:], actives[2:]):
        assert not (b & ~a).any()
    # the passes are not degenerate at this tolerance (unit mode at this size is:
    # no pixel's first two samples disagree, so every pixel stops at min_spp)
    n_act = [int(a.sum()) for a in actives]
    print(mode, n_act)
    if mode != "unit":
        assert all(0 < n < W * H for n in n_act[1:]), n_act


def test_sky_converges_at_min_spp():
    """Unit mode: a sky pixel's samples all escape, so its variance is 0 after two."""
    x = samples("unit")
    sky = (x == x[0]).all(axis=0).all(axis=0) & (x[0].sum(axis=0) > 0)
    assert sky.sum() > 4
    for mn in (2, 4):
        _, _, count, _ = R.schedule(x, [mn, 4, 8], mn, 16, 0.1, 0.03)
        assert (count[sky] == mn).all()


def test_max_spp_is_a_hard_cap_and_min_spp_a_floor():
    x = samples("albedo")
    # tolerance 0: nothing with variance converges; the cap stops them
    _, _, count, actives = R.schedule(x, [4, 4, 4, 4], 2, 8, 0.0, 0.0)
    assert count.max() == 8 and not actives[2].any() and not actives[3].any()
    # a huge tolerance: everything converges at once, but not before min_spp
    _, _, count, actives = R.schedule(x, [2, 2, 4, 8], 8, 16, 1e9, 1.0)
    assert (count == 8).all() and actives[1].all() and actives[2].all() and not actives[3].any()


@pytest.mark.parametrize("where", ["sum", "sum_sq"])
def test_nan_pixel_runs_to_max_spp(where):
    x = samples("albedo").copy()
    s, q = prefix_moments(x, 4)
    s, q = s.copy(), q.copy()
    (s if where == "sum" else q)[1, 3, 5] = np.nan
    count = np.full((H, W), 4)
    act = R.active(s, q, count, 4, 2, 16, 1e9, 1.0).reshape(H, W)
    assert act[3, 5] and act.sum() == 1            # everything else converged at this tolerance
    assert not R.active(s, q, count, 16, 2, 16, 1e9, 1.0).any()   # ... and the cap holds for it too
    # through a schedule: a NaN contribution poisons the sums from sample 1 on
    x[1, 0, 2, 2] = np.nan
    _, _, c, _ = R.schedule(x, PASSES, 2, 16, 1e9, 1.0)
    assert c[2, 2] == 16 and (np.delete(c.ravel(), 2 * W + 2) == 2).all()


def test_count_mismatch_is_never_active():
    s, q = prefix_moments(samples("albedo"), 4)
    count = np.full((H, W), 4)
    count[0, 0] = 2
    count[0, 1] = 8
    act = R.active(s, q, count, 4, 8, 16, 0.0, 0.0).reshape(H, W)   # n < min_spp: all that hold n
    assert not act[0, 0] and not act[0, 1] and act.sum() == W * H - 2
