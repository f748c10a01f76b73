"""numpy restatement of spt_adapt_select's rule (include/spt.h) and of a whole
adaptive schedule, written from the definition, not from the kernels.

Pixel p is active for a pass starting at n = sample_base iff
  n == 0, or count[p] == n and (n < min_spp or (n < max_spp and not converged(p))),
with, in float32, one rounded operation at a time (accum_ref.moments' mean and
variance), per channel c
  m_c = sum_c / n,  q_c = sum_sq_c / n,  var_c = 0 if n < 2 else max(q_c - m_c m_c, 0) / (n - 1),
  v = (var_r + var_g) + var_b,  m = (m_r + m_g) + m_b,
  t = tolerance max(m, floor),  converged = v <= t t,
the two max() keeping a NaN operand, so that a NaN anywhere makes the comparison false.

schedule() runs the rule over per-sample contributions x[s] (accum_ref.contributions:
the oracle's) pass by pass: an active pixel's sums take the pass's samples in
sample order, the others keep theirs.
"""
import numpy as np

F = np.float32


def nanmax(a, b):
    """max(a, b) that keeps a NaN of a (the rule's fmaxf: spt.h), float32."""
    a = np.asarray(a, F)
    return np.where(np.isnan(a), a, np.where(a > b, a, b)).astype(F)


def converged(sum, sum_sq, n, tolerance, floor):
    """(npix,) bool for planes (3, npix) float32 holding n >= 1 samples each."""
    with np.errstate(invalid="ignore", over="ignore"):
        s, q = np.asarray(sum, F).reshape(3, -1), np.asarray(sum_sq, F).reshape(3, -1)
        m = (s / F(n)).astype(F)
        if n < 2:
            var = np.zeros_like(m)
        else:
            qq = (q / F(n)).astype(F)
            d = (qq - (m * m).astype(F)).astype(F)
            var = (nanmax(d, F(0)) / F(n - 1)).astype(F)
        v = ((var[0] + var[1]).astype(F) + var[2]).astype(F)
        ms = ((m[0] + m[1]).astype(F) + m[2]).astype(F)
        mf = nanmax(ms, F(floor))
        t = (F(tolerance) * mf).astype(F)
        return v <= (t * t).astype(F)


def active(sum, sum_sq, count, n, min_spp, max_spp, tolerance, floor):
    """(npix,) bool: the pixels a pass starting at sample n samples."""
    count = np.asarray(count).reshape(-1)
    if n == 0:
        return np.ones(count.shape, bool)
    here = count == n
    if n < min_spp:
        return here
    if n >= max_spp:
        return np.zeros(count.shape, bool)
    return here & ~converged(sum, sum_sq, n, tolerance, floor)


def converged_f64(sum, sum_sq, n, tolerance, floor):
    """The same rule in float64: (converged, v, t^2), each (npix,)."""
    s, q = np.asarray(sum, np.float64).reshape(3, -1), np.asarray(sum_sq, np.float64).reshape(3, -1)
    m = s / n
    var = np.zeros_like(m) if n < 2 else np.maximum(q / n - m * m, 0.0) / (n - 1)
    v, ms = var.sum(axis=0), m.sum(axis=0)
    t2 = (tolerance * np.maximum(ms, floor)) ** 2
    return v <= t2, v, t2


def schedule(x, passes, min_spp, max_spp, tolerance, floor):
    """x: (N, 3, rows, width) per-sample contributions, N >= sum(passes).
    Returns (sum, sum_sq, count, actives): the planes (3, rows, width) float32
    and count (rows, width) after the passes, and each pass's active mask."""
    x = np.asarray(x, F)
    shape = x.shape[1:]
    s, q = np.zeros(shape, F), np.zeros(shape, F)
    count = np.zeros(shape[1:], np.int64)
    actives, base = [], 0
    for spp in passes:
        act = active(s, q, count, base, min_spp, max_spp, tolerance, floor).reshape(shape[1:])
        actives.append(act)
        if act.any():
            for k in range(base, base + spp):
                s = np.where(act, (s + x[k]).astype(F), s)
                q = np.where(act, (q + (x[k] * x[k]).astype(F)).astype(F), q)
            count = np.where(act, base + spp, count)
            base += spp
    return s, q, count, actives
