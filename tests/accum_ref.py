"""numpy restatement of spt_render_accum's sums, film and variance
(include/spt.h), written from the definition, not from the kernels.

The per-sample contributions x_s come from the oracle, one sample at a time
(oracle_trace_sample's L3); everything else is restated here in float32, one
rounded operation at a time:

  sum    = (((0 + x_0) + x_1) + ...)            in sample order
  sum_sq = (((0 + x_0 x_0) + x_1 x_1) + ...)    each product rounded first
  film   = sum / n
  m = sum / n,  q = sum_sq / n,  variance = 0 if n < 2 else max(q - m m, 0) / (n - 1)
"""
import ctypes

import numpy as np

import oracle as O

F = np.float32


def contributions(osc, p, rows=None):
    """x[s] for every pixel of `rows` (default: all) of the oracle scene under
    OracleParams p: (spp, 3, len(rows), width) float32."""
    rows = range(p.height) if rows is None else rows
    rows = [int(r) for r in rows]
    x = np.zeros((p.spp, 3, len(rows), p.width), F)
    rays = np.zeros((p.max_depth, 6), F)
    ids = np.zeros(p.max_depth, np.int32)
    tuv = np.zeros((p.max_depth, 3), F)
    L = np.zeros(3, F)
    for i, y in enumerate(rows):
        for px in range(p.width):
            for s in range(p.spp):
                O.lib.oracle_trace_sample(osc.h, ctypes.byref(p), px, y, s, rays.ctypes.data, ids.ctypes.data,
                                          tuv.ctypes.data, L.ctypes.data)
                x[s, :, i, px] = L
    return x


def moments(x):
    """(sum, sum_sq, film, variance), each (3, rows, width) float32, of the
    contributions x (n, 3, rows, width) added in sample order."""
    x = np.asarray(x, F)
    n = x.shape[0]
    s = np.zeros(x.shape[1:], F)
    q = np.zeros(x.shape[1:], F)
    for k in range(n):
        s = (s + x[k]).astype(F)
        q = (q + (x[k] * x[k]).astype(F)).astype(F)
    m = (s / F(n)).astype(F)
    if n < 2:
        var = np.zeros_like(m)
    else:
        qq = (q / F(n)).astype(F)
        var = (np.maximum((qq - (m * m).astype(F)).astype(F), F(0)) / F(n - 1)).astype(F)
    return s, q, m, var


def variance_f64(x):
    """The unbiased variance of the pixel mean in float64 (what `variance` estimates)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    return x.var(axis=0, ddof=1) / n if n > 1 else np.zeros(x.shape[1:])
