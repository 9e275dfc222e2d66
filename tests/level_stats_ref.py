"""numpy / exact-arithmetic reference of the per-level ensemble statistics (include/kidmp_stats.h) and the rules a result
is judged by, shared by test_level_stats_abi.py (kidmp_stats_merge, no GPU) and test_gpu_level_stats.py.

  exact      count, min, max (as numbers) and every histogram slot equal numpy's
  mean       |mean - fsum mean| <= 4 n 2**-53 max|x|         the worst case of the updating form, times 4
  M2         |M2 - exact M2| / exact M2 <= 8 n kappa 2**-53,  kappa = sqrt(sum x**2 / M2): the Chan-Golub-LeVeque bound of
             the updating algorithm; the exact M2 is formed in integer arithmetic (fractions).  Where the exact M2 is zero
             (one value, a constant cell) the result must be zero.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
NMOM = 5


def cell_values(x, group, g, k):
    """The values of level k of the columns of group g (group None: all in group 0)."""
    if group is None:
        return x[:, k] if g == 0 else x[:0, k]
    return x[group == g, k]


def moment_values(v, floor):
    v = v[np.isfinite(v)]
    return v if floor is None else v[v > floor]


def reference(fields, group, ngroup, edges=None, floors=None):
    """mom [ngroup, nfield, 5, nz] (mean by math.fsum, M2 two-pass by math.fsum) and hist [ngroup, nfield, nz, nbin+3]
    (None without edges) of the list `fields` of [ncol, nz] float64 arrays; edges [nfield, nbin+1]."""
    nfield, nz = len(fields), fields[0].shape[1]
    mom = np.zeros((ngroup, nfield, NMOM, nz))
    mom[:, :, 3, :], mom[:, :, 4, :] = np.inf, -np.inf
    nbin = 0 if edges is None else edges.shape[1] - 1
    hist = np.zeros((ngroup, nfield, nz, nbin + 3), dtype=np.int64) if nbin else None
    for g in range(ngroup):
        for f, x in enumerate(fields):
            for k in range(nz):
                allv = cell_values(x, group, g, k)
                v = moment_values(allv, None if floors is None else floors[f])
                if v.size:
                    mean = math.fsum(v) / v.size
                    mom[g, f, :, k] = (v.size, mean, math.fsum((v - mean) ** 2), v.min(), v.max())
                if nbin:
                    nan = np.isnan(allv)
                    slot = np.searchsorted(edges[f], allv[~nan], side="right")
                    hist[g, f, k, :nbin + 2] = np.bincount(slot, minlength=nbin + 2)
                    hist[g, f, k, nbin + 2] = int(nan.sum())
    return mom, hist


def exact_sums(v):
    """(S1, S2, e): sum x = S1 * 2**e and sum x**2 = S2 * 4**e exactly, as Python integers, of finite float64 values."""
    m, e = np.frexp(v)
    mant = (m * 2.0 ** 53).astype(np.int64).astype(object)            # |m| < 1: exact
    e = e.astype(np.int64) - 53
    e0 = int(e.min())
    ints = mant << (e - e0).astype(object)
    return int(ints.sum()), int((ints * ints).sum()), e0


def exact_m2(v):
    """(M2, sum x**2) of the values as Fractions."""
    s1, s2, e0 = exact_sums(v)
    scale = Fraction(4) ** e0
    return Fraction(s2 * v.size - s1 * s1, v.size) * scale, s2 * scale


def check(got_mom, got_hist, fields, group, ngroup, edges=None, floors=None):
    """Judge a result by the rules at the top.  Returns (worst mean error / bound, worst M2 error / bound)."""
    want_mom, want_hist = reference(fields, group, ngroup, edges, floors)
    assert got_mom.shape == want_mom.shape
    for r, what in ((0, "count"), (3, "min"), (4, "max")):
        assert np.array_equal(got_mom[:, :, r, :], want_mom[:, :, r, :]), what
    if want_hist is None:
        assert got_hist is None
    else:
        assert got_hist.shape == want_hist.shape and got_hist.dtype == np.int64
        assert np.array_equal(got_hist, want_hist), "histogram"
    worst_mean = worst_m2 = 0.0
    nz = fields[0].shape[1]
    for g in range(ngroup):
        for f, x in enumerate(fields):
            for k in range(nz):
                v = moment_values(cell_values(x, group, g, k), None if floors is None else floors[f])
                n, mean, m2 = v.size, got_mom[g, f, 1, k], got_mom[g, f, 2, k]
                if n == 0:
                    assert mean == 0.0 and m2 == 0.0, (g, f, k)
                    continue
                bound = 4.0 * n * U * float(np.max(np.abs(v)))
                err = abs(mean - want_mom[g, f, 1, k])
                assert err <= bound, ("mean", g, f, k, n, err, bound)
                if bound > 0.0:
                    worst_mean = max(worst_mean, err / bound)
                m2e, s2 = exact_m2(v)
                if m2e == 0:
                    assert m2 == 0.0, ("M2 of a constant cell", g, f, k, n, m2)
                    continue
                assert math.isfinite(m2), (g, f, k)
                rel = float(abs(Fraction(m2) - m2e) / m2e)
                bound = 8.0 * n * math.sqrt(float(s2 / m2e)) * U
                assert rel <= bound, ("M2", g, f, k, n, rel, bound)
                worst_m2 = max(worst_m2, rel / bound)
    return worst_mean, worst_m2
