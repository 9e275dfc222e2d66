"""The per-column summary of include/kidmp_summary.h in numpy, for the tests: the 15 numbers of a state from a dBZ profile
and an re_qc profile with its "formed" mask (those of the oracles, or the library's own profiles passed in), every sum
taken with math.fsum.  Each sum comes back with the sum of the magnitudes of its terms, which is what its error bound is
stated in: the terms are correctly rounded IEEE operations in the order of the header, so numpy forms them bit for bit, and
any summation order of nz terms errs by at most (nz - 1) * 2**-53 * sum|term|."""
import math

import numpy as np

import refl_oracle as ro

N = 16
NAMES = ("wvp", "cwp", "rwp", "iwp", "swp", "gwp", "tau_c", "dbz_max", "z_dbz_max", "z_echo_top", "dbz_sfc",
         "z_cloud_base", "z_cloud_top", "n_cloud", "z_freeze")
WVP, CWP, RWP, IWP, SWP, GWP, TAU_C, DBZ_MAX, Z_DBZ_MAX, Z_ECHO_TOP, DBZ_SFC, Z_CLOUD_BASE, Z_CLOUD_TOP, N_CLOUD, Z_FREEZE = range(15)
SUMS = (WVP, CWP, RWP, IWP, SWP, GWP, TAU_C)
HEIGHTS = (Z_DBZ_MAX, Z_ECHO_TOP, Z_CLOUD_BASE, Z_CLOUD_TOP, Z_FREEZE)
DEFAULT_CFG = (18.0, 1.0e-5, 273.15)
R_GAS = 287.04
RE_QC_PRESET = 2.49e-6
EPS = 2.0 ** -53
BOUND_DB = 3e-13                                   # test_gpu_reflectivity.py
BOUND_RE = 1e-12                                   # test_gpu_column_outputs.py
INPUTS = ("t", "p", "qv", "qc", "nc", "qi", "qr", "nr", "qs", "qg")


def oracle_dbz(consts, st):
    return ro.of_state(consts, {k: st.get(k) for k in ("t", "p", "qv", "qr", "nr", "qs", "qg")})


def oracle_re_qc(oracle, st):
    """(re_qc, formed) of Oracle.calc_effectRad started from the presets: formed <=> the value is not the preset."""
    z = np.zeros_like(st["t"])
    full = {k: (st[k] if st.get(k) is not None else z) for k in ("t", "p", "qv", "qc", "nc", "qi", "ni", "qs")}
    re = oracle.calc_effectRad(full)[0]
    return re, re != RE_QC_PRESET


def _broadcast_dz(dz, shape):
    dz = np.asarray(dz, dtype=np.float64)
    return np.broadcast_to(dz, shape) if dz.ndim == 1 else dz


def terms(st, dz, re_qc, formed):
    """[7, ncol, nz]: the terms of slots 0-6 in the arithmetic of the header."""
    t, p = st["t"].astype(np.float64), st["p"].astype(np.float64)
    qv = np.maximum(1e-10, st["qv"].astype(np.float64))
    rho = 0.622 * p / (R_GAS * t * (qv + 0.622))
    dz = _broadcast_dz(dz, t.shape)
    zero = np.zeros_like(t)
    g = lambda k: st[k].astype(np.float64) if st.get(k) is not None else zero   # noqa: E731
    out = [rho * qv * dz] + [rho * g(k) * dz for k in ("qc", "qr", "qi", "qs", "qg")]
    with np.errstate(divide="ignore", invalid="ignore"):
        out.append(np.where(formed, 1.5 * out[1] / (1000.0 * re_qc), 0.0))
    return np.stack(out)


def levels(st, dbz, cfg=DEFAULT_CFG):
    """[ncol, 5] int: the levels of slots 8, 9, 11, 12, 14 (-1: none), and n_cloud [ncol]."""
    dbz_echo, q_cloud, t_freeze = cfg
    ncol, nz = dbz.shape
    qi = st["qi"].astype(np.float64) if st.get("qi") is not None else 0.0
    cloudy = st["qc"].astype(np.float64) + qi > q_cloud
    echo = dbz >= dbz_echo
    frozen = st["t"].astype(np.float64) < t_freeze
    first = lambda m: np.where(m.any(axis=1), m.argmax(axis=1), -1)                 # noqa: E731
    last = lambda m: np.where(m.any(axis=1), nz - 1 - m[:, ::-1].argmax(axis=1), -1)   # noqa: E731
    k = np.stack([dbz.argmax(axis=1), last(echo), first(cloudy), last(cloudy), first(frozen)], axis=1)
    return k, cloudy.sum(axis=1)


def summary(st, dz, dbz, re_qc, formed, cfg=DEFAULT_CFG):
    """(out [ncol, 16], mag [ncol, 16], k [ncol, 5]): the summary, for slots 0-6 the sum of |term| and for the height slots
    the sum of dz (0 elsewhere), and the chosen levels."""
    ncol, nz = dbz.shape
    tm = terms(st, dz, re_qc, formed)
    dzb = _broadcast_dz(dz, (ncol, nz))
    k, ncloud = levels(st, dbz, cfg)
    out, mag = np.zeros((ncol, N)), np.zeros((ncol, N))
    for c in range(ncol):
        for s in SUMS:
            out[c, s] = math.fsum(tm[s, c])
            mag[c, s] = math.fsum(np.abs(tm[s, c]))
        col_dz = dzb[c]
        below = lambda kk: math.fsum(col_dz[:kk])                                   # noqa: E731
        kmax, kecho, kbase, ktop, kfrz = (int(x) for x in k[c])
        out[c, DBZ_MAX], out[c, DBZ_SFC] = dbz[c, kmax], dbz[c, 0]
        out[c, Z_DBZ_MAX] = math.fsum(list(col_dz[:kmax]) + [0.5 * col_dz[kmax]])
        out[c, Z_ECHO_TOP] = below(kecho + 1) if kecho >= 0 else np.nan
        out[c, Z_CLOUD_BASE] = below(kbase) if kbase >= 0 else np.nan
        out[c, Z_CLOUD_TOP] = below(ktop + 1) if ktop >= 0 else np.nan
        out[c, Z_FREEZE] = math.fsum(list(col_dz[:kfrz]) + [0.5 * col_dz[kfrz]]) if kfrz >= 0 else np.nan
        out[c, N_CLOUD] = float(ncloud[c])
        mag[c, list(HEIGHTS)] = math.fsum(col_dz)
    return out, mag, k


def check(got, want, mag, nz, extra_tau=0.0, db_bound=0.0, skip_levels=None):
    """Assert `got` [ncol, 16] against the reference under the rules of the tests: a summed slot and a height within
    (nz + 4) * 2**-53 * mag (TAU_C: + extra_tau * mag, the bound of oracle radii), the dBZ slots within db_bound (0: equal
    bits), NaN where the reference has NaN, n_cloud and slot 15 exact.  skip_levels: columns whose level choice the
    reference cannot decide (slots 8 and 9 are then not compared).  Returns the worst error in units of its bound."""
    assert got.shape == want.shape and got.dtype == np.float64
    worst = 0.0
    ok = np.ones(got.shape[0], dtype=bool) if skip_levels is None else ~skip_levels
    for s in SUMS + HEIGHTS:
        rows = ok if s in (Z_DBZ_MAX, Z_ECHO_TOP) else np.ones_like(ok)
        g, w, m = got[rows, s], want[rows, s], mag[rows, s]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (NAMES[s], np.flatnonzero(np.isnan(g) != np.isnan(w))[:5])
        f = ~np.isnan(w)
        bound = ((nz + 4) * EPS + (extra_tau if s == TAU_C else 0.0)) * m[f]
        err = np.abs(g[f] - w[f])
        bad = err > bound
        assert not bad.any(), "%s: column %d got %r, want %r, bound %.3e" % (
            NAMES[s], np.flatnonzero(bad)[0], g[f][bad][0], w[f][bad][0], bound[bad][0])
        if err.size and (bound > 0).any():
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    for s in (DBZ_MAX, DBZ_SFC):
        if db_bound:
            assert np.max(np.abs(got[:, s] - want[:, s])) <= db_bound, NAMES[s]
        else:
            assert np.array_equal(got[:, s].view(np.uint64), want[:, s].view(np.uint64)), NAMES[s]
    assert np.array_equal(got[:, N_CLOUD], want[:, N_CLOUD])
    assert np.array_equal(got[:, 15].view(np.uint64), np.zeros(got.shape[0], dtype=np.uint64))
    return worst


def undecidable(dbz, dbz_echo=DEFAULT_CFG[0], margin=1e-9):
    """[ncol] bool: columns where a dBZ profile known to `margin` cannot decide the levels of slots 8 and 9: a level within
    the margin of dbz_echo, or a maximum less than the margin above the runner-up in a column that is not empty."""
    near = (np.abs(dbz - dbz_echo) <= margin).any(axis=1)
    top2 = np.sort(dbz, axis=1)[:, -2:]
    empty = dbz.max(axis=1) == dbz.min(axis=1)              # every level at the floor of calc_refl10cm
    return near | ((top2[:, 1] - top2[:, 0] <= margin) & ~empty)
