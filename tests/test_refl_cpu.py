"""Independent checks of the numpy restatement of calc_refl10cm (tests/refl_oracle.py), the checker of the reflectivity
kernel: no GPU needed."""
import math

import numpy as np
import pytest

import refl_oracle as ro

NZ = 12


@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)          # the gamma-function constants do not depend on iiwarm (M:452-553)
    c = ro.constants(o)
    o.close()
    return c


def _column(nz=NZ):
    z = np.linspace(0.0, 11000.0, nz)
    t = 300.0 - 6.5e-3 * z
    p = 1.0e5 * np.exp(-z / 8000.0)
    qv = 0.016 * np.exp(-z / 2500.0)
    zero = np.zeros(nz)
    return dict(t=t, p=p, qv=qv, qr=zero.copy(), nr=zero.copy(), qs=zero.copy(), qg=zero.copy())


def _dbz(c, st):
    return ro.calc_refl10cm(c, st["qv"], st["qr"], st["nr"], st["qs"], st["qg"], st["t"], st["p"])


def test_empty_level_is_three_floors(consts):
    st = _column()
    st["qr"][:] = 1e-12                        # at R1: not rain (M:4998 tests qr1d > R1)
    st["qs"][:] = 1e-6                         # at R2: not snow (M:5012)
    st["qg"][:] = 1e-6                         # at R2: not graupel (M:5019)
    d = _dbz(consts, st)
    assert np.all(np.abs(d - 10.0 * math.log10(3e-4)) < 1e-12), d
    assert abs(ro.EMPTY_DBZ - 10.0 * math.log10(3e-4)) < 1e-12


def _laguerre_moment(n, N0, lam, nodes=40):
    """int_0^inf D**n N0 exp(-lam D) dD by Gauss-Laguerre quadrature in x = lam D."""
    x, w = np.polynomial.laguerre.laggauss(nodes)
    return N0 / lam ** (n + 1) * np.sum(w * x ** n)


def test_rain_and_graupel_distributions_reproduce_their_moments(consts):
    c = consts
    st = _column()
    st["qr"][:] = np.geomspace(1e-7, 5e-3, NZ)
    st["nr"][:] = np.geomspace(1e2, 1e5, NZ)[::-1]
    st["qg"][:] = np.geomspace(2e-6, 8e-3, NZ)
    ze_rain, ze_snow, ze_graupel, v, ilamg, N0_g = ro.ze_terms(c, st["qv"], st["qr"], st["nr"], st["qs"], st["qg"],
                                                               st["t"], st["p"])
    fac_g = (0.176 / 0.93) * (6.0 / ro.PI) ** 2 * (ro.am_g / 900.0) ** 2
    for k in range(NZ):
        # rain: N(D) = N0_r exp(-lamr D) (mu_r = 0, M:65)
        lamr = 1.0 / v["ilamr"][k]
        m3 = _laguerre_moment(3, v["N0_r"][k], lamr)
        assert abs(ro.am_r * m3 / v["rr"][k] - 1.0) < 1e-8                            # rho q_r
        assert abs(_laguerre_moment(0, v["N0_r"][k], lamr) / v["nr"][k] - 1.0) < 1e-8  # number concentration
        assert abs(_laguerre_moment(6, v["N0_r"][k], lamr) / ze_rain[k] - 1.0) < 1e-8
        # graupel: N(D) = N0_g exp(-lamg D) (mu_g = 0)
        lamg = 1.0 / ilamg[k]
        assert abs(ro.am_g * _laguerre_moment(3, N0_g[k], lamg) / v["rg"][k] - 1.0) < 1e-8
        assert abs(fac_g * _laguerre_moment(6, N0_g[k], lamg) / ze_graupel[k] - 1.0) < 1e-8


def test_graupel_intercept_is_a_top_down_running_minimum(consts):
    st = _column()
    st["qg"][:] = 1e-3
    st["qg"][NZ - 2] = 0.0                     # a level without graupel enters the minimum with rg = R1
    v = ro.load(consts, st["qv"], st["qr"], st["nr"], st["qs"], st["qg"], st["t"], st["p"])
    _, N0_g = ro.graupel(consts, v["temp"], v["L_qr"], v["mvd_r"], v["rg"])
    # exponential graupel (mu_g = 0): N0_g equals the (running-minimum) N0_exp, non-increasing downwards from the top
    assert np.all(np.diff(N0_g[::-1]) <= 0)
    # rg = R1 gives ygra1 = 4.31 + log10(5e-5): N0_exp of the empty level sets the minimum for everything below it
    ygra1 = 4.31 + math.log10(5e-5)
    zans1 = 3.1 + (100. / (300. * 0.01 * ygra1 / (10. / 0.01 + 1. + 0.25 * ygra1) + 30. + 10. * ygra1))
    n0_empty = max(ro.gonv_min, min(10.0 ** zans1, ro.gonv_max))
    assert np.all(N0_g[: NZ - 1] <= n0_empty * (1 + 1e-15))


def test_melting_layer_gives_the_dry_formula(consts):
    """Rain below and snow/graupel above the 0 C level is where the reference finds a melting level (M:5107-5121) and
    enters its wet-ice block; with nrbins = 0 that block changes nothing, so every level carries the dry terms."""
    c = consts
    st = _column()
    k0 = int(np.argmax(st["t"] < 273.15))       # first level below freezing
    assert 2 <= k0 < NZ - 2
    st["qr"][:k0] = 1e-3
    st["nr"][:k0] = 3e3
    st["qs"][k0 - 1:] = 5e-4                   # melting snow and graupel reach one level below the 0 C level
    st["qg"][k0 - 1:] = 2e-3
    # the reference's melting-level search finds k_0 > kts here
    L_qr, L_qs, L_qg = st["qr"] > ro.R1, st["qs"] > ro.R2, st["qg"] > ro.R2
    melti = any(st["t"][k] > 273.15 and L_qr[k] and (L_qs[k + 1] or L_qg[k + 1]) for k in range(NZ - 2, -1, -1))
    assert melti
    d = _dbz(c, st)
    # the dry formulas level by level, scalar code
    fac = (0.176 / 0.93) * (6.0 / ro.PI) * (6.0 / ro.PI)
    v = ro.load(c, st["qv"], st["qr"], st["nr"], st["qs"], st["qg"], st["t"], st["p"])
    ilamg, N0_g = ro.graupel(c, v["temp"], v["L_qr"], v["mvd_r"], v["rg"])
    for k in range(NZ):
        zr = v["N0_r"][k] * c["crg"][3] * v["ilamr"][k] ** 7 if L_qr[k] else 1e-22
        zs = 1e-22
        if L_qs[k]:
            tc0 = min(-0.1, st["t"][k] - 273.15)
            x = c["cse"][2]
            terms = [1, tc0, x, tc0 * x, tc0 * tc0, x * x, tc0 * tc0 * x, tc0 * x * x, tc0 ** 3, x ** 3]
            loga = sum(a * t for a, t in zip(ro.sa, terms))
            b = sum(a * t for a, t in zip(ro.sb, terms))
            zs = fac * (ro.am_s / 900.0) ** 2 * 10.0 ** loga * (v["rs"][k] * c["oams"]) ** b
        zg = fac * (ro.am_g / 900.0) ** 2 * N0_g[k] * c["cgg"][3] * ilamg[k] ** 7 if L_qg[k] else 1e-22
        assert abs(d[k] - 10.0 * math.log10((zr + zs + zg) * 1e18)) < 1e-9, k
