"""kid_amd/csrc/limit_bracket.h on the host (no GPU): the header compiled into tests/native/limit_bracket_eval.cpp and
held against exact rational arithmetic (limit_bracket_cases.py).  Per site -- ice, rain, cloud droplets with nu = 2, 9, 15 --
10**5 pairs (num, den): log-uniform over 30 decades, pairs 0, +-1, +-2, +-8, +-64, +-4096 ulp around both exact thresholds
(with den at the floor R1 among them), num at the number floors (K R2 for ice and rain, 2 K(nu) for the droplets, K from
the library's own host init, and its neighbours) against den = R1, a spread of den and the den that puts the floor on
either threshold, and operands outside the domain.

  certain = exact     a BELOW / INSIDE / ABOVE answer is the decision of exact arithmetic
  certain = robust    ... and stays the decision for every xD (1 + e), |e| <= E_X, the header's bound on the original
                      path's error (fm::div, root3 and the last quotient at 1 ulp each): whatever a cube root and a
                      division within their tested bounds return, the original path decides the same
  ambiguity is rare   AMBIGUOUS only within EPS (1 + 2**-40) + BOUND of a threshold or outside the domain; at most 1e-3 of
                      the log-uniform pairs (in fact none is expected: the sliver is 1e-13 of 30 decades)
  the margin          EPS = 16 BOUND, BOUND = E_X cubed plus the bracket's own roundings, as the header derives them"""
import numpy as np
import pytest

import limit_bracket_cases as lc

N_PAIRS = 100000
N_DENS = 200                                    # x 2 thresholds x 11 offsets = 4 400 threshold-adjacent pairs per site


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("lbeval")
    exe = lc.build_driver(d)
    return exe, d, lc.constants(exe)


def test_margin_is_the_derived_one(driver):
    _, _, c = driver
    u = 2.0 ** -53
    assert c["E_X"] == 6 * u                    # 2/3 u (quotient through the root) + 2 u (root3) + 3 u (rcp and product) < 6 u
    assert c["BOUND"] == 3 * c["E_X"] + 8 * u   # the cube triples E_X; T 5 u, T (1 +- EPS) 1 u, the products with den 2 u
    assert c["EPS"] == 16 * c["BOUND"]
    assert c["R1"] == 1e-12 and c["R2"] == 1e-6
    assert all(c["cloud_c_%d" % nu] ** 3 == float(int(c["cloud_c_%d" % nu]) ** 3) < 2 ** 53 for nu in range(2, 16))


@pytest.mark.parametrize("site", lc.SITES)
def test_bracket_against_exact_arithmetic(driver, site):
    exe, d, c = driver
    rng = np.random.default_rng(1000 + site)
    an, ad = lc.adjacent_pairs(c, site, N_DENS, rng)
    fn, fd = lc.floor_pairs(c, site, 100, rng)
    an, ad = np.concatenate([an, fn]), np.concatenate([ad, fd])
    on, od = lc.outside_domain(c)
    un, ud = lc.log_uniform_pairs(c, site, N_PAIRS - an.size - on.size, rng)
    num, den = np.concatenate([un, an, on]), np.concatenate([ud, ad, od])
    assert num.size == N_PAIRS
    got = lc.host_answers(exe, d, num, den, np.full(num.size, float(site)))
    in_domain = np.arange(num.size) < un.size + an.size
    floor = got[un.size + an.size - fn.size:un.size + an.size]
    assert len(set(floor)) >= 3, set(floor)       # the floor pairs meet a limit from both sides and its sliver
    assert (got[~in_domain] == lc.AMBIGUOUS).all()

    num, den, got = num[in_domain], den[in_domain], got[in_domain]
    for rel in (0.0, c["E_X"]):
        below, not_below, above, not_above = lc.exact_classes(c, site, num, den, rel)
        assert below[got == lc.BELOW].all() and above[got == lc.ABOVE].all()
        assert (not_below & not_above)[got == lc.INSIDE].all()
        assert not_above[got == lc.BELOW].all() and not_below[got == lc.ABOVE].all()

    amb = got == lc.AMBIGUOUS
    dist = lc.distance_to_thresholds(c, site, num, den)
    assert (dist[amb] <= c["EPS"] * (1 + 2.0 ** -40) + c["BOUND"]).all(), dist[amb].max()
    assert amb[:un.size].mean() < 1e-3
    # the adjacent pairs do exercise all four answers: +-4096 ulp (9e-13) is outside the sliver, 0 ulp inside it
    adj = got[un.size:un.size + an.size - fn.size]
    assert all((adj == a).any() for a in (lc.BELOW, lc.INSIDE, lc.ABOVE, lc.AMBIGUOUS))
    k = np.tile(np.array(lc.ULPS), adj.size // len(lc.ULPS))
    assert (adj[np.abs(k) == 4096] != lc.AMBIGUOUS).all() and (adj[k == 0] == lc.AMBIGUOUS).all()
