"""Operand pairs and exact decisions for kid_amd/csrc/limit_bracket.h, shared by test_limit_bracket.py (host build of the
header) and test_gpu_limit_bracket.py (the device's bracket and the column kernel's original expression).

A site tests xD = c / cbrt(num / den) against D_lo < D_hi.  With r = num / den and T = (c / D)**3, all rationals:
    xD < D_lo  <=>  r > T_lo        xD > D_hi  <=>  r < T_hi        (T_hi < T_lo)
The constants come from the header itself (limit_bracket_eval consts prints them as hexadecimal floats)."""
import os
import subprocess
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BELOW, INSIDE, ABOVE, AMBIGUOUS = 0, 1, 2, 3
ULPS = (0, 1, -1, 2, -2, 8, -8, 64, -64, 4096, -4096)
SITES = (0, 1, 2, 9, 15)            # ice, rain, cloud droplets with nu = 2, 9, 15 (the ends and the middle of 2 .. 15)


def build_driver(workdir, extra=()):
    exe = os.path.join(str(workdir), "limit_bracket_eval")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "kid_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "limit_bracket_eval.cpp"),
                           os.path.join(ROOT, "kid_amd", "csrc", "thompson_host_init.cpp"), "-o", exe])
    return exe


def constants(exe):
    out = subprocess.run([exe, "consts"], check=True, capture_output=True, text=True).stdout
    return {k: float.fromhex(v) for k, v in (l.split() for l in out.splitlines())}


def host_answers(exe, workdir, num, den, site):
    fin, fout = os.path.join(str(workdir), "lb_in.bin"), os.path.join(str(workdir), "lb_out.bin")
    with open(fin, "wb") as f:
        f.write(np.int64(num.size).tobytes())
        for a in (num, den, site):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    subprocess.check_call([exe, fin, fout])
    out = np.fromfile(fout, dtype=np.int32)
    assert np.array_equal(out // 4 == 1, out % 4 == INSIDE)     # certainly_inside(): decide() == INSIDE and nothing else
    return out % 4


def thresholds(consts, site):
    """(T_lo, T_hi) as Fractions: the exact cubes of c / D_lo and c / D_hi of the site's binary64 constants"""
    name = "ice" if site == 0 else "rain" if site == 1 else "cloud"
    c = Fraction(consts["cloud_c_%d" % site] if site >= 2 else consts[name + "_c"])
    return (c / Fraction(consts[name + "_D_lo"])) ** 3, (c / Fraction(consts[name + "_D_hi"])) ** 3


def adjacent_pairs(consts, site, ndens, rng):
    """num = the binary64 nearest to T * den, moved by every offset of ULPS, for both thresholds and `ndens` values of
    den (the floors R1 and its successor among them): the pairs on which the two ways of deciding could disagree"""
    dens = np.concatenate([[consts["R1"], np.nextafter(consts["R1"], 1.0)], 10.0 ** rng.uniform(-12.0, -1.0, ndens - 2)])
    num, den = [], []
    for T in thresholds(consts, site):
        for d in dens:
            n0 = np.float64(float(T * Fraction(float(d))))                  # Fraction -> float rounds correctly
            for k in ULPS:
                num.append((n0.view(np.int64) + np.int64(k)).view(np.float64))
                den.append(d)
    return np.array(num), np.array(den)


def floor_pairs(consts, site, ndens, rng):
    """num at the site's number floor -- K R2 for ice and rain (n = fmax(R2, ...)), 2 K(nu) for the droplets
    (fmax(2., ...)), K as the kernel forms it -- and its neighbours 0, +-1, +-2 ulp; den = R1, its successor, `ndens`
    log-uniform values over [1e-12, 1e-1], and for both thresholds the den that puts the floor 0, +-1, +-64, +-4096 ulp
    (of den) around the exact threshold"""
    n0 = np.float64(consts["floor_num_%d" % site])
    nums = [(n0.view(np.int64) + np.int64(k)).view(np.float64) for k in (0, 1, -1, 2, -2)]
    dens = [consts["R1"], np.nextafter(consts["R1"], 1.0)] + list(10.0 ** rng.uniform(-12.0, -1.0, ndens))
    for T in thresholds(consts, site):
        d0 = np.float64(float(Fraction(float(n0)) / T))
        dens += [(d0.view(np.int64) + np.int64(k)).view(np.float64) for k in (0, 1, -1, 64, -64, 4096, -4096)]
    num, den = np.meshgrid(np.array(nums), np.array(dens))
    return num.ravel(), den.ravel()


def log_uniform_pairs(consts, site, n, rng):
    """num / den log-uniform over 30 decades around the two thresholds, den log-uniform over [1e-12, 1e-1]"""
    T_lo, T_hi = thresholds(consts, site)
    mid = 0.5 * (np.log10(float(T_lo)) + np.log10(float(T_hi)))
    den = 10.0 ** rng.uniform(-12.0, -1.0, n)
    return 10.0 ** rng.uniform(mid - 15.0, mid + 15.0, n) * den, den


def outside_domain(consts):
    """zeros, negatives, non-finite and absurd operands: the bracket hands them to the original path"""
    bad = [0.0, -1.0, np.inf, np.nan, consts["LIM_TINY"] * 0.5, consts["LIM_HUGE"] * 2.0]
    num = np.array(bad + [1.0] * len(bad) + [0.0])
    den = np.array([1.0] * len(bad) + bad + [0.0])
    return num, den


def exact_classes(consts, site, num, den, rel=0.0):
    """The decision in exact arithmetic, as two boolean arrays per threshold: (below, not_below, above, not_above) hold
    for EVERY xD (1 + e), |e| <= rel (rel = 0: the exact decision, where not_below = ~below).  Pairs further than 1e-6
    (relative) from both thresholds are classified in longdouble, whose 1e-19 error cannot matter there; the others in
    Fractions."""
    T_lo, T_hi = thresholds(consts, site)
    up, dn = (1 + Fraction(rel)) ** 3, (1 - Fraction(rel)) ** 3
    r = num.astype(np.longdouble) / den.astype(np.longdouble)
    out = []
    for T, below_means_greater in ((T_lo, True), (T_hi, False)):
        Tl = np.longdouble(T.numerator) / np.longdouble(T.denominator)
        gt, lt = r > Tl, r < Tl                                             # far pairs: r > T (1 + rel)**3 etc. follow
        near = np.abs(r / Tl - 1) < 1e-6
        for i in np.nonzero(near)[0]:
            ri = Fraction(float(num[i])) / Fraction(float(den[i]))
            if below_means_greater:
                gt[i], lt[i] = ri > T * up, ri <= T * dn                    # xD (1 + e) < D for all e / for no e
            else:
                lt[i], gt[i] = ri < T * dn, ri >= T * up                    # xD (1 + e) > D for all e / for no e
        out += [gt, lt] if below_means_greater else [lt, gt]
    return tuple(out)


def distance_to_thresholds(consts, site, num, den):
    """min over the two thresholds of |num / (den T) - 1|, in longdouble (compared with EPS ~ 5e-14: ample)"""
    r = num.astype(np.longdouble) / den.astype(np.longdouble)
    d = [np.abs(r / (np.longdouble(T.numerator) / np.longdouble(T.denominator)) - 1) for T in thresholds(consts, site)]
    return np.minimum(d[0], d[1]).astype(np.float64)
