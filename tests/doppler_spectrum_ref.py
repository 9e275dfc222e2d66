"""The Doppler spectrum of include/kidmp_dspectrum.h restated in numpy, binary64, for arrays [ncol, nz]: the checker of
kidmp::k_doppler_spectrum.  The load, ze_x, the slopes and the intercepts come from tests/refl_oracle.py (ze_terms) and
tests/doppler_ref.py (snow_smoc), so the load is the existing checker's; new here are the reflectivity of a diameter
bin, its fall speed, and the linear deposit on the velocity grid, in the kernel's order: rain's bins ascending, then
snow's, then graupel's.  Constants that thompson_init does not hold come from math.gamma.
"""
import math

import numpy as np

import doppler_ref as dr
import refl_oracle as ro

NAMES = ("total", "rain", "snow", "graupel", "below", "above")
SPECIES = ("r", "s", "g")
INPUTS = dr.INPUTS
EXP_MAX = 700.0
G = math.gamma
NS = 2.0 * dr.bm_s + 1.0                                        # 5: the order of the reflectivity moment of snow, plus one
IA00 = 1.0 / (dr.Kap0 * G(NS) * dr.Lam0 ** -NS + dr.Kap1 * G(NS + dr.mu_s) * dr.Lam1 ** -(NS + dr.mu_s))
ZE_GRAUPEL_FAC = (0.176 / 0.93) * (6.0 / ro.PI) * (6.0 / ro.PI) * (ro.am_g / 900.0) * (ro.am_g / 900.0)


def exp_neg(x):
    """EXP(-x), exact +0.0 where x exceeds EXP_MAX (or is a NaN)."""
    with np.errstate(invalid="ignore", under="ignore"):
        return np.where(x <= EXP_MAX, np.exp(-np.where(x <= EXP_MAX, x, 0.0)), 0.0)


def bin_speed(x, D):
    """vfac_b: the fall speed of diameter D in air of density rho_not."""
    if x == "r":
        return dr.av_r * D ** dr.bv_r * exp_neg(dr.fv_r * D)
    if x == "s":
        return dr.av_s * D ** dr.bv_s * exp_neg(dr.fv_s * D)
    return dr.av_g * D ** dr.bv_g


def levels(c, st):
    """What a level keeps of each species: present [..], the factors of echo(), rhof, and ze_x for the tests."""
    z = np.zeros_like(np.asarray(st["t"], dtype=np.float64))
    g = lambda k: np.asarray(st[k], dtype=np.float64) if st.get(k) is not None else z   # noqa: E731
    ze_r, ze_s, ze_g, v, ilamg, N0_g = ro.ze_terms(c, g("qv"), g("qr"), g("nr"), g("qs"), g("qg"), g("t"), g("p"))
    with np.errstate(all="ignore"):
        smoc, smob = dr.snow_smoc(c, v["temp"], v["rs"])
        Mrat = smob / smoc
        lv = dict(rhof=np.sqrt(dr.RHO_NOT / v["rho"]),
                  r=dict(present=v["L_qr"], A=v["N0_r"], lam=1.0 / v["ilamr"], ze=ze_r),
                  g=dict(present=v["L_qg"], A=ZE_GRAUPEL_FAC * N0_g, lam=1.0 / ilamg, ze=ze_g),
                  s=dict(present=v["L_qs"], zs=ze_s * (Mrat ** 5 * IA00), x0=Mrat * dr.Lam0, x1=Mrat * dr.Lam1,
                         k1=dr.Kap1 * Mrat ** dr.mu_s, ze=ze_s, Mrat=Mrat))
    return lv


def echo(x, p, D, dD):
    """z_b of species x at every level for the bin (D, dD): +0.0 where the species is absent."""
    with np.errstate(all="ignore"):
        if x == "s":
            z = (p["zs"] * (dr.Kap0 * exp_neg(p["x0"] * D) + (p["k1"] * D ** dr.mu_s) * exp_neg(p["x1"] * D))) * (D ** 4 * dD)
        else:
            z = (p["A"] * exp_neg(p["lam"] * D)) * (D ** 6 * dD)
    return np.where(p["present"], z, 0.0)


def slot(p, nv):
    """(j, f) of positions p: j in [-1, nv-1], f in [0, 1]; a NaN lies in `below`."""
    with np.errstate(invalid="ignore"):
        q = np.where(~(p >= -1.0), -1.0, np.where(p > nv, float(nv), p))
    j = np.minimum(np.floor(q), nv - 1.0)
    return j.astype(np.int64), q - j


def deposit(targets, present, z, v, v0, idv, nv):
    """Adds the bin's z at velocity v to the slots of every array [ncol, nv+2, nz] in `targets` (slot s holds bin s-1;
    0 = below, nv+1 = above)."""
    j, f = slot((v - v0) * idv, nv)
    c, k = np.nonzero(present)
    jj, ff, zz = j[c, k], f[c, k], z[c, k]
    lo, hi = (1.0 - ff) * zz, ff * zz
    for S in targets:
        S[c, jj + 1, k] += lo
        S[c, jj + 2, k] += hi


def doppler_spectrum(c, st, v0, dv, nv, w=None, grids=None, default=None, want=NAMES):
    """The outputs of `want` of a state dict (numpy [ncol, nz]); grids: species -> (D, dD), a species without an entry
    takes `default[species]`.  Also returns under "sum_r/s/g" the sums of z_b per level, the scale of the tests' bounds."""
    lv = levels(c, st)
    shape = lv["rhof"].shape
    wind = np.zeros(shape) if w is None else np.asarray(w, dtype=np.float64)
    idv = 1.0 / dv
    grid = {x: (grids or {}).get(x) or default[x] for x in SPECIES}
    name_of = {"r": "rain", "s": "snow", "g": "graupel"}
    out = {}
    need_total = any(n in want for n in ("total", "below", "above"))
    total = np.zeros((shape[0], nv + 2, shape[1])) if need_total else None
    for x in SPECIES:                                         # every accumulator receives its terms in the kernel's order
        D, dD = grid[x]
        own = np.zeros((shape[0], nv + 2, shape[1])) if name_of[x] in want else None
        out["sum_" + x] = np.zeros(shape)
        for b in range(len(D)):
            z = echo(x, lv[x], D[b], dD[b])
            out["sum_" + x] += z
            with np.errstate(all="ignore"):
                v = lv["rhof"] * bin_speed(x, D[b]) - wind
            deposit([S for S in (total, own) if S is not None], lv[x]["present"], z, v, v0, idv, nv)
        if own is not None:
            out[name_of[x]] = np.ascontiguousarray(own[:, 1:nv + 1, :])
    if need_total:
        out["total"] = np.ascontiguousarray(total[:, 1:nv + 1, :])
        out["below"], out["above"] = np.ascontiguousarray(total[:, 0, :]), np.ascontiguousarray(total[:, nv + 1, :])
    out["levels"] = lv
    return out


def deposit_broadening(c, st, v0, dv, nv, w=None, grids=None, default=None):
    """By how much the linear deposit widens the total spectrum of every level, in units of dv**2: a mass z split
    (1-f) : f between two bins dv apart has the second moment v**2 + f(1-f) dv**2 about zero where its own is v**2, so the
    spectrum's second moment exceeds that of the bins by dv**2 * sum f(1-f) z_b / sum z_b.  Returns that ratio."""
    lv = levels(c, st)
    wind = np.zeros(lv["rhof"].shape) if w is None else np.asarray(w, dtype=np.float64)
    num, den = np.zeros(lv["rhof"].shape), np.zeros(lv["rhof"].shape)
    for x in SPECIES:
        D, dD = (grids or {}).get(x) or default[x]
        for b in range(len(D)):
            z = echo(x, lv[x], D[b], dD[b])
            with np.errstate(all="ignore"):
                _, f = slot((lv["rhof"] * bin_speed(x, D[b]) - wind - v0) * (1.0 / dv), nv)
            num += f * (1.0 - f) * z
            den += z
    with np.errstate(all="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


# ---- what tests/test_doppler_spectrum_abi.py measures the convergence of the definitions on, and the GPU cross-check
# against doppler_moments reuses: hand-built levels, a fine diameter grid, and the measured figures ----
NL = 8


def hand_levels(x):
    """One column of NL levels that hold species x alone, from a broad distribution (level 0) to a narrow one."""
    st = {k: np.zeros((1, NL)) for k in INPUTS}
    st["t"][:], st["p"][:], st["qv"][:] = np.linspace(268.0, 240.0, NL) if x != "r" else np.linspace(295.0, 275.0, NL), 7.0e4, 1.0e-3
    if x == "r":
        st["qr"][0] = np.geomspace(5.0e-3, 1.0e-5, NL)
        st["nr"][0] = np.geomspace(3.0e1, 3.0e5, NL)
    elif x == "s":
        st["qs"][0] = np.geomspace(3.0e-3, 2.0e-6, NL)
    else:
        st["qg"][0] = np.geomspace(5.0e-3, 2.0e-6, NL)
    return st


def fine_grid():
    """Log-spaced 256 bins over [1e-6 m, 0.3 m]: geometric centres, widths the differences of the edges."""
    edges = np.geomspace(1.0e-6, 0.3, 257)
    return np.sqrt(edges[:-1] * edges[1:]), edges[1:] - edges[:-1]


# |sum z_b/ze - 1|, |sum v z/sum z / vz - 1|, |sum v2 z/sum z / v2 - 1| on fine_grid() over hand_levels(x), as
# test_doppler_spectrum_abi.py measures and asserts them: with a factor two, but no tighter than ROUNDING_FLOOR, because a
# figure at the level of rounding moves by more than its own size with a few ulp of numpy's exp and pow
FINE_MEASURED = {"r": (1.011e-4, 7.6e-14, 7.7e-14), "s": (1.011e-4, 2.03e-10, 2.10e-10), "g": (1.011e-4, 1.1e-15, 2.0e-15)}
ROUNDING_FLOOR = 2e-13
# the bound the GPU cross-check takes from there: twice the largest measured value of each quantity
FINE_BOUND = tuple(2.0 * max(FINE_MEASURED[x][i] for x in "rsg") for i in range(3))


def bin_moments(c, st, x, D, dD):
    """Sum z_b, sum v z_b / sum z_b and sum v**2 z_b / sum z_b of species x in still air, per level, on the grid (D, dD)."""
    lv = levels(c, st)
    s0 = np.zeros(lv["rhof"].shape)
    s1, s2 = s0.copy(), s0.copy()
    for b in range(len(D)):
        z = echo(x, lv[x], D[b], dD[b])
        v = lv["rhof"] * bin_speed(x, D[b])
        s0 += z
        s1 += v * z
        s2 += v * v * z
    with np.errstate(all="ignore"):
        return s0, s1 / s0, s2 / s0
