"""The bright band of include/kidmp_brightband.h restated in numpy, binary64, for arrays [ncol, nz]: the checker of
kidmp::k_bright_band.  The load, ze_x, rs, rg and graupel's slope and intercept come from tests/refl_oracle.py (ze_terms),
snow's smob and smoc from tests/doppler_ref.py (snow_smoc), the densities per bin are those of tests/size_spectra_ref.py
(spectrum) written for one bin; new here are the melting level, the melt fractions, the per-particle dielectric model --
complex arithmetic written out in real and imaginary parts, operation for operation as kidmp_brightband_mix.h has it --
and the sums in the kernel's order: lane j takes bins j, j+64, ... ascending, the 64 partial sums meet in a butterfly
over xor 32, 16, ..., 1.
"""
import math

import numpy as np

import doppler_ref as dr
import refl_oracle as ro

NAMES = ("dbz", "dbz_s", "dbz_g", "enh_s", "enh_g", "fmelt_s", "fmelt_g", "k0")
PROFILES = NAMES[:-1]
SPECIES = ("s", "g")
INPUTS = dr.INPUTS
EXP_MAX = 700.0
WATER_MATRIX, ICE_MATRIX = 0, 1


def default_eps_i():
    k = math.sqrt(0.176)
    return (1.0 + 2.0 * k) / (1.0 - k)


def default_cfg(**over):
    cfg = dict(eps_w=complex(79.5, 24.9), eps_i=default_eps_i(), rho_w=1000.0, rho_i=900.0, kw2=0.93, topology=WATER_MATRIX)
    cfg.update(over)
    return cfg


def exp_neg(x):
    """EXP(-x), exact +0.0 where x exceeds EXP_MAX (or is a NaN)."""
    with np.errstate(invalid="ignore", under="ignore"):
        return np.where(x <= EXP_MAX, np.exp(-np.where(x <= EXP_MAX, x, 0.0)), 0.0)


# ---- the per-particle model: kidmp_brightband_mix.h ----
def cdiv(ar, ai, br, bi):
    r = 1.0 / (br * br + bi * bi)
    return (ar * br + ai * bi) * r, (ai * br - ar * bi) * r


def cK(er, ei):
    return cdiv(er - 1.0, ei, er + 2.0, ei)


def k_ice(cfg):
    return (cfg["eps_i"] - 1.0) / (cfg["eps_i"] + 2.0)


def bin_consts(cfg, x, D):
    """m, Vi0, Ve, dry of a bin of species x ('s' or 'g') at diameter D."""
    m = ro.am_s * (D * D) if x == "s" else ro.am_g * (D * D * D)
    Vi0 = m / cfg["rho_i"]
    Ve = np.maximum((ro.PI / 6.0) * D * D * D, Vi0)
    ki = k_ice(cfg)
    return m, Vi0, Ve, ki * ki * Vi0 * Vi0


def wet(cfg, b, fm):
    """|K(eps_p)|**2 * V * V of the bin b = bin_consts(...) at melt fraction fm (array or number)."""
    m, Vi0, Ve, _ = b
    ew = complex(cfg["eps_w"])
    ki = k_ice(cfg)
    dryf = 1.0 - fm
    Vi = dryf * Vi0
    Vw = (fm * m) / cfg["rho_w"]
    Va = dryf * (Ve - Vi0)
    c = Vi + Va
    V = c + Vw
    with np.errstate(all="ignore"):
        Kc = np.where(c > 0.0, (Vi / np.where(c > 0.0, c, 1.0)) * ki, 0.0)
        eps_c = (1.0 + 2.0 * Kc) / (1.0 - Kc)
        if cfg["topology"] == WATER_MATRIX:
            g = c / V
            br, bi = cdiv(eps_c - ew.real, -ew.imag, eps_c + 2.0 * ew.real, 2.0 * ew.imag)
        else:
            g = Vw / V
            br, bi = cdiv(ew.real - eps_c, ew.imag, ew.real + 2.0 * eps_c, ew.imag)
        gr, gi = g * br, g * bi
        qr, qi = cdiv(1.0 + 2.0 * gr, 2.0 * gi, 1.0 - gr, -gi)
        if cfg["topology"] == WATER_MATRIX:
            er, ei = ew.real * qr - ew.imag * qi, ew.real * qi + ew.imag * qr
        else:
            er, ei = eps_c * qr, eps_c * qi
        kr, kim = cK(er, ei)
        return (kr * kr + kim * kim) * V * V


# ---- the level part ----
def melting_level(temp, L_qr, L_qs, L_qg):
    """k0 [ncol]: k + 1 of the highest k in [0, nz-2] with warm rain under snow or graupel (M:5109-5118), else -1."""
    ncol, nz = temp.shape
    k0 = np.full(ncol, -1, dtype=np.int32)
    for k in range(nz - 2, -1, -1):
        hit = (temp[:, k] > 273.15) & L_qr[:, k] & (L_qs[:, k + 1] | L_qg[:, k + 1]) & (k0 < 0)
        k0[hit] = k + 1
    return k0


def melt_fraction(k0, L, r):
    """fm [ncol, nz] of a species with presence L and content r: M:5152 / M:5176, +0.0 where the species is dry."""
    ncol, nz = r.shape
    kk = np.arange(nz)[None, :]
    at = np.maximum(k0, 0)
    r0 = r[np.arange(ncol), at][:, None]
    L0 = L[np.arange(ncol), at][:, None]
    act = (k0[:, None] >= 0) & (kk < k0[:, None]) & L & L0
    with np.errstate(all="ignore"):
        fm = np.maximum(0.05, np.minimum(1.0 - r / r0, 0.99))
    return np.where(act, fm, 0.0)


def density(x, p, D, dD):
    """n = N_x(D)*dD of every level for the bin: the formulas of size_spectra_ref.spectrum."""
    with np.errstate(all="ignore"):
        if x == "s":
            r = p["smob"] / p["smoc"]
            Mrat = p["smob"] * r * r * r
            return Mrat * (dr.Kap0 * exp_neg(r * dr.Lam0 * D) + dr.Kap1 * r ** dr.mu_s * D ** dr.mu_s * exp_neg(r * dr.Lam1 * D)) * dD
        return p["N0"] * exp_neg(p["lam"] * D) * dD


def butterfly(part):
    """The sum of part[64, ...] as the wave forms it: xor 32, 16, ..., 1; every lane ends with the same bits."""
    idx = np.arange(64)
    v = part
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[idx ^ m]
    return v[0]


def enhancement(cfg, x, p, fm, D, dD):
    """E_x [ncol, nz]: (sum n s)/(sum n s0) in the kernel's order where fm > 0, exactly 1.0 elsewhere."""
    act = fm > 0.0
    num, den = np.zeros((64,) + fm.shape), np.zeros((64,) + fm.shape)
    f = np.where(act, fm, 0.5)
    for b in range(len(D)):
        bc = bin_consts(cfg, x, D[b])
        n = density(x, p, D[b], dD[b])
        with np.errstate(all="ignore"):
            num[b % 64] += n * wet(cfg, bc, f)
            den[b % 64] += n * bc[3]
    num, den = butterfly(num), butterfly(den)
    with np.errstate(all="ignore"):
        ok = act & (den > 0.0)
        return np.where(ok, num / np.where(ok, den, 1.0), 1.0)


def bright_band(c, st, cfg=None, grids=None, default=None, warm=False):
    """Every output of NAMES for a state dict (numpy [ncol, nz]; missing or None qs / qg = 0); grids: species ->
    (D, dD), a species without an entry takes default[species].  Also the locals ze_r, ze_s, ze_g."""
    cfg = default_cfg() if cfg is None else cfg
    z = np.zeros_like(np.asarray(st["t"], dtype=np.float64))
    g = lambda k: np.asarray(st[k], dtype=np.float64) if st.get(k) is not None else z   # noqa: E731
    ze_r, ze_s, ze_g, v, ilamg, N0_g = ro.ze_terms(c, g("qv"), g("qr"), g("nr"), g("qs"), g("qg"), g("t"), g("p"))
    k0 = melting_level(v["temp"], v["L_qr"], v["L_qs"], v["L_qg"])
    if warm:
        k0[:] = -1
    fm_s = melt_fraction(k0, v["L_qs"], v["rs"])
    fm_g = melt_fraction(k0, v["L_qg"], v["rg"])
    with np.errstate(all="ignore"):
        smoc, smob = dr.snow_smoc(c, v["temp"], v["rs"])
        par = {"s": dict(smob=smob, smoc=smoc), "g": dict(N0=N0_g, lam=1.0 / ilamg)}
    grid = {x: (grids or {}).get(x) or default[x] for x in SPECIES}
    e_s = enhancement(cfg, "s", par["s"], fm_s, *grid["s"])
    e_g = enhancement(cfg, "g", par["g"], fm_g, *grid["g"])
    zs, zg = ze_s * e_s, ze_g * e_g
    dbz_of = lambda ze: 10.0 * np.log10(ze * 1.e18)   # noqa: E731
    return dict(dbz=dbz_of(ze_r + zs + zg), dbz_s=dbz_of(zs), dbz_g=dbz_of(zg), enh_s=e_s, enh_g=e_g, fmelt_s=fm_s, fmelt_g=fm_g,
                k0=k0, ze_r=ze_r, ze_s=ze_s, ze_g=ze_g)
