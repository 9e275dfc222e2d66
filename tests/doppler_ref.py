"""The Doppler moments of include/kidmp_doppler.h restated in numpy, binary64, for arrays [..., nz]: the checker of
kidmp::k_doppler_moments.  The load, ze_rain, ze_snow, ze_graupel, the rain slope, the graupel slope with its running
minimum and the snow moment smob come from tests/refl_oracle.py (ze_terms), so the dBZ part is the existing checker.
What is new here are the reflectivity-weighted moments of the fall speed v(D) = rhof*av*D**bv*EXP(-fv*D) in closed form;
the gamma ratios they need are not among thompson_init's arrays and come from math.gamma.

The scheme's run-time constants come from the C oracle's Oracle.const(); the compile-time PARAMETERs are stated below
with their lines.
"""
import math

import numpy as np

import refl_oracle as ro

# ---- PARAMETERs of module_mp_thompson09n ----
R1, R2 = ro.R1, ro.R2
mu_r, mu_g, mu_s = 0.0, 0.0, 0.6357  # M:65, M:66, M:75
Kap0, Kap1, Lam0, Lam1 = 490.6, 17.46, 20.78, 3.29   # M:76-79
bm_s = 2.0                           # M:93
av_r, bv_r, fv_r = 4854.0, 1.0, 195.0   # M:102-104
av_s, bv_s, fv_s = 40.0, 0.55, 100.0    # M:105-107
av_g, bv_g = 442.0, 0.89             # M:108-109
RHO_NOT = 101325.0 / (287.05 * 298.0)   # M:141

NAMES = ("dbz", "vd", "sw", "vz_r", "vz_s", "vz_g", "dbz_r", "dbz_s", "dbz_g")
INPUTS = ("t", "p", "qv", "qr", "nr", "qs", "qg")
G = math.gamma


def constants(oracle):
    """The thompson_init values calc_refl10cm reads (refl_oracle.constants; cse(1) is among them)."""
    return ro.constants(oracle)


# ---- the closed forms, each for arrays; (vz, v2) ----
def rain_moments(rhof, lamr):
    """Gamma PSD N ~ D**mu_r EXP(-lamr D), sigma ~ D**6: n = 7 + mu_r."""
    n = 7.0 + mu_r
    vz = rhof * av_r * (G(n + bv_r) / G(n)) * lamr ** n / (lamr + fv_r) ** (n + bv_r)
    v2 = rhof ** 2 * av_r ** 2 * (G(n + 2 * bv_r) / G(n)) * lamr ** n / (lamr + 2 * fv_r) ** (n + 2 * bv_r)
    return vz, v2


def graupel_moments(rhof, ilamg):
    """N ~ D**mu_g EXP(-D/ilamg), sigma ~ D**6, no exponential in the fall-speed law: n = 7 + mu_g."""
    n = 7.0 + mu_g
    vz = rhof * av_g * (G(n + bv_g) / G(n)) * ilamg ** bv_g
    v2 = rhof ** 2 * av_g ** 2 * (G(n + 2 * bv_g) / G(n)) * ilamg ** (2 * bv_g)
    return vz, v2


def snow_A(Mrat, b, f):
    n = 2.0 * bm_s + 1.0
    return (Kap0 * G(n + b) * (Mrat * Lam0 + f) ** -(n + b)
            + Kap1 * Mrat ** mu_s * G(n + mu_s + b) * (Mrat * Lam1 + f) ** -(n + mu_s + b))


def snow_moments(rhof, Mrat):
    """N ~ Kap0 EXP(-Mrat Lam0 D) + Kap1 (Mrat D)**mu_s EXP(-Mrat Lam1 D) (M:3289-3299), sigma ~ D**(2 bm_s)."""
    a0 = snow_A(Mrat, 0.0, 0.0)
    return rhof * av_s * snow_A(Mrat, bv_s, fv_s) / a0, rhof ** 2 * av_s ** 2 * snow_A(Mrat, 2 * bv_s, 2 * fv_s) / a0


def snow_smoc(c, temp, rs):
    """The Field fit at cse(1) on smob = rs*oams (M:4920-4930 / M:1590-1600)."""
    tc0 = np.minimum(-0.1, temp - 273.15)
    smob = rs * c["oams"]
    x = c["cse"][0]
    return 10.0 ** ro._fit(ro.sa, tc0, x) * smob ** ro._fit(ro.sb, tc0, x), smob


def doppler_moments(c, st, w=None):
    """All nine profiles of a state dict (numpy [..., nz]; missing or None qs / qg = 0) and the locals the tests bound
    with: present_r/s/g, W, V, m2."""
    z = np.zeros_like(np.asarray(st["t"], dtype=np.float64))
    g = lambda k: np.asarray(st[k], dtype=np.float64) if st.get(k) is not None else z   # noqa: E731
    ze_r, ze_s, ze_g, v, ilamg, _ = ro.ze_terms(c, g("qv"), g("qr"), g("nr"), g("qs"), g("qg"), g("t"), g("p"))
    pr, ps, pg = v["L_qr"], v["L_qs"], v["L_qg"]
    rhof = np.sqrt(RHO_NOT / v["rho"])
    with np.errstate(all="ignore"):
        vz_r, v2_r = rain_moments(rhof, 1.0 / v["ilamr"])
        vz_g, v2_g = graupel_moments(rhof, ilamg)
        smoc, smob = snow_smoc(c, v["temp"], v["rs"])
        vz_s, v2_s = snow_moments(rhof, smob / smoc)
    vz_r, v2_r = np.where(pr, vz_r, 0.0), np.where(pr, v2_r, 0.0)
    vz_s, v2_s = np.where(ps, vz_s, 0.0), np.where(ps, v2_s, 0.0)
    vz_g, v2_g = np.where(pg, vz_g, 0.0), np.where(pg, v2_g, 0.0)
    W = np.where(pr, ze_r, 0.0) + np.where(ps, ze_s, 0.0) + np.where(pg, ze_g, 0.0)
    some = pr | ps | pg
    with np.errstate(all="ignore"):
        V = np.where(some, (ze_r * vz_r + ze_s * vz_s + ze_g * vz_g) / W, 0.0)
        m2 = np.where(some, (ze_r * v2_r + ze_s * v2_s + ze_g * v2_g) / W, 0.0)
    wind = z if w is None else np.asarray(w, dtype=np.float64)
    dbz_of = lambda ze: 10.0 * np.log10(ze * 1.e18)   # noqa: E731
    return dict(dbz=dbz_of(ze_r + ze_s + ze_g), dbz_r=dbz_of(ze_r), dbz_s=dbz_of(ze_s), dbz_g=dbz_of(ze_g),
                vz_r=vz_r, vz_s=vz_s, vz_g=vz_g, vd=np.where(some, V - wind, 0.0), sw=np.sqrt(np.maximum(0.0, m2 - V * V)),
                present_r=pr, present_s=ps, present_g=pg, W=W, V=V, m2=m2, w=wind)
