"""calc_refl10cm (M:4946-5244) restated in numpy, binary64 (the reference's P64 build): the checker of the reflectivity
kernel (kid_amd/csrc/thompson_reflectivity.hip).  Only the lines that can change dBZ as the reference ships them are
restated, in the reference's order; the melting-level search (M:5107-5121) and the wet-snow / wet-graupel block
(M:5140-5192) are dead with nrbins = 0 (M:204), and rc, rhof, smoc never reach dBZ.

The scheme's run-time constants (gamma functions of thompson_init, M:452-553) come from the C oracle's Oracle.const();
the compile-time PARAMETERs are stated below with their lines.
"""
import numpy as np

# ---- PARAMETERs of module_mp_thompson09n ----
PI = 3.1415926536                    # M:35 (sic, 10 digits)
R = 287.04                           # M:153 (the gas constant the scheme calls R)
R1 = 1.E-12                          # M:132
R2 = 1.E-6                           # M:133
rho_w, rho_g = 1000.0, 500.0         # M:38, M:40
am_r = PI * rho_w / 6.0              # M:90
am_s = 0.069                         # M:92
am_g = PI * rho_g / 6.0              # M:94
mu_r = 0.0                           # M:65
gonv_min, gonv_max = 1.E4, 3.E6      # M:85-86
# Field et al. (2005) snow-moment fit, M:306-311
sa = np.array([5.065339, -0.062659, -3.032362, 0.029469, -0.000285, 0.31255, 0.000204, 0.003199, 0.0, -0.015952])
sb = np.array([0.476221, -0.015896, 0.165977, 0.007468, -0.000141, 0.060366, 0.000079, 0.000594, 0.0, -0.003577])

CONST_NAMES = ("cre", "crg", "cgg", "cge", "cse", "org2", "obmr", "oge1", "ogg1", "ogg2", "obmg", "oams")

# a level with neither rain nor snow nor graupel: 10*log10(3 * 1e-22 * 1e18)
EMPTY_DBZ = 10.0 * np.log10(3e-22 * 1e18)


def constants(oracle):
    """The thompson_init values calc_refl10cm reads, from an oracle.oracle.Oracle (1-based Fortran arrays -> 0-based)."""
    c = {k: oracle.const(k) for k in CONST_NAMES}
    return {k: (v if v.size > 1 else float(v[0])) for k, v in c.items()}


def _fit(coef, tc0, x):
    # M:5066-5070 / M:5073-5077, the terms summed left to right
    return (coef[0] + coef[1] * tc0 + coef[2] * x + coef[3] * tc0 * x + coef[4] * tc0 * tc0 + coef[5] * x * x
            + coef[6] * tc0 * tc0 * x + coef[7] * tc0 * x * x + coef[8] * tc0 * tc0 * tc0 + coef[9] * x * x * x)


def load(c, qv1d, qr1d, nr1d, qs1d, qg1d, t1d, p1d):
    """M:4991-5028 for arrays [..., nz]: returns a dict of the per-level locals."""
    temp = np.asarray(t1d, dtype=np.float64)
    qv = np.maximum(1.E-10, np.asarray(qv1d, dtype=np.float64))
    pres = np.asarray(p1d, dtype=np.float64)
    rho = 0.622 * pres / (R * temp * (qv + 0.622))
    qr1d = np.asarray(qr1d, dtype=np.float64)
    nr1d = np.asarray(nr1d, dtype=np.float64)
    qs1d = np.asarray(qs1d, dtype=np.float64)
    qg1d = np.asarray(qg1d, dtype=np.float64)
    L_qr = qr1d > R1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rr = np.where(L_qr, qr1d * rho, R1)
        nr = np.where(L_qr, np.maximum(R2, nr1d * rho), R1)          # R1, not R2, for the number of a rain-free level
        lamr = (am_r * c["crg"][2] * c["org2"] * nr / rr) ** c["obmr"]
        ilamr = 1.0 / lamr
        N0_r = nr * c["org2"] * lamr ** c["cre"][1]
        mvd_r = np.where(L_qr, (3.0 + mu_r + 0.672) * ilamr, 50.E-6)
    L_qs = qs1d > R2                                                  # R2, not R1
    rs = np.where(L_qs, qs1d * rho, R1)
    L_qg = qg1d > R2
    rg = np.where(L_qg, qg1d * rho, R1)
    return dict(temp=temp, rho=rho, rr=rr, nr=nr, ilamr=ilamr, N0_r=N0_r, mvd_r=mvd_r, rs=rs, rg=rg,
                L_qr=L_qr, L_qs=L_qs, L_qg=L_qg)


def snow_smoz(c, temp, rs):
    """M:5031-5081: bm_s = 2, so smo2 = smob = rs*oams; smoz = a_ * smo2**b_ of the fit at cse(3)."""
    tc0 = np.minimum(-0.1, temp - 273.15)
    smob = rs * c["oams"]
    smo2 = smob
    x = c["cse"][2]
    a_ = 10.0 ** _fit(sa, tc0, x)
    b_ = _fit(sb, tc0, x)
    return a_ * smo2 ** b_


def graupel(c, temp, L_qr, mvd_r, rg):
    """M:5086-5103: the top-down running minimum of the intercept over ALL levels (the last axis, kts first)."""
    nz = temp.shape[-1]
    N0_min = np.full(temp.shape[:-1], gonv_max)
    ilamg = np.empty_like(temp)
    N0_g = np.empty_like(temp)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(nz - 1, -1, -1):
            slw = (temp[..., k] < 270.65) & L_qr[..., k] & (mvd_r[..., k] > 100.E-6)
            xslw1 = np.where(slw, 4.01 + np.log10(mvd_r[..., k]), 0.01)
            ygra1 = 4.31 + np.log10(np.maximum(5.E-5, rg[..., k]))
            zans1 = 3.1 + (100. / (300. * xslw1 * ygra1 / (10. / xslw1 + 1. + 0.25 * ygra1) + 30. + 10. * ygra1))
            N0_exp = 10. ** zans1
            N0_exp = np.maximum(gonv_min, np.minimum(N0_exp, gonv_max))
            N0_min = np.minimum(N0_exp, N0_min)
            N0_exp = N0_min
            lam_exp = (N0_exp * am_g * c["cgg"][0] / rg[..., k]) ** c["oge1"]
            lamg = lam_exp * (c["cgg"][2] * c["ogg2"] * c["ogg1"]) ** c["obmg"]
            ilamg[..., k] = 1. / lamg
            N0_g[..., k] = N0_exp / (c["cgg"][1] * lam_exp) * lamg ** c["cge"][1]
    return ilamg, N0_g


def ze_terms(c, qv1d, qr1d, nr1d, qs1d, qg1d, t1d, p1d):
    """ze_rain, ze_snow, ze_graupel of M:5127-5136."""
    v = load(c, qv1d, qr1d, nr1d, qs1d, qg1d, t1d, p1d)
    smoz = snow_smoz(c, v["temp"], v["rs"])
    ilamg, N0_g = graupel(c, v["temp"], v["L_qr"], v["mvd_r"], v["rg"])
    with np.errstate(invalid="ignore", over="ignore"):
        ze_rain = np.where(v["L_qr"], v["N0_r"] * c["crg"][3] * v["ilamr"] ** c["cre"][3], 1.e-22)
        ze_snow = np.where(v["L_qs"], (0.176 / 0.93) * (6.0 / PI) * (6.0 / PI) * (am_s / 900.0) * (am_s / 900.0) * smoz,
                           1.e-22)
        ze_graupel = np.where(v["L_qg"], (0.176 / 0.93) * (6.0 / PI) * (6.0 / PI) * (am_g / 900.0) * (am_g / 900.0)
                              * N0_g * c["cgg"][3] * ilamg ** c["cge"][3], 1.e-22)
    return ze_rain, ze_snow, ze_graupel, v, ilamg, N0_g


def calc_refl10cm(c, qv1d, qr1d, nr1d, qs1d, qg1d, t1d, p1d):
    """dBZ [..., nz] (M:5196).  qc1d is not an argument: the reference never lets it reach dBZ."""
    ze_rain, ze_snow, ze_graupel, _, _, _ = ze_terms(c, qv1d, qr1d, nr1d, qs1d, qg1d, t1d, p1d)
    return 10. * np.log10((ze_rain + ze_snow + ze_graupel) * 1.e18)


def of_state(c, st):
    """calc_refl10cm of a state dict (numpy [ncol, nz]; missing qs/qg = 0, as an iiwarm run keeps them)."""
    z = np.zeros_like(np.asarray(st["t"], dtype=np.float64))
    g = lambda k: np.asarray(st[k], dtype=np.float64) if st.get(k) is not None else z   # noqa: E731
    return calc_refl10cm(c, g("qv"), g("qr"), g("nr"), g("qs"), g("qg"), g("t"), g("p"))
