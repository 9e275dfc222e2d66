"""Block O (M:3206-3354) of a state as mp_thompson loads it (M:1387-1493), with the snow moments of block D (M:1545-1628)
and the graupel slope of block E (M:1633-1654), restated in numpy, binary64 (the reference's P64 build), in the
reference's order of operations, for arrays [..., nz]: the checker of kidmp::k_fall_speeds (include/kidmp_fall.h).  The
method of tests/refl_oracle.py.

The scheme's run-time constants (gamma functions of thompson_init, M:452-553) come from the C oracle's Oracle.const();
the compile-time PARAMETERs are stated below with their lines.  The inheritance vtrk(k) = vtrk(k+1) is a plain top-down
loop over the levels.
"""
import numpy as np

# ---- PARAMETERs of module_mp_thompson09n ----
T_0 = 273.15                         # M:34
PI = 3.1415926536                    # M:35 (sic, 10 digits)
R = 287.04                           # M:153 (the gas constant the scheme calls R)
R1 = 1.E-12                          # M:132
R2 = 1.E-6                           # M:133
rho_w, rho_g, rho_i = 1000.0, 500.0, 890.0   # M:38, M:40, M:41
mu_r, mu_i, mu_s = 0.0, 0.0, 0.6357  # M:65, M:67, M:75
Kap0, Kap1, Lam0, Lam1 = 490.6, 17.46, 20.78, 3.29   # M:76-79
gonv_min, gonv_max = 1.E4, 3.E6      # M:85-86
am_r, bm_r = PI * rho_w / 6.0, 3.0   # M:90-91
bm_s = 2.0                           # M:93
am_g = PI * rho_g / 6.0              # M:94
am_i, bm_i = PI * rho_i / 6.0, 3.0   # M:96-97
av_r, fv_r = 4854.0, 195.0           # M:102, M:104
av_s, fv_s = 40.0, 100.0             # M:105, M:107
av_g, bv_g = 442.0, 0.89             # M:108-109
av_i, bv_i = 1847.5, 1.0             # M:110-111
RHO_NOT = 101325.0 / (287.05 * 298.0)   # M:141
D0r = 50.E-6                         # M:174
MAX_SUBSTEPS = 10000                 # U5 of DESIGN.md section 2
# Field et al. (2005) snow-moment fit, M:306-311
sa = np.array([5.065339, -0.062659, -3.032362, 0.029469, -0.000285, 0.31255, 0.000204, 0.003199, 0.0, -0.015952])
sb = np.array([0.476221, -0.015896, 0.165977, 0.007468, -0.000141, 0.060366, 0.000079, 0.000594, 0.0, -0.003577])

CONST_NAMES = ("crg", "cre", "org2", "org3", "obmr", "cig", "cie", "oig1", "oig2", "obmi", "csg", "cse", "oams", "cgg", "cge",
               "oge1", "ogg1", "ogg2", "ogg3", "obmg")
NAMES = ("vt_r", "vt_nr", "vt_i", "vt_ni", "vt_s", "vt_g", "flux_r", "flux_i", "flux_s", "flux_g", "flux_total")
INPUTS = ("t", "p", "qv", "qr", "nr", "qi", "ni", "qs", "qg")
SPECIES = ("r", "i", "s", "g")       # the order of nstep


def constants(oracle):
    """The thompson_init values block O and the load read, from an oracle.oracle.Oracle (1-based Fortran arrays -> 0-based)."""
    c = {k: oracle.const(k) for k in CONST_NAMES}
    return {k: (v if v.size > 1 else float(v[0])) for k, v in c.items()}


def default_boost(temp):
    """vts_boost of a level without riming: 1.0 where T < T_0 (M:2027), 1.5 elsewhere (M:1751)."""
    return np.where(np.asarray(temp) < T_0, 1.0, 1.5)


def _fit(coef, tc0, x):
    # M:1590-1599, the terms summed left to right
    return (coef[0] + coef[1] * tc0 + coef[2] * x + coef[3] * tc0 * x + coef[4] * tc0 * tc0 + coef[5] * x * x
            + coef[6] * tc0 * tc0 * x + coef[7] * tc0 * x * x + coef[8] * tc0 * tc0 * tc0 + coef[9] * x * x * x)


def load(c, st, warm=False):
    """M:1387-1493 for arrays [..., nz] (the inputs are not changed): a dict of the per-level locals."""
    g = lambda k: np.asarray(st[k], dtype=np.float64)   # noqa: E731
    temp, pres = g("t"), g("p")
    qv = np.maximum(1.E-10, g("qv"))
    rho = 0.622 * pres / (R * temp * (qv + 0.622))
    z = np.zeros_like(temp)
    qr1d, nr1d = g("qr"), g("nr")
    qi1d, ni1d, qs1d, qg1d = (z, z, z, z) if warm else (g("qi"), g("ni"), g("qs"), g("qg"))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # ice, M:1420-1445
        L_qi = qi1d > R1
        ri = np.where(L_qi, qi1d * rho, R1)
        ni = np.where(L_qi, np.maximum(R2, ni1d * rho), R2)
        lami = c["cie"][1] / 25.E-6
        ni = np.where(L_qi & (ni <= R2), np.minimum(499.E3, c["cig"][0] * c["oig2"] * ri / am_i * lami ** bm_i), ni)
        lami = (am_i * c["cig"][1] * c["oig1"] * ni / ri) ** c["obmi"]
        ilami = 1. / lami
        xDi = (bm_i + mu_i + 1.) * ilami
        lo = c["cie"][1] / 5.E-6
        hi = c["cie"][1] / 300.E-6
        ni = np.where(L_qi & (xDi < 5.E-6), np.minimum(499.E3, c["cig"][0] * c["oig2"] * ri / am_i * lo ** bm_i),
                      np.where(L_qi & (xDi > 300.E-6), c["cig"][0] * c["oig2"] * ri / am_i * hi ** bm_i, ni))
        # rain, M:1447-1474
        L_qr = qr1d > R1
        rr = np.where(L_qr, qr1d * rho, R1)
        nr = np.where(L_qr, np.maximum(R2, nr1d * rho), R2)

        def nr_of(mvd):
            lamr = (3.0 + mu_r + 0.672) / mvd
            return c["crg"][1] * c["org3"] * rr * lamr ** bm_r / am_r

        nr = np.where(L_qr & (nr <= R2), nr_of(1.0E-3), nr)
        lamr = (am_r * c["crg"][2] * c["org2"] * nr / rr) ** c["obmr"]
        mvd_r = (3.0 + mu_r + 0.672) / lamr
        big, small = L_qr & (mvd_r > 2.5E-3), L_qr & (mvd_r < D0r * 0.75)
        mvd_r = np.where(big, 2.5E-3, np.where(small, D0r * 0.75, mvd_r))
        nr = np.where(big, nr_of(2.5E-3), np.where(small, nr_of(D0r * 0.75), nr))
    L_qs = qs1d > R1
    rs = np.where(L_qs, qs1d * rho, R1)
    L_qg = qg1d > R1
    rg = np.where(L_qg, qg1d * rho, R1)
    return dict(temp=temp, rho=rho, rr=rr, nr=nr, mvd_r=mvd_r, ri=ri, ni=ni, rs=rs, rg=rg, L_qr=L_qr, L_qi=L_qi, L_qs=L_qs, L_qg=L_qg)


def snow_moments(c, temp, rs):
    """Block D, M:1548-1600: smob and smoc (bm_s = 2: smo2 = smob)."""
    tc0 = np.minimum(-0.1, temp - 273.15)
    smob = rs * c["oams"]
    smo2 = smob
    x = c["cse"][0]
    a_ = 10.0 ** _fit(sa, tc0, x)
    b_ = _fit(sb, tc0, x)
    return smob, a_ * smo2 ** b_


def graupel_ilamg(c, v):
    """Block E, M:1633-1654: the running minimum of the intercept from the top down."""
    temp, rg = v["temp"], v["rg"]
    nz = temp.shape[-1]
    k_0 = np.zeros(temp.shape[:-1], dtype=np.int64)                      # kts
    for k in range(nz - 1, -1, -1):
        k_0 = np.where(temp[..., k] >= 270.65, np.maximum(k_0, k), k_0)
    N0_min = np.full(temp.shape[:-1], gonv_max)
    ilamg = np.empty_like(temp)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(nz - 1, -1, -1):
            slw = (k > k_0) & v["L_qr"][..., k] & (v["mvd_r"][..., k] > 100.E-6)
            xslw1 = np.where(slw, 4.01 + np.log10(v["mvd_r"][..., k]), 0.01)
            ygra1 = 4.31 + np.log10(np.maximum(5.E-5, rg[..., k]))
            zans1 = 3.1 + (100. / (300. * xslw1 * ygra1 / (10. / xslw1 + 1. + 0.25 * ygra1) + 30. + 10. * ygra1))
            N0_exp = 10. ** zans1
            N0_exp = np.maximum(gonv_min, np.minimum(N0_exp, gonv_max))
            N0_min = np.minimum(N0_exp, N0_min)
            N0_exp = N0_min
            lam_exp = (N0_exp * am_g * c["cgg"][0] / rg[..., k]) ** c["oge1"]
            lamg = lam_exp * (c["cgg"][2] * c["ogg2"] * c["ogg1"]) ** c["obmg"]
            ilamg[..., k] = 1. / lamg
    return ilamg


def _inherit(own, has):
    """vt(k) = own(k) where the level has the species, else vt(k+1); vt(kte+1) = 0 (M:3209-3216)."""
    out = np.empty_like(own)
    above = np.zeros(own.shape[:-1])
    for k in range(own.shape[-1] - 1, -1, -1):
        above = np.where(has[..., k], own[..., k], above)
        out[..., k] = above
    return out


def source_level(has):
    """The level each level takes its value from: itself, the nearest level above that has the species, or -1."""
    src = np.empty(has.shape, dtype=np.int64)
    above = np.full(has.shape[:-1], -1, dtype=np.int64)
    for k in range(has.shape[-1] - 1, -1, -1):
        above = np.where(has[..., k], k, above)
        src[..., k] = above
    return src


def fall_speeds(c, st, boost=None, dz=None, dt=None, warm=False):
    """Steps 1-7 of the diagnostic.  Returns a dict: NAMES -> [..., nz]; r_r, r_i, r_s, r_g (the loaded contents), has_r ..
    has_g (the `> R1` tests of block O), vts0 (snow before the boost); and, when dz and dt are given, nstep [..., 4] int and
    int_arg [..., 4, nz]: INT's argument dt/(dz/v) + 1. of every level (NaN where the level does not fall)."""
    v = load(c, st, warm)
    temp, rho = v["temp"], v["rho"]
    boost = default_boost(temp) if boost is None else np.asarray(boost, dtype=np.float64)
    rhof = np.sqrt(RHO_NOT / rho)                                        # M:3219
    out = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        # rain, M:3221-3237
        has_r = v["rr"] > R1
        lamr = (am_r * c["crg"][2] * c["org2"] * v["nr"] / v["rr"]) ** c["obmr"]
        vtr = rhof * av_r * c["crg"][5] * c["org3"] * lamr ** c["cre"][2] * ((lamr + fv_r) ** (-c["cre"][5]))
        vtnr = rhof * av_r * c["crg"][6] / c["crg"][11] * lamr ** c["cre"][11] * ((lamr + fv_r) ** (-c["cre"][6]))
        vtrk, vtnrk = _inherit(np.where(has_r, vtr, 0.), has_r), _inherit(np.where(has_r, vtnr, 0.), has_r)
        z = np.zeros_like(temp)
        no = np.zeros(temp.shape, dtype=bool)
        if warm:                                                         # M:3346-3352
            vtik = vtnik = vtsk = vtgk = vts = z
            has_i = has_s = has_g = no
        else:
            # ice, M:3256-3269
            has_i = v["ri"] > R1
            lami = (am_i * c["cig"][1] * c["oig1"] * v["ni"] / v["ri"]) ** c["obmi"]
            ilami = 1. / lami
            vti = rhof * av_i * c["cig"][2] * c["oig2"] * ilami ** bv_i
            vtni = rhof * av_i * c["cig"][5] / c["cig"][6] * ilami ** bv_i
            vtik, vtnik = _inherit(np.where(has_i, vti, 0.), has_i), _inherit(np.where(has_i, vtni, 0.), has_i)
            # snow, M:3288-3308
            has_s = v["rs"] > R1
            smob, smoc = snow_moments(c, temp, v["rs"])
            xDs = smoc / smob
            Mrat = 1. / xDs
            ils1 = 1. / (Mrat * Lam0 + fv_s)
            ils2 = 1. / (Mrat * Lam1 + fv_s)
            t1_vts = Kap0 * c["csg"][3] * ils1 ** c["cse"][3]
            t2_vts = Kap1 * Mrat ** mu_s * c["csg"][9] * ils2 ** c["cse"][9]
            ils1 = 1. / (Mrat * Lam0)
            ils2 = 1. / (Mrat * Lam1)
            t3_vts = Kap0 * c["csg"][0] * ils1 ** c["cse"][0]
            t4_vts = Kap1 * Mrat ** mu_s * c["csg"][6] * ils2 ** c["cse"][6]
            vts = rhof * av_s * (t1_vts + t2_vts) / (t3_vts + t4_vts)
            own = np.where(temp > (T_0 + 0.1), np.maximum(vts * boost, vts * ((vtrk - vts * boost) / (temp - T_0))), vts * boost)
            vtsk = _inherit(np.where(has_s, own, 0.), has_s)
            # graupel, M:3325-3334
            has_g = v["rg"] > R1
            ilamg = graupel_ilamg(c, v)
            vtg = rhof * av_g * c["cgg"][5] * c["ogg3"] * ilamg ** bv_g
            own = np.where(temp > T_0, np.maximum(vtg, vtrk), vtg)
            vtgk = _inherit(np.where(has_g, own, 0.), has_g)
    out.update(vt_r=vtrk, vt_nr=vtnrk, vt_i=vtik, vt_ni=vtnik, vt_s=vtsk, vt_g=vtgk)
    out.update(r_r=v["rr"], r_i=v["ri"], r_s=v["rs"], r_g=v["rg"], has_r=has_r, has_i=has_i, has_s=has_s, has_g=has_g,
               vts0=np.where(has_s, vts, 0.), temp=temp)
    if warm:
        out.update(flux_r=vtrk * v["rr"], flux_i=z, flux_s=z, flux_g=z)
        out["flux_total"] = out["flux_r"]
    else:
        out.update(flux_r=vtrk * v["rr"], flux_i=vtik * v["ri"], flux_s=vtsk * v["rs"], flux_g=vtgk * v["rg"])   # M:3368
        out["flux_total"] = ((out["flux_r"] + out["flux_i"]) + out["flux_s"]) + out["flux_g"]
    if dz is not None and dt is not None:
        dzq = np.broadcast_to(np.asarray(dz, dtype=np.float64), temp.shape)
        speeds = (np.maximum(vtrk, vtnrk), vtik, vtsk, vtgk)             # M:3239
        arg = np.full(temp.shape[:-1] + (4, temp.shape[-1]), np.nan)
        for s, vt in enumerate(speeds):
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                a = dt / (dzq / vt) + 1.                                  # M:3241-3242
            arg[..., s, :] = np.where(vt > 1.E-3, a, np.nan)
        n = np.where(np.isnan(arg), 0., np.minimum(np.floor(np.where(np.isnan(arg), 0., arg)), float(MAX_SUBSTEPS))).max(axis=-1).astype(np.int64)
        out["nstep"] = np.where(n == 0, 1, n)                            # NINT(1./onstep), M:3365
        out["int_arg"] = arg
    return out
