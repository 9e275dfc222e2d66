"""The size spectra (include/kidmp_spectra.h) restated in numpy, binary64, from the reference's lines: the load of
mp_thompson (M:1387-1493; tests/fall_speeds_ref.py restates rain, ice, snow and graupel and is used for them), cloud water
(M:1395-1410, M:1690-1692), block E's graupel intercept (M:1633-1654), the bin grids of thompson_init (M:605-657) and the
bin formulas of the table builders (M:3768, M:3967-3975, M:4157-4164, M:4206-4221).  The checker of kidmp::k_size_spectra.

Every gamma constant of thompson_init (M:452-553) is formed here with math.gamma: nothing comes from the library or from
the C oracle.  An exponential whose argument exceeds 700 contributes exact +0.0 (the rule of the header).
"""
import math

import numpy as np

import fall_speeds_ref as fr
from fall_speeds_ref import (PI, R1, R2, Kap0, Kap1, Lam0, Lam1, am_g, am_i, am_r, bm_i, bm_r, bm_s, bv_g, bv_i, gonv_max, gonv_min,  # noqa: F401
                             mu_i, mu_r, mu_s)

SPECIES = ("c", "i", "r", "s", "g")
PARAMS = ("lam_c", "n0_c", "nu_c", "lam_i", "n0_i", "lam_r", "n0_r", "smob", "smoc", "lam_g", "n0_g")
PARAMS_OF = {"c": ("lam_c", "n0_c", "nu_c"), "i": ("lam_i", "n0_i"), "r": ("lam_r", "n0_r"), "s": ("smob", "smoc"), "g": ("lam_g", "n0_g")}
INPUTS = ("t", "p", "qv", "qc", "nc", "qi", "ni", "qr", "nr", "qs", "qg")
EXP_MAX = 700.0
MAX_BINS, DEFAULT_BINS = 256, 100
mu_g, bm_g = 0.0, 3.0                # M:66, M:95
bv_r, bv_s = 1.0, 0.55               # M:103, M:106
am_s = 0.069                         # M:92
Nt_c_max = 1999.E6                   # M:60
xm0i = 1.E-12                        # M:172
D0c, D0r, D0s, D0g = 1.E-6, 50.E-6, 200.E-6, 250.E-6   # M:173-176
nbins = 100                          # M:180


def constants(set_Nc=100.0):
    """thompson_init, M:442-553, with math.gamma for WGAMMA; 0-based arrays hold the Fortran element n at n-1.  Holds what
    fall_speeds_ref.load, snow_moments and the functions below read.  set_Nc: cm**-3 (Nt_c = set_Nc*1.e6, M:381)."""
    g = math.gamma
    n = np.arange(1, 16, dtype=np.float64)
    cce = np.array([n + 1., bm_r + n + 1.])                                       # M:453-454
    ccg = np.array([[g(x) for x in row] for row in cce])
    cie = np.array([mu_i + 1., bm_i + mu_i + 1., bm_i + mu_i + bv_i + 1., mu_i + bv_i + 1., mu_i + 2., bm_i * 0.5 + mu_i + bv_i + 1.,
                    bm_i * 0.5 + mu_i + 1.])                                      # M:467-473
    cre = np.array([bm_r + 1., mu_r + 1., bm_r + mu_r + 1., bm_r * 2. + mu_r + 1., mu_r + bv_r + 1., bm_r + mu_r + bv_r + 1.,
                    bm_r * 0.5 + mu_r + bv_r + 1., bm_r + mu_r + bv_r + 3., mu_r + bv_r + 3., mu_r + 2., 0.5 * (bv_r + 5. + 2. * mu_r),
                    bm_r * 0.5 + mu_r + 1., bm_r * 2. + mu_r + bv_r + 1.])        # M:485-497
    cse = np.array([bm_s + 1., bm_s + 2., bm_s * 2.])                             # M:507-509 (the first three)
    cge = np.array([bm_g + 1., mu_g + 1., bm_g + mu_g + 1.])                      # M:532-534 (the first three)
    cig, crg, cgg = (np.array([g(x) for x in e]) for e in (cie, cre, cge))
    return dict(Nt_c=set_Nc * 1.e6, cce=cce, ccg=ccg, ocg1=1. / ccg[0], ocg2=1. / ccg[1],
                cie=cie, cig=cig, oig1=1. / cig[0], oig2=1. / cig[1], obmi=1. / bm_i,
                cre=cre, crg=crg, org1=1. / crg[0], org2=1. / crg[1], org3=1. / crg[2], obmr=1. / bm_r,
                cse=cse, oams=1. / am_s,
                cge=cge, cgg=cgg, oge1=1. / cge[0], ogg1=1. / cgg[0], ogg2=1. / cgg[1], obmg=1. / bm_g)


def default_grids():
    """M:605-657: species -> (D, dD), 100 bins each."""
    out = {}
    Dc, dtc = np.empty(nbins), np.empty(nbins)
    Dc[0] = dtc[0] = D0c * 1.0
    for n in range(1, nbins):                                                     # M:607-610
        Dc[n] = Dc[n - 1] + 1.0E-6
        dtc[n] = Dc[n] - Dc[n - 1]
    out["c"] = (Dc, dtc)
    D0i = (xm0i / am_i) ** (1. / bm_i)                                            # M:445
    for x, lo, hi in (("i", D0i, 5.0 * D0s), ("r", D0r, 0.005), ("s", D0s, 0.02), ("g", D0g, 0.05)):
        xDx = np.empty(nbins + 1)
        xDx[0], xDx[nbins] = lo, hi
        n = np.arange(1, nbins, dtype=np.float64)
        xDx[1:nbins] = np.exp(n / float(nbins) * np.log(xDx[nbins] / xDx[0]) + np.log(xDx[0]))
        out[x] = (np.sqrt(xDx[:-1] * xDx[1:]), xDx[1:] - xDx[:-1])
    return out


def _nu_c(nc):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.minimum(15, np.rint(1000.E6 / nc) + 2).astype(np.int64)         # M:1400, M:1690


def cloud(c, rho, qc1d, nc1d, aero=False, Nt_c=None):
    """M:1395-1410 and M:1690-1692: has, nc, nu_c (int), lamc, N0_c (M:4158).  Nt_c: scalar or [..., 1] per column."""
    has = qc1d > R1
    rc = np.where(has, qc1d * rho, 1.0)
    Nt_c = c["Nt_c"] if Nt_c is None else Nt_c
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if aero:
            nc = np.maximum(2., nc1d * rho)                                       # M:1398
            nu = _nu_c(nc)
            lamc = (nc * am_r * c["ccg"][1][nu - 1] * c["ocg1"][nu - 1] / rc) ** c["obmr"]
            xDc = (bm_r + nu + 1.) / lamc
            lamc = np.where(xDc < D0c, c["cce"][1][nu - 1] / D0c, np.where(xDc > D0r * 2., c["cce"][1][nu - 1] / (D0r * 2.), lamc))
            nc = np.minimum(Nt_c_max, c["ccg"][0][nu - 1] * c["ocg2"][nu - 1] * rc / am_r * lamc ** bm_r)
        else:
            nc = np.broadcast_to(np.asarray(Nt_c, dtype=np.float64), rho.shape)   # M:1410
        has = has & (nc > R2)
        nc = np.where(has, nc, 1.0e8)
        nu = _nu_c(nc)
        lamc = (nc * am_r * c["ccg"][1][nu - 1] * c["ocg1"][nu - 1] / rc) ** c["obmr"]          # M:1692
        n0 = nc * c["ocg1"][nu - 1] * lamc ** c["cce"][0][nu - 1]                 # M:4158
    return has, nc, nu, lamc, n0


def graupel(c, v):
    """Block E, M:1633-1654: lamg and N0_g of every level, with the running minimum of the intercept from the top down."""
    temp, rg = v["temp"], v["rg"]
    nz = temp.shape[-1]
    k_0 = np.zeros(temp.shape[:-1], dtype=np.int64)
    for k in range(nz - 1, -1, -1):
        k_0 = np.where(temp[..., k] >= 270.65, np.maximum(k_0, k), k_0)
    N0_min = np.full(temp.shape[:-1], gonv_max)
    lamg, N0_g = np.empty_like(temp), np.empty_like(temp)
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
            lamg[..., k] = lam_exp * (c["cgg"][2] * c["ogg2"] * c["ogg1"]) ** c["obmg"]
            N0_g[..., k] = N0_exp / (c["cgg"][1] * lam_exp) * lamg[..., k] ** c["cge"][1]
    return lamg, N0_g


def parameters(c, st, warm=False, aero=False, Nt_c=None):
    """The eleven profiles of PARAMS ([..., nz], +0.0 where the species is absent), `has_x` per species and nu (int)."""
    v = fr.load(c, st, warm)
    rho = v["rho"]
    z = np.zeros_like(rho)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        has_c, nc, nu, lamc, n0c = cloud(c, rho, np.asarray(st["qc"], dtype=np.float64),
                                         np.asarray(st["nc"], dtype=np.float64) if aero else z, aero, Nt_c)
        lamr = (am_r * c["crg"][2] * c["org2"] * v["nr"] / v["rr"]) ** c["obmr"]
        n0r = v["nr"] * c["org2"] * lamr ** c["cre"][1]                           # M:1664
        lami = (am_i * c["cig"][1] * c["oig1"] * v["ni"] / v["ri"]) ** c["obmi"]
        n0i = v["ni"] * c["oig1"] * lami ** c["cie"][0]                           # M:4206
        smob, smoc = fr.snow_moments(c, v["temp"], v["rs"])
        lamg, n0g = graupel(c, v)
    has = dict(c=has_c, i=v["L_qi"], r=v["L_qr"], s=v["L_qs"], g=v["L_qg"])
    vals = dict(lam_c=lamc, n0_c=n0c, nu_c=nu.astype(np.float64), lam_i=lami, n0_i=n0i, lam_r=lamr, n0_r=n0r, smob=smob, smoc=smoc,
                lam_g=lamg, n0_g=n0g)
    for x in SPECIES:
        for n in PARAMS_OF[x]:
            out[n] = np.where(has[x], vals[n], 0.0)
        out["has_" + x] = has[x]
    out["nu"] = np.where(has_c, nu, 0)
    return out


def _exp_neg(x):
    """EXP(-x), exact +0.0 where x exceeds EXP_MAX (or is a NaN)."""
    with np.errstate(invalid="ignore", under="ignore"):
        return np.where(x <= EXP_MAX, np.exp(-np.where(x <= EXP_MAX, x, 0.0)), 0.0)


def spectrum(par, x, D, dD):
    """N_x [..., nb, nz] of species x on the grid (D, dD) from the profiles of `parameters`; `arg` [..., nb, nz] is the
    largest exponential argument of the bin (0 where absent) and `nu` the power of D, for the bound of the GPU test."""
    D = np.asarray(D, dtype=np.float64)[:, None]
    dD = np.asarray(dD, dtype=np.float64)[:, None]
    has = par["has_" + x][..., None, :]
    e = lambda k: par[k][..., None, :]   # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        if x in ("r", "g", "i"):
            lam, n0 = e("lam_" + x), e("n0_" + x)
            arg = lam * D
            N = n0 * D ** 0.0 * _exp_neg(arg) * dD                                # mu_r = mu_g = mu_i = 0
            power = 0.0
        elif x == "c":
            lam, n0, nu = e("lam_c"), e("n0_c"), par["nu"][..., None, :]
            arg = lam * D
            N = n0 * D ** nu * _exp_neg(arg) * dD                                 # M:4164
            power = nu.astype(np.float64)
        else:
            smob, smoc = e("smob"), np.where(has, e("smoc"), 1.0)
            r = smob / smoc                                                       # M2*oM3, M:3967-3971
            Mrat = smob * r ** 3
            M0 = np.where(has, r, 1.0) ** mu_s
            slam1, slam2 = r * Lam0, r * Lam1
            arg = slam1 * D
            N = Mrat * (Kap0 * _exp_neg(slam1 * D) + Kap1 * M0 * D ** mu_s * _exp_neg(slam2 * D)) * dD
            power = 3.0 + mu_s
    shape = np.broadcast_shapes(has.shape, D.shape)
    return dict(N=np.where(has, N, 0.0), arg=np.where(has, arg, 0.0) + np.zeros(shape), nu=np.where(has, power, 0.0) + np.zeros(shape))


def size_spectra(c, st, want=SPECIES, grids=None, warm=False, aero=False, Nt_c=None):
    """parameters() plus, for every species in `want`, N_x under its letter and the bound's terms under x + '_arg', x + '_nu'."""
    par = parameters(c, st, warm, aero, Nt_c)
    own = default_grids()
    out = dict(par)
    for x in SPECIES:
        if x in want:
            D, dD = (grids or {}).get(x) or own[x]
            s = spectrum(par, x, D, dD)
            out[x], out[x + "_arg"], out[x + "_nu"] = s["N"], s["arg"], s["nu"]
    return out
