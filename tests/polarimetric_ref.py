"""Numpy restatement of include/kidmp_polarimetric.h for the tests.

The particle (kid_amd/csrc/kidmp_spheroid.h) is restated operation for operation in Python floats (binary64, one rounding
per operation), the complex arithmetic written out as the header writes it: shape, spheroid_P, moments, spheroid_rows,
rain_ratio, bins.  sqrt, atan and exp are math's, which call the host's libm as the C++ does.

The kernel (kidmp::k_polarimetric) is restated in numpy: the load of refl_oracle / doppler_ref as tests/mie_radar_ref.py
takes it, the densities of size_spectra_ref.spectrum, the seven sums over the bins ascending into accumulators that start
at +0.0, the carriers in the kernel's order.  The table -- D, dD, the seven rows, the flag and the scalars of each species
-- is the library's own, read back through kidmp_pol_table_get, so this reference pins the kernel and the first part pins
the table.
"""
import math

import numpy as np

import bright_band_ref as bbr
import doppler_ref as dr
import mie_ref as mr
import refl_oracle as ro

NAMES = ("dbz_h", "zdr", "kdp", "rhohv", "dbz_h_r", "dbz_h_s", "dbz_h_g", "zdr_r", "zdr_s", "zdr_g", "kdp_r", "kdp_s", "kdp_g")
INPUTS = ("t", "p", "qv", "qr", "nr", "qs", "qg")
SPECIES = ("r", "s", "g")
ROWS = ("s_h", "s_v", "c_re", "c_im", "s_0", "k", "mass")
PI = 3.14159265358979323846
BRANDES = (0.9951, 0.02510, -0.03644, 0.005303, -0.0002492)


class PolCfg:
    """What kidmp_pol_cfg holds, with the defaults of kidmp_pol_defaults."""

    def __init__(self, axis_r=BRANDES, axis_r_min=0.2, axis_s=0.75, axis_g=0.8, sigma=None, force_quadrature=False):
        deg = PI / 180.0
        self.axis_r, self.axis_r_min, self.axis_s, self.axis_g = tuple(axis_r), axis_r_min, axis_s, axis_g
        self.sigma = (10.0 * deg, 40.0 * deg, 40.0 * deg) if sigma is None else tuple(sigma)
        self.force_quadrature = force_quadrature


# ---- the particle ----
def shape_closed(f2):
    f = math.sqrt(f2)
    return ((1.0 + f2) / f2) * (1.0 - math.atan(f) / f)


def shape_series(f2):
    s, p, sign = 0.0, 1.0, 1.0
    for n in range(1, 13):
        s = s + (sign * p) / float(2 * n + 1)
        p = p * f2
        sign = -sign
    return (1.0 + f2) * s


def shape(r):
    """(L_a, L_b) as kidmp::spheroid_shape forms them."""
    if r >= 1.0:
        return 1.0 / 3.0, 1.0 / 3.0
    f2 = 1.0 / (r * r) - 1.0
    La = shape_series(f2) if f2 < 1.0 / 64.0 else shape_closed(f2)
    return La, 0.5 * (1.0 - La)


def spheroid_P(eps, L):
    e1 = (eps[0] - 1.0, eps[1])
    return mr._div(e1, (3.0 * (1.0 + L * e1[0]), 3.0 * (L * e1[1])))


def moments(sigma):
    """(A1, A2, A3, A4, A5, A7) as kidmp::pol_moments forms them."""
    q = math.exp(-2.0 * (sigma * sigma))
    q2 = q * q
    q4 = q2 * q2
    plus, minus = (0.375 + 0.5 * q) + 0.125 * q4, (0.375 - 0.5 * q) + 0.125 * q4
    return (0.25 * ((1.0 + q) * (1.0 + q)), 0.25 * (1.0 - q2), plus * plus, minus * plus, 0.125 * (plus * (1.0 - q4)),
            0.5 * (q * (1.0 + q)))


def _copolar(d6, Pb, dl, Aa, Ab):
    pb2 = Pb[0] * Pb[0] + Pb[1] * Pb[1]
    re = Pb[0] * dl[0] + Pb[1] * dl[1]
    dd = dl[0] * dl[0] + dl[1] * dl[1]
    return d6 * ((pb2 - (2.0 * Aa) * re) + Ab * dd)


def spheroid_rows(eps, ratio, A, D):
    """Rows 0..5 as kidmp::pol_spheroid forms them; eps = (re, im), A = moments(sigma)."""
    A1, A2, A3, A4, A5, A7 = A
    La, Lb = shape(ratio)
    Pa, Pb, P0 = spheroid_P(eps, La), spheroid_P(eps, Lb), spheroid_P(eps, 1.0 / 3.0)
    dl = (Pb[0] - Pa[0], Pb[1] - Pa[1])
    d3 = (D * D) * D
    d6 = d3 * d3
    pb2 = Pb[0] * Pb[0] + Pb[1] * Pb[1]
    dd = dl[0] * dl[0] + dl[1] * dl[1]
    re = Pb[0] * dl[0] + Pb[1] * dl[1]
    im1 = Pb[0] * dl[1] - Pb[1] * dl[0]
    im2 = Pb[1] * dl[0] - Pb[0] * dl[1]
    return [_copolar(d6, Pb, dl, A2, A4), _copolar(d6, Pb, dl, A1, A3), d6 * (((pb2 + A5 * dd) - A1 * re) - A2 * re),
            d6 * ((0.0 - A1 * im1) - A2 * im2), _copolar(d6, P0, (0.0, 0.0), A2, A4), (d3 * dl[0]) * A7]


def rain_ratio(pol, D):
    d = D * 1e3
    c = pol.axis_r
    r = c[0] + d * (c[1] + d * (c[2] + d * (c[3] + d * c[4])))
    return pol.axis_r_min if r < pol.axis_r_min else 1.0 if r > 1.0 else r


def permittivity(cfg, species, D, mass):
    """kidmp::mie_permittivity: (re, im)."""
    ew, ei = complex(cfg.eps_w), complex(cfg.eps_i)
    if species == "r":
        return (ew.real, ew.imag)
    sphere = mr.PI_S / 6.0 * D * D * D
    vi = mass / cfg.rho_i
    f = vi / sphere if vi < sphere else 1.0
    k = mr._K((ei.real, ei.imag))
    fk = (f * k[0], f * k[1])
    return mr._div((1.0 + 2.0 * fk[0], 2.0 * fk[1]), (1.0 - fk[0], -fk[1]))


def bins(cfg, pol, species, D):
    """rows [7, nb] as kidmp::pol_bins forms them.  cfg: an object with eps_w, eps_i, rho_w, rho_i."""
    A = moments(pol.sigma[SPECIES.index(species)])
    rows = np.empty((7, len(D)))
    for b, d in enumerate(D):
        d = float(d)
        d2 = d * d
        d3 = d2 * d
        mass = (mr.PI_S / 6.0) * cfg.rho_w * d3 if species == "r" else mr.AM_S * d2 if species == "s" else mr.AM_G * d3
        ratio = rain_ratio(pol, d) if species == "r" else pol.axis_s if species == "s" else pol.axis_g
        rows[:6, b] = spheroid_rows(permittivity(cfg, species, d, mass), ratio, A, d)
        rows[6, b] = mass
    return rows


def scalars(rows):
    """The five scalars of a uniform species: the ratios of the rows of its first bin."""
    return np.array([rows[0, 0] / rows[4, 0], rows[1, 0] / rows[4, 0], rows[2, 0] / rows[4, 0], rows[3, 0] / rows[4, 0],
                     rows[5, 0] / rows[6, 0]])


# ---- the kernel ----
def sums(x, par, has, D, dD, rows):
    """H, V, Cr, Ci, S, K, M [ncol, nz] of species x in the kernel's order."""
    acc = [np.zeros(has.shape) for _ in range(7)]
    for b in range(len(D)):
        with np.errstate(all="ignore"):
            n = np.where(has, bbr.density(x, par, D[b], dD[b]), 0.0)
            for i in range(7):
                acc[i] += n * rows[i, b]
    return acc


def kfac(wavelength):
    return (90.0e3 * PI) / wavelength


def polarimetric(c, wavelength, table, st, warm=False, quadrature=False):
    """Every output of NAMES.  c: refl_oracle.constants; table: species -> (D, dD, rows[7, nb], uniform, scalars[5]) as
    kidmp_pol_table_get returns them; st: numpy [ncol, nz], missing or None qs, qg = 0; warm: an iiwarm context;
    quadrature: walk the bins of a uniform species too (what force_quadrature = 1 makes the kernel do).  Also the locals
    ze_r, ze_s, ze_g (closed-form)."""
    z = np.zeros_like(np.asarray(st["t"], dtype=np.float64))
    g = lambda k: np.asarray(st[k], dtype=np.float64) if st.get(k) is not None else z   # noqa: E731
    qs, qg = (z, z) if warm else (g("qs"), g("qg"))
    ze_r, ze_s, ze_g, v, ilamg, N0_g = ro.ze_terms(c, g("qv"), g("qr"), g("nr"), qs, qg, g("t"), g("p"))
    rho = v["rho"]
    with np.errstate(all="ignore"):
        smoc, smob = dr.snow_smoc(c, v["temp"], v["rs"])
        par = {"r": dict(N0=v["N0_r"], lam=1.0 / v["ilamr"]), "s": dict(smob=smob, smoc=smoc), "g": dict(N0=N0_g, lam=1.0 / ilamg)}
    has = {"r": v["L_qr"], "s": v["L_qs"], "g": v["L_qg"]}
    rq = {"r": np.where(v["L_qr"], g("qr") * rho, 0.0), "s": v["rs"], "g": v["rg"]}
    ze = {"r": ze_r, "s": ze_s, "g": ze_g}
    out = dict(ze_r=ze_r, ze_s=ze_s, ze_g=ze_g)
    Zh, Zv, Cr, Ci, Kd = (np.zeros_like(z) for _ in range(5))
    kf = kfac(wavelength)
    for x in SPECIES:
        D, dD, rows, uniform, scal = table[x]
        one = np.ones_like(z)
        with np.errstate(all="ignore"):
            if uniform and not quadrature:
                rh, rv, rcr, rci, rk = (np.where(has[x], scal[i], e) for i, e in enumerate((1.0, 1.0, 1.0, 0.0, 0.0)))
            else:
                H, V, Xr, Xi, S, K, M = sums(x, par[x], has[x], D, dD, rows)
                oks = has[x] & (S > 0.0)
                Ss = np.where(oks, S, 1.0)
                rh, rv, rcr, rci = (np.where(oks, H / Ss, 1.0), np.where(oks, V / Ss, 1.0), np.where(oks, Xr / Ss, 1.0),
                                    np.where(oks, Xi / Ss, 0.0))
                okm = has[x] & (M > 0.0)
                rk = np.where(okm, K / np.where(okm, M, 1.0), 0.0)
            zh, zv = ze[x] * rh, ze[x] * rv
            kd = np.where(has[x], (kf * rq[x]) * rk, 0.0)
            Zh, Zv, Cr, Ci, Kd = Zh + zh, Zv + zv, Cr + ze[x] * rcr, Ci + ze[x] * rci, Kd + kd
            out["dbz_h_" + x] = 10.0 * np.log10(zh * 1.e18)
            out["zdr_" + x] = 10.0 * np.log10(zh / zv)
            out["kdp_" + x] = kd
            out["ratio_h_" + x], out["ratio_v_" + x] = rh * one, rv * one
    out["dbz_h"] = 10.0 * np.log10(Zh * 1.e18)
    out["zdr"] = 10.0 * np.log10(Zh / Zv)
    out["kdp"] = Kd
    out["rhohv"] = np.minimum(1.0, np.sqrt(Cr * Cr + Ci * Ci) / np.sqrt(Zh * Zv))
    return out


def cfg_of(wavelength=0.10, eps_w=complex(79.5, 24.9), eps_i=None, rho_w=1000.0, rho_i=900.0, kw2=0.93):
    """An object with the members of kidmp_mie_cfg; the defaults are kidmp_mie_defaults'."""
    class Cfg:
        pass
    c = Cfg()
    c.wavelength, c.eps_w, c.rho_w, c.rho_i, c.kw2 = wavelength, complex(eps_w), rho_w, rho_i, kw2
    c.eps_i = complex(bbr.default_eps_i(), 0.0) if eps_i is None else complex(eps_i)
    return c


def ulps(got, want):
    """|got - want| in units of the spacing of `want`."""
    with np.errstate(all="ignore"):
        return np.abs(got - want) / np.spacing(np.abs(want))
