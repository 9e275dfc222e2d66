"""References for the Lorenz-Mie sphere of include/kidmp_mie.h (kid_amd/csrc/kidmp_mie_sphere.h).

mie_bh      the header's series restated operation for operation, in Python floats (binary64, one rounding per operation)
            with the complex arithmetic written out as the header writes it.  sin, cos, sqrt, pow and exp are math's, which
            call the host's libm as the C++ does, so the two agree bit for bit.
bins_bh     the five rows of a species in the same way.
mie_scipy   an independent form: a_n and b_n from scipy's Bessel functions of half-integer order and complex argument,
            psi_n(z) = sqrt(pi z/2) J_{n+1/2}(z), chi_n(z) = -sqrt(pi z/2) Y_{n+1/2}(z), and their derivatives from
            psi_n' = psi_{n-1} - n psi_n/z.  No recurrence of the header's is used.
"""
import math

import numpy as np

PI_S = 3.1415926536                                             # the scheme's PI (M:35)
PI = 3.14159265358979323846
AM_S, AM_G = 0.069, PI_S * 500.0 / 6.0
AV_R, BV_R, FV_R = 4854.0, 1.0, 195.0
AV_S, BV_S, FV_S = 40.0, 0.55, 100.0
AV_G, BV_G = 442.0, 0.89
ROWS = ("s_mie", "s_ray", "s_ext", "mass", "v0")
SPECIES = ("r", "s", "g")


def _div(a, b):
    r = 1.0 / (b[0] * b[0] + b[1] * b[1])
    return ((a[0] * b[0] + a[1] * b[1]) * r, (a[1] * b[0] - a[0] * b[1]) * r)


def _mul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def _K(e):
    return _div((e[0] - 1.0, e[1]), (e[0] + 2.0, e[1]))


def csqrt(e):
    mod = math.sqrt(e[0] * e[0] + e[1] * e[1])
    if e[0] >= 0.0:
        re = math.sqrt(0.5 * (mod + e[0]))
        return (re, e[1] / (2.0 * re) if re > 0.0 else 0.0)
    im = math.sqrt(0.5 * (mod - e[0]))
    return (e[1] / (2.0 * im), im)


def mie_bh(x, m):
    """(Q_ext, Q_back) as kidmp::mie_sphere forms them."""
    m = complex(m)
    m = (m.real, m.imag)
    y = (m[0] * x, m[1] * x)
    ymod = math.sqrt(y[0] * y[0] + y[1] * y[1])
    xstop = x + 4.0 * math.pow(x, 1.0 / 3.0) + 2.0
    nstop = int(xstop)
    nmx = int(float(nstop) if float(nstop) > ymod else ymod) + 15
    d = [(0.0, 0.0)] * (nmx + 1)
    for n in range(nmx, 0, -1):
        ny = _div((float(n), 0.0), y)
        r = _div((1.0, 0.0), (d[n][0] + ny[0], d[n][1] + ny[1]))
        d[n - 1] = (ny[0] - r[0], ny[1] - r[1])
    psi0, psi1 = math.cos(x), math.sin(x)
    chi0, chi1 = -math.sin(x), math.cos(x)
    sum_ext = back_re = back_im = 0.0
    sign = -1.0
    for n in range(1, nstop + 1):
        en = float(n)
        f, nx = (2.0 * en - 1.0) / x, en / x
        psi = f * psi1 - psi0
        chi = f * chi1 - chi0
        dm, md = _div(d[n], m), _mul(m, d[n])
        ta, tb = (dm[0] + nx, dm[1]), (md[0] + nx, md[1])
        xi, xi1 = (psi, -chi), (psi1, -chi1)
        txa, txb = _mul(ta, xi), _mul(tb, xi)
        an = _div((ta[0] * psi - psi1, ta[1] * psi), (txa[0] - xi1[0], txa[1] - xi1[1]))
        bn = _div((tb[0] * psi - psi1, tb[1] * psi), (txb[0] - xi1[0], txb[1] - xi1[1]))
        w = 2.0 * en + 1.0
        sum_ext = sum_ext + w * (an[0] + bn[0])
        back_re = back_re + (w * sign) * (an[0] - bn[0])
        back_im = back_im + (w * sign) * (an[1] - bn[1])
        sign = -sign
        psi0, psi1 = psi1, psi
        chi0, chi1 = chi1, chi
    x2 = x * x
    return (2.0 / x2) * sum_ext, (back_re * back_re + back_im * back_im) / x2


def index_of(cfg, species, D, mass):
    """The refractive index (re, im) of the species' particle: kidmp::mie_index.  cfg: an object with wavelength, eps_w,
    eps_i (complex), rho_w, rho_i, kw2."""
    ew, ei = complex(cfg.eps_w), complex(cfg.eps_i)
    if species == "r":
        return csqrt((ew.real, ew.imag))
    sphere = PI_S / 6.0 * D * D * D
    vi = mass / cfg.rho_i
    f = vi / sphere if vi < sphere else 1.0
    k = _K((ei.real, ei.imag))
    fk = (f * k[0], f * k[1])
    return csqrt(_div((1.0 + 2.0 * fk[0], 2.0 * fk[1]), (1.0 - fk[0], -fk[1])))


def bins_bh(cfg, species, D):
    """rows [5, nb] as kidmp::mie_bins forms them."""
    ze_ice = (0.176 / 0.93) * (6.0 / PI_S) * (6.0 / PI_S)
    ze_snow, ze_graupel = ze_ice * (AM_S / 900.0) * (AM_S / 900.0), ze_ice * (AM_G / 900.0) * (AM_G / 900.0)
    lam = float(cfg.wavelength)
    lam2 = lam * lam
    pi2 = PI * PI
    pi5 = pi2 * pi2 * PI
    scale = (lam2 * lam2) / (pi5 * cfg.kw2)
    rows = np.empty((5, len(D)))
    for b, d in enumerate(D):
        d = float(d)
        d2 = d * d
        d3 = d2 * d
        if species == "r":
            mass, ray, v0 = (PI_S / 6.0) * cfg.rho_w * d3, d3 * d3, AV_R * math.pow(d, BV_R) * math.exp(-FV_R * d)
        elif species == "s":
            mass, ray, v0 = AM_S * d2, ze_snow * (d2 * d2), AV_S * math.pow(d, BV_S) * math.exp(-FV_S * d)
        else:
            mass, ray, v0 = AM_G * d3, ze_graupel * (d3 * d3), AV_G * math.pow(d, BV_G)
        m = index_of(cfg, species, d, mass)
        qext, qback = mie_bh(PI * d / lam, complex(*m))
        area = 0.25 * PI * d2
        rows[:, b] = (scale * (qback * area), ray, qext * area, mass, v0)
    return rows


def mie_scipy(x, m):
    """(Q_ext, Q_back) from scipy's Bessel functions: the independent form."""
    from scipy.special import jv, yv
    m = complex(m)
    nstop = int(x + 4.0 * x ** (1.0 / 3.0) + 2.0)
    n = np.arange(0, nstop + 1)
    y = m * x

    def psi(z):
        return np.sqrt(0.5 * np.pi * z) * jv(n + 0.5, z)

    def chi(z):
        return -np.sqrt(0.5 * np.pi * z) * yv(n + 0.5, z)

    px, cx, py = psi(x), chi(x), psi(y)
    xi = px - 1j * cx
    k = n[1:]
    dpx = px[:-1] - k * px[1:] / x
    dxi = xi[:-1] - k * xi[1:] / x
    dpy = py[:-1] - k * py[1:] / y
    px, xi, py = px[1:], xi[1:], py[1:]
    an = (m * py * dpx - px * dpy) / (m * py * dxi - xi * dpy)
    bn = (py * dpx - m * px * dpy) / (py * dxi - m * xi * dpy)
    qext = 2.0 / x ** 2 * float(np.sum((2 * k + 1) * (an + bn).real))
    back = np.sum((2 * k + 1) * (-1.0) ** k * (an - bn))
    return qext, float(abs(back) ** 2 / x ** 2)


def absK2(eps):
    e = complex(eps)
    return abs((e - 1.0) / (e + 2.0)) ** 2
