"""Numpy restatement of the microwave radiometer (include/kidmp_radiometer.h) for its tests.

sphere_bh    the series of kid_amd/csrc/kidmp_mie_sphere.h (mie_series, mie_efficiencies) restated operation for operation in
             Python floats, as tests/mie_ref.py restates mie_sphere: (Q_ext, Q_sca, Q_back, g) and g Q_sca.
bins_bh      the three rows of a species in the same way.
sphere_scipy the independent Bessel form of tests/mie_ref.py extended to Q_sca and g.
layer, combine, face   kid_amd/csrc/kidmp_radiometer_layer.h operation for operation, on numpy arrays or scalars.
radiometer   k_radiometer: the load of tests/mie_radar_ref.py, the sums over the bins ascending, the carriers, the layers,
             the two scans in the kernel's own Kogge-Stone and carry order, the closure.  The table is the library's own,
             read back through kidmp_radiometer_table_get.
sequential   the same layers added one by one from the surface up and from the top down: an independent order of the
             same algebra.
"""
import math

import numpy as np

import bright_band_ref as bbr
import doppler_ref as dr
import lidar_ref as lr
import mie_radar_ref as mr
import mie_ref
import refl_oracle as ro
from mie_ref import _div, _mul

NAMES = ("k_abs", "k_bsc", "refl", "trans", "tb_up", "tb_down", "tb_toa", "tb_ground", "tau_abs")
SUMMARY = ("tb_toa", "tb_ground", "tau_abs")
INPUTS = mr.INPUTS
SPECIES = mr.SPECIES
ROWS = ("s_abs", "s_bsc", "mass")
PI = mie_ref.PI
R1 = 1.0e-12


# ---- the sphere ----
def sphere_bh(x, m):
    """(Q_ext, Q_sca, Q_back, g, gQ) as kidmp::mie_efficiencies forms them."""
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
    sum_ext = back_re = back_im = sum_sca = sum_adj = sum_ab = 0.0
    sign = -1.0
    pa = pb = (0.0, 0.0)
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
        sum_sca = sum_sca + w * ((an[0] * an[0] + an[1] * an[1]) + (bn[0] * bn[0] + bn[1] * bn[1]))
        if n > 1:
            e1 = en - 1.0
            sum_adj = sum_adj + ((e1 * (e1 + 2.0)) / (e1 + 1.0)) * ((pa[0] * an[0] + pa[1] * an[1]) + (pb[0] * bn[0] + pb[1] * bn[1]))
        sum_ab = sum_ab + (w / (en * (en + 1.0))) * (an[0] * bn[0] + an[1] * bn[1])
        pa, pb = an, bn
        sign = -sign
        psi0, psi1 = psi1, psi
        chi0, chi1 = chi1, chi
    x2 = x * x
    qext = (2.0 / x2) * sum_ext
    qback = (back_re * back_re + back_im * back_im) / x2
    qsca = (2.0 / x2) * sum_sca
    gq = (4.0 / x2) * (sum_adj + sum_ab)
    g = gq / qsca if qsca > 0.0 else 0.0
    return qext, qsca, qback, g, gq


def bins_bh(cfg, species, D):
    """rows [3, nb] as kidmp::radiometer_bins forms them."""
    lam = float(cfg.wavelength)
    rows = np.empty((3, len(D)))
    for b, d in enumerate(D):
        d = float(d)
        d2 = d * d
        d3 = d2 * d
        mass = (mie_ref.PI_S / 6.0) * cfg.rho_w * d3 if species == "r" else mie_ref.AM_S * d2 if species == "s" else mie_ref.AM_G * d3
        m = mie_ref.index_of(cfg, species, d, mass)
        qext, qsca, _, _, gq = sphere_bh(PI * d / lam, complex(*m))
        area = 0.25 * PI * d2
        qa, qb = (qext - qsca if m[1] > 0.0 else 0.0), 0.5 * (qsca - gq)
        rows[:, b] = ((qa if qa > 0.0 else 0.0) * area, (qb if qb > 0.0 else 0.0) * area, mass)
    return rows


def sphere_scipy(x, m):
    """(Q_ext, Q_sca, Q_back, g) from scipy's Bessel functions: the independent form of mie_ref.mie_scipy."""
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
    qsca = 2.0 / x ** 2 * float(np.sum((2 * k + 1) * (np.abs(an) ** 2 + np.abs(bn) ** 2)))
    kk = k[:-1]
    gq = 4.0 / x ** 2 * float(np.sum(kk * (kk + 2.0) / (kk + 1.0) * (an[:-1] * np.conj(an[1:]) + bn[:-1] * np.conj(bn[1:])).real)
                              + np.sum((2 * k + 1.0) / (k * (k + 1.0)) * (an * np.conj(bn)).real))
    return qext, qsca, float(abs(back) ** 2 / x ** 2), gq / qsca


# ---- the layer, the adding and the closure: kidmp_radiometer_layer.h ----
IDENTITY = (0.0, 0.0, 1.0, 0.0, 0.0)


def layer_x(ta, b):
    ta, b = np.asarray(ta, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(ta > 0.0, np.sqrt(np.where(ta > 0.0, ta * (ta + 2.0 * b), 0.0)), 0.0)


def layer(ta, b, x, mu, e, f):
    """(R, T, a) as rad_layer forms them."""
    ta, b = np.asarray(ta, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        c = b / mu
        Rc, Tc = c / (1.0 + c), 1.0 / (1.0 + c)
        S = (ta + b) + x
        G = b / S
        H = (ta + x) / S
        p = H + G * f
        q = 1.0 + G * e
        R = (G * f * (1.0 + e)) / (p * q)
        T = (H * (1.0 + G) * e) / (p * q)
        a = (H * f) / q
    gen, cons = ta > 0.0, ~(ta > 0.0) & (b > 0.0)
    return np.where(gen, R, np.where(cons, Rc, 0.0)), np.where(gen, T, np.where(cons, Tc, 1.0)), np.where(gen, a, 0.0)


def device_ef(y):
    """e = exp_neg(y) and f = y*layer_mean(y) as the kernel forms them (up to its exp)."""
    return bbr.exp_neg(y), y * lr.g(y)


def host_ef(y):
    """e and f of the host program: libm's exp and expm1."""
    return math.exp(-y), -math.expm1(-y)


def state_of(R, T, a, t):
    em = a * t
    return (R, R, T, em, em)


def combine(A, B):
    """The stack of A below B: rad_combine."""
    with np.errstate(all="ignore"):
        d = 1.0 - A[0] * B[1]
        T = (A[2] * B[2]) / d
        Rb = A[1] + ((A[2] * A[2]) * B[1]) / d
        Rt = B[0] + ((B[2] * B[2]) * A[0]) / d
        Eu = B[3] + (B[2] * (A[3] + A[0] * B[4])) / d
        Ed = A[4] + (A[2] * (B[4] + B[1] * A[3])) / d
    return (Rt, Rb, T, Eu, Ed)


def face(P, S, emissivity, ts, tc):
    """(up, down, 1 - Rt* Rb_S) at the face between the stacks P (below) and S (above): rad_face."""
    rs = 1.0 - emissivity
    with np.errstate(all="ignore"):
        ds = 1.0 - rs * P[1]
        Rt = P[0] + ((P[2] * P[2]) * rs) / ds
        Eu = P[3] + (P[2] * (emissivity * ts + rs * P[4])) / ds
        Dn = S[4] + S[2] * tc
        d = 1.0 - Rt * S[1]
        return (Eu + Rt * Dn) / d, (Dn + S[1] * Eu) / d, d


def _select(c, a, b):
    return tuple(np.where(c, x, y) for x, y in zip(a, b))


def wave_scan(v, down):
    """wave_adding_scan over 64 lanes; v: five arrays [..., 64]."""
    lane = np.arange(64)
    d = 1
    while d < 64:
        o = tuple(np.concatenate([c[..., d:], c[..., 64 - d:]], axis=-1) if down else np.concatenate([c[..., :d], c[..., :64 - d]], axis=-1)
                  for c in v)                                     # lanes without a partner: any finite filler, thrown away
        v = _select(lane + d < 64, combine(v, o), v) if down else _select(lane >= d, combine(o, v), v)
        d <<= 1
    return v


def _groups(a, nj, fill):
    ncol, nz = a.shape
    pad = np.full((ncol, 64 * nj), fill)
    pad[:, :nz] = a
    return pad.reshape(ncol, nj, 64)


def stacks(R, T, E):
    """(below, above): the exclusive stacks of every level, five arrays [ncol, nz] each, in the kernel's order."""
    ncol, nz = R.shape
    nj = (nz + 63) // 64
    g = (_groups(R, nj, 0.0), _groups(R, nj, 0.0), _groups(T, nj, 1.0), _groups(E, nj, 0.0), _groups(E, nj, 0.0))
    ident = tuple(np.full(ncol, v) for v in IDENTITY)
    col = lambda s: tuple(c[:, None] for c in s)   # noqa: E731
    lane = np.arange(64)
    above = [None] * nj
    carry = ident
    for j in range(nj - 1, -1, -1):
        inc = wave_scan(tuple(c[:, j] for c in g), True)
        first = tuple(c[:, 0] for c in inc)
        nxt = tuple(np.concatenate([c[:, 1:], c[:, 63:]], axis=1) for c in inc)
        above[j] = _select(lane < 63, combine(nxt, col(carry)), tuple(np.broadcast_to(c, (ncol, 64)) for c in col(carry)))
        carry = combine(first, carry)
    below = [None] * nj
    carry = ident
    for j in range(nj):
        inc = wave_scan(tuple(c[:, j] for c in g), False)
        last = tuple(c[:, 63] for c in inc)
        prev = tuple(np.concatenate([c[:, :1], c[:, :63]], axis=1) for c in inc)
        below[j] = _select(lane > 0, combine(col(carry), prev), tuple(np.broadcast_to(c, (ncol, 64)) for c in col(carry)))
        carry = combine(carry, last)
    join = lambda parts: tuple(np.concatenate([p[i] for p in parts], axis=1)[:, :nz] for i in range(5))   # noqa: E731
    return join(below), join(above)


def sequential(R, T, E):
    """(below, above) with the layers added one by one: below[k] = ((L0 + L1) + ...) + L(k-1), above[k] = L(k+1) + (... + L(nz-1))."""
    ncol, nz = R.shape
    ident = tuple(np.full(ncol, v) for v in IDENTITY)
    L = lambda k: (R[:, k], R[:, k], T[:, k], E[:, k], E[:, k])   # noqa: E731
    below, above = [None] * nz, [None] * nz
    acc = ident
    for k in range(nz):
        below[k] = acc
        acc = combine(acc, L(k))
    acc = ident
    for k in range(nz - 1, -1, -1):
        above[k] = acc
        acc = combine(L(k), acc)
    join = lambda parts: tuple(np.stack([p[i] for p in parts], axis=1) for i in range(5))   # noqa: E731
    return join(below), join(above)


def brightness(R, T, E, below, above, emissivity, ts, tc):
    """(tb_up, tb_down, d_up, d_down) from the exclusive stacks, d the closure's denominators 1 - Rt* Rb_S."""
    own = (R, R, T, E, E)
    ts = np.asarray(ts, dtype=np.float64)[:, None]
    up, _, d_up = face(combine(below, own), above, emissivity, ts, tc)
    _, down, d_down = face(below, combine(own, above), emissivity, ts, tc)
    return up, down, d_up, d_down


def sums(x, par, has, D, dD, rows):
    """A, S, M [ncol, nz] of species x in the kernel's order."""
    A, S, M = (np.zeros(has.shape) for _ in range(3))
    for b in range(len(D)):
        with np.errstate(all="ignore"):
            n = np.where(has, bbr.density(x, par, D[b], dD[b]), 0.0)
            A += n * rows[0, b]
            S += n * rows[1, b]
            M += n * rows[2, b]
    return A, S, M


def optics(c, cfg, table, st, k_gas=None, warm=False):
    """(k_abs, k_bsc, temp): the coefficients of every level.  c: refl_oracle.constants; cfg: the table's configuration;
    table: species -> (D, dD, rows[3, nb]); st: numpy [ncol, nz], missing or None qc, qs, qg = 0; warm: an iiwarm context."""
    z = np.zeros_like(np.asarray(st["t"], dtype=np.float64))
    g = lambda k: np.asarray(st[k], dtype=np.float64) if st.get(k) is not None else z   # noqa: E731
    qs, qg = (z, z) if warm else (g("qs"), g("qg"))
    _, _, _, v, ilamg, N0_g = ro.ze_terms(c, g("qv"), g("qr"), g("nr"), qs, qg, g("t"), g("p"))
    rho = v["rho"]
    with np.errstate(all="ignore"):
        smoc, smob = dr.snow_smoc(c, v["temp"], v["rs"])
        par = {"r": dict(N0=v["N0_r"], lam=1.0 / v["ilamr"]), "s": dict(smob=smob, smoc=smoc), "g": dict(N0=N0_g, lam=1.0 / ilamg)}
    has = {"r": v["L_qr"], "s": v["L_qs"], "g": v["L_qg"]}
    rq = {"r": g("qr") * rho, "s": v["rs"], "g": v["rg"]}
    kabs, kbsc = np.zeros_like(z), np.zeros_like(z)
    for x in SPECIES:
        D, dD, rows = table[x]
        A, S, M = sums(x, par[x], has[x], D, dD, rows)
        with np.errstate(all="ignore"):
            ok = has[x] & (M > 0.0)
            Ms = np.where(ok, M, 1.0)
            kabs = kabs + np.where(ok, rq[x] * A / Ms, 0.0)
            kbsc = kbsc + np.where(ok, rq[x] * S / Ms, 0.0)
    qc = g("qc")
    kabs = np.where(qc > R1, kabs + mr.cloud_factor(cfg) * ((rho * qc) / cfg.rho_w), kabs)
    if k_gas is not None:
        kabs = kabs + np.broadcast_to(np.asarray(k_gas, dtype=np.float64), z.shape)
    return kabs, kbsc, g("t")


def layers(kabs, kbsc, temp, dz, mu):
    """(ta, b, R, T, E) of every level."""
    dzf = np.broadcast_to(np.asarray(dz, dtype=np.float64), kabs.shape)
    ta, b = kabs * dzf, kbsc * dzf
    x = layer_x(ta, b)
    y = x / mu
    e, f = device_ef(y)
    R, T, a = layer(ta, b, x, mu, e, f)
    return ta, b, R, T, a * temp


def radiometer(c, cfg, table, st, dz=None, k_gas=None, t_sfc=None, mu=1.0, emissivity=1.0, t_cosmic=2.725, warm=False, order=stacks):
    """Every output of NAMES (those that need dz only with dz), and ta, b, d_up, d_down for the tests."""
    kabs, kbsc, temp = optics(c, cfg, table, st, k_gas, warm)
    out = dict(k_abs=kabs, k_bsc=kbsc)
    if dz is None:
        return out
    ta, b, R, T, E = layers(kabs, kbsc, temp, dz, mu)
    out.update(ta=ta, b=b, refl=R, trans=T, tau_abs=mr.wave_total(ta))
    below, above = order(R, T, E)
    ts = temp[:, 0] if t_sfc is None else np.asarray(t_sfc, dtype=np.float64)
    up, down, d_up, d_down = brightness(R, T, E, below, above, emissivity, ts, t_cosmic)
    out.update(tb_up=up, tb_down=down, d_up=d_up, d_down=d_down, tb_toa=up[:, -1].copy(), tb_ground=down[:, 0].copy())
    return out


def ulps(got, want):
    """|got - want| in units of the spacing of `want`."""
    with np.errstate(all="ignore"):
        return np.abs(got - want) / np.spacing(np.abs(want))


cfg_of = mr.cfg_of
