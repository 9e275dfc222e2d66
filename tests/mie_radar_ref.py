"""Numpy restatement of k_mie_radar (include/kidmp_mie.h) for the GPU tests: the load of refl_oracle / doppler_ref, the
densities of size_spectra_ref.spectrum, the sums over the bins ascending into accumulators that start at +0.0, the
carriers and the scans in the kernel's order.  The table -- D, dD and the five rows of each species -- is the library's
own, read back through kidmp_mie_table_get, so the reference pins the kernel and tests/mie_ref.py pins the table.
"""
import math

import numpy as np

import bright_band_ref as bbr
import doppler_ref as dr
import refl_oracle as ro

NAMES = ("dbz", "dbz_up", "dbz_down", "dbz_r", "dbz_s", "dbz_g", "mie_r", "mie_s", "mie_g", "ext", "pia_up", "pia_down", "vd",
         "pia_total")
INPUTS = ("t", "p", "qv", "qc", "qr", "nr", "qs", "qg")
SPECIES = ("r", "s", "g")
PIA = 20.0 / 2.302585092994045684
R1 = 1.0e-12
PI = 3.14159265358979323846


def cloud_factor(cfg):
    """kc = (6 pi/lambda) Im(K(eps_w)) as kidmp::mie_cloud_absorption forms it."""
    ew = complex(cfg.eps_w)
    r = 1.0 / ((ew.real + 2.0) * (ew.real + 2.0) + ew.imag * ew.imag)
    k_im = (ew.imag * (ew.real + 2.0) - (ew.real - 1.0) * ew.imag) * r
    return (6.0 * PI / cfg.wavelength) * k_im


def sums(x, par, has, D, dD, rows):
    """A, B, E, M, V [ncol, nz] of species x in the kernel's order."""
    A, B, E, M, V = (np.zeros(has.shape) for _ in range(5))
    for b in range(len(D)):
        with np.errstate(all="ignore"):
            n = np.where(has, bbr.density(x, par, D[b], dD[b]), 0.0)
            ns = n * rows[0, b]
            A += ns
            B += n * rows[1, b]
            E += n * rows[2, b]
            M += n * rows[3, b]
            V += ns * rows[4, b]
    return A, B, E, M, V


def wave_scan(v, down):
    """Kogge-Stone inclusive scan over 64 lanes as wave_prefix_sum forms it; v [..., 64]."""
    v = v.copy()
    lane = np.arange(64)
    d = 1
    while d < 64:
        o = np.zeros_like(v)
        if down:
            o[..., :64 - d] = v[..., d:]
            v = np.where(lane + d < 64, v + o, v)
        else:
            o[..., d:] = v[..., :64 - d]
            v = np.where(lane >= d, v + o, v)
        d <<= 1
    return v


def column_depths(dt):
    """(up, dn) [ncol, nz]: the exclusive sums below and above each level as column_depths chains the level groups."""
    ncol, nz = dt.shape
    nj = (nz + 63) // 64
    pad = np.zeros((ncol, 64 * nj))
    pad[:, :nz] = dt
    g = pad.reshape(ncol, nj, 64)
    up, dn = np.zeros_like(g), np.zeros_like(g)
    carry = np.zeros(ncol)
    for j in range(nj):
        inc = wave_scan(g[:, j], False)
        up[:, j, 1:] = carry[:, None] + inc[:, :-1]
        up[:, j, 0] = carry + 0.0
        carry = carry + inc[:, 63]
    carry = np.zeros(ncol)
    for j in range(nj - 1, -1, -1):
        inc = wave_scan(g[:, j], True)
        dn[:, j, :-1] = carry[:, None] + inc[:, 1:]
        dn[:, j, 63] = carry + 0.0
        carry = carry + inc[:, 0]
    return up.reshape(ncol, -1)[:, :nz], dn.reshape(ncol, -1)[:, :nz]


def wave_total(dt):
    """The column's sum as the kernel forms it: per lane over the level groups ascending, then the butterfly xor 1, 2, ..., 32."""
    ncol, nz = dt.shape
    nj = (nz + 63) // 64
    pad = np.zeros((ncol, 64 * nj))
    pad[:, :nz] = dt
    g = pad.reshape(ncol, nj, 64)
    s = np.zeros((ncol, 64))
    for j in range(nj):
        s = s + g[:, j]
    idx = np.arange(64)
    for m in (1, 2, 4, 8, 16, 32):
        s = s + s[:, idx ^ m]
    return s[:, 0]


def mie_radar(c, cfg, table, st, dz=None, w=None, k_gas=None, warm=False):
    """Every output of NAMES.  c: refl_oracle.constants; cfg: the table's configuration (wavelength, eps_w, rho_w);
    table: species -> (D, dD, rows[5, nb]) as kidmp_mie_table_get returns them; st: numpy [ncol, nz], missing or None qc,
    qs, qg = 0; warm: an iiwarm context.  Also the locals ze_r, ze_s, ze_g (closed-form), A_x, B_x."""
    z = np.zeros_like(np.asarray(st["t"], dtype=np.float64))
    g = lambda k: np.asarray(st[k], dtype=np.float64) if st.get(k) is not None else z   # noqa: E731
    qs, qg = (z, z) if warm else (g("qs"), g("qg"))
    ze_r, ze_s, ze_g, v, ilamg, N0_g = ro.ze_terms(c, g("qv"), g("qr"), g("nr"), qs, qg, g("t"), g("p"))
    rho = v["rho"]
    rhof = np.sqrt(dr.RHO_NOT / rho)
    with np.errstate(all="ignore"):
        smoc, smob = dr.snow_smoc(c, v["temp"], v["rs"])
        par = {"r": dict(N0=v["N0_r"], lam=1.0 / v["ilamr"]), "s": dict(smob=smob, smoc=smoc), "g": dict(N0=N0_g, lam=1.0 / ilamg)}
    has = {"r": v["L_qr"], "s": v["L_qs"], "g": v["L_qg"]}
    rq = {"r": g("qr") * rho, "s": v["rs"], "g": v["rg"]}
    ze = {"r": ze_r, "s": ze_s, "g": ze_g}
    out = dict(ze_r=ze_r, ze_s=ze_s, ze_g=ze_g)
    ext, zw, zv = np.zeros_like(z), np.zeros_like(z), np.zeros_like(z)
    zp = {}
    for x in SPECIES:
        D, dD, rows = table[x]
        A, B, E, M, V = sums(x, par[x], has[x], D, dD, rows)
        with np.errstate(all="ignore"):
            okb = has[x] & (B > 0.0)
            mie = np.where(okb, A / np.where(okb, B, 1.0), 1.0)
            zp[x] = ze[x] * mie
            okm = has[x] & (M > 0.0)
            ext = ext + np.where(okm, rq[x] * E / np.where(okm, M, 1.0), 0.0)
            oka = has[x] & (A > 0.0)
            zw = np.where(oka, zw + zp[x], zw)
            zv = np.where(oka, zv + zp[x] * (V / np.where(oka, A, 1.0)), zv)
        out["mie_" + x], out["A_" + x], out["B_" + x] = mie, A, B
        out["dbz_" + x] = 10.0 * np.log10(zp[x] * 1.e18)
    out["dbz"] = 10.0 * np.log10((zp["r"] + zp["s"] + zp["g"]) * 1.e18)
    wind = z if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        echo = zw > 0.0
        out["vd"] = np.where(echo, rhof * (zv / np.where(echo, zw, 1.0)) - wind, 0.0)
    qc = g("qc")
    ext = np.where(qc > R1, ext + cloud_factor(cfg) * ((rho * qc) / cfg.rho_w), ext)
    if k_gas is not None:
        ext = ext + np.broadcast_to(np.asarray(k_gas, dtype=np.float64), z.shape)
    out["ext"] = ext
    if dz is not None:
        dt = ext * np.broadcast_to(np.asarray(dz, dtype=np.float64), z.shape)
        up, dn = column_depths(dt)
        out["pia_up"], out["pia_down"] = PIA * (up + 0.5 * dt), PIA * (dn + 0.5 * dt)
        out["dbz_up"], out["dbz_down"] = out["dbz"] - out["pia_up"], out["dbz"] - out["pia_down"]
        out["pia_total"] = PIA * wave_total(dt)
    return out


def rayleigh_gap(table):
    """The largest |s_mie/s_ray - 1| of a table: what bounds mie_x - 1 of any size distribution on it."""
    return max(float(np.max(np.abs(rows[0] / rows[1] - 1.0))) for _, _, rows in table.values())


def ulps(got, want):
    """|got - want| in units of the spacing of `want`."""
    with np.errstate(all="ignore"):
        return np.abs(got - want) / np.spacing(np.abs(want))


def cfg_of(wavelength, eps_w, eps_i, rho_w=1000.0, rho_i=917.0, kw2=0.75):
    class Cfg:
        pass
    c = Cfg()
    c.wavelength, c.eps_w, c.eps_i, c.rho_w, c.rho_i, c.kw2 = wavelength, complex(eps_w), complex(eps_i), rho_w, rho_i, kw2
    return c


assert math.isclose(PIA, 20.0 / math.log(10.0), rel_tol=1e-15)
