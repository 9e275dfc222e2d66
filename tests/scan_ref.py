"""The range-height scan of include/kidmp_scan.h restated in numpy, operation for operation (binary64, every operation
rounded once).  The path is the wave_scan / column_depths construction of tests/mie_radar_ref.py with gates in place of
levels; the beam uses numpy's exp and log where the kernel uses fastmath.h's, which is why a scan with nsub > 1 is held
to a bound and one with nsub = 1 to the bit.

geometry(...) returns what scan::sample of kid_amd/csrc/kidmp_scan_geom.h returns; scan(...) the six outputs.
"""
import math

import numpy as np

import mie_radar_ref as mrr

NAMES = ("dbz", "dbz_att", "pia", "vr", "height", "cell")
LN10 = 2.302585092994045684
PIA = 20.0 / LN10
DB_TO_LN, LN_TO_DB = LN10 / 10.0, 10.0 / LN10
SMALLEST_NORMAL = 2.2250738585072014e-308


def ray_valid(row, nslab):
    """The row can hit a cell at all: slab a whole number in [0, nslab), wgt finite and above 0."""
    slab, wgt = row[0], row[5]
    return bool(slab >= 0.0 and slab < float(nslab) and slab == np.floor(slab) and wgt > 0.0 and np.isfinite(wgt))


def geometry(row, zf, dx, nx, r0, dr, ngate, half_inv_ae, periodic):
    """(inside [ngate] bool, i, k [ngate] int64 (-1 outside), h [ngate]) of one row of the ray table; the row's slab and
    wgt are not looked at (ray_valid)."""
    zf = np.asarray(zf, dtype=np.float64)
    nz = zf.size - 1
    _, x0, z0, ce, se, _ = (np.float64(v) for v in row)
    g = np.arange(ngate, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.float64(r0) + (g + 0.5) * np.float64(dr)
        s = r * ce
        x = x0 + s
        h = (z0 + r * se) + (s * s) * np.float64(half_inv_ae)
        xi = np.floor(x / np.float64(dx))
    ok = np.isfinite(x) & np.isfinite(h)
    with np.errstate(all="ignore"):
        ok &= np.abs(xi) < 2.0 ** 52
    whole = np.where(ok, xi, 0.0).astype(np.int64)
    if periodic:
        i = np.mod(whole, nx)                                        # numpy's mod of whole numbers: in [0, nx)
    else:
        i = whole
        ok &= (whole >= 0) & (whole < nx)
    with np.errstate(all="ignore"):
        ok &= (zf[0] <= h) & (h < zf[nz])
    k = np.searchsorted(zf, np.where(ok, h, zf[0]), side="right") - 1   # the number of faces <= h, less one
    ok &= (k >= 0) & (k < nz)
    return ok, np.where(ok, i, -1), np.where(ok, k, -1), h


def _lin(t):
    """E of the header with numpy's exp."""
    with np.errstate(all="ignore"):
        return np.where(t > -700.0, np.exp(np.minimum(t, 700.0)), 0.0)


def _db(q):
    """L of the header with numpy's log, times 10/ln 10."""
    with np.errstate(all="ignore"):
        return np.where(q >= SMALLEST_NORMAL, LN_TO_DB * np.log(np.where(q >= SMALLEST_NORMAL, q, 1.0)), -np.inf)


def scan(fields, zf, rays, dx, nx, r0, dr, ngate, nsub, half_inv_ae=0.0, periodic=False, missing=float("nan"), parts=False):
    """dict name -> [nray, ngate] (float64; cell int32) of float64 fields {"dbz", "ext", "vd", "u"} [ncol, nz] (u may be
    [nx, nz]; ext, vd, u may be missing).  With parts=True also "scale" [nray, ngate]: max over the inside samples of
    |uc*ce| + |vd*se|, what a difference in vr is measured against."""
    dbz = np.asarray(fields["dbz"], dtype=np.float64)
    ncol, nz = dbz.shape
    nslab = ncol // nx
    ext, vd, u = (None if fields.get(n) is None else np.asarray(fields[n], dtype=np.float64) for n in ("ext", "vd", "u"))
    shared = u is not None and u.shape[0] == nx and ncol != nx
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, nsub, 6)
    nray = rays.shape[0]
    shape = (nray, nsub, ngate)
    inside = np.zeros(shape, dtype=bool)
    d, a, v, h = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.full(shape, np.nan)
    vscale = np.zeros(shape)
    flat = np.full(shape, -1, dtype=np.int64)
    for n in range(nray):
        for j in range(nsub):
            row = rays[n, j]
            valid = ray_valid(row, nslab)
            ok, i, k, hh = geometry(row, zf, dx, nx, r0, dr, ngate, half_inv_ae, periodic)
            if valid:
                h[n, j] = hh
            else:
                continue
            if not ok.any():
                continue
            gi, ii, kk = np.nonzero(ok)[0], i[ok], k[ok]
            col = int(row[0]) * nx + ii
            inside[n, j, gi] = True
            flat[n, j, gi] = col * nz + kk
            d[n, j, gi] = dbz[col, kk]
            if ext is not None:
                a[n, j, gi] = ext[col, kk] * np.float64(dr)
            uc = np.zeros(gi.size)
            if u is not None:
                ir = np.where(ii + 1 < nx, ii + 1, 0)
                c0, c1 = (ii, ir) if shared else (col, col - ii + ir)
                uc = 0.5 * (u[c0, kk] + u[c1, kk])
            vdv = vd[col, kk] if vd is not None else np.zeros(gi.size)
            v[n, j, gi] = uc * row[3] - vdv * row[4]
            vscale[n, j, gi] = np.abs(uc * row[3]) + np.abs(vdv * row[4])
    if ext is not None:
        up = mrr.column_depths(a.reshape(nray * nsub, ngate))[0].reshape(shape)
        tau = up + 0.5 * a
    else:
        tau = np.zeros(shape)
    p = PIA * tau
    with np.errstate(all="ignore"):
        e = d - p
    hits = inside.any(axis=1)
    out = {}
    if nsub == 1:
        vals = {"dbz": d[:, 0], "dbz_att": e[:, 0], "pia": p[:, 0], "vr": v[:, 0]}
    else:
        wgt = rays[:, :, 5][:, :, None]
        Sz, Sa, Sv, W = (np.zeros((nray, ngate)) for _ in range(4))
        with np.errstate(all="ignore"):
            for j in range(nsub):
                m = inside[:, j]
                z = wgt[:, j] * _lin(DB_TO_LN * d[:, j])
                za = wgt[:, j] * _lin(DB_TO_LN * e[:, j])
                Sz = np.where(m, Sz + z, Sz)
                Sa = np.where(m, Sa + za, Sa)
                Sv = np.where(m, Sv + za * v[:, j], Sv)
                W = np.where(m, W + wgt[:, j], W)
            Ws = np.where(hits, W, 1.0)
            o_dbz, o_att = _db(Sz / Ws), _db(Sa / Ws)
            vals = {"dbz": o_dbz, "dbz_att": o_att, "pia": o_dbz - o_att, "vr": np.where(Sa > 0.0, Sv / np.where(Sa > 0.0, Sa, 1.0), 0.0)}
    for n, val in vals.items():
        out[n] = np.where(hits, val, np.float64(missing))
    c = nsub // 2
    out["height"] = h[:, c]
    out["cell"] = flat[:, c].astype(np.int32)
    if parts:
        out["scale"] = np.where(inside, vscale, 0.0).max(axis=1)
        out["hits"] = hits
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def stretched_faces(nz, top=12000.0, ratio=1.02):
    """nz + 1 ascending faces from 0 to `top` whose layer depths grow by `ratio` per level."""
    dz = ratio ** np.arange(nz)
    zf = np.concatenate([[0.0], np.cumsum(dz)])
    return zf * (top / zf[-1])


def unit_rows(slab, x0, z0, elevations_deg):
    """Single-row rays with wgt = 1; 90 degrees gives ce = 0, se = 1 exactly."""
    rows = []
    for el in elevations_deg:
        ce, se = (0.0, 1.0) if el == 90.0 else (math.cos(math.radians(el)), math.sin(math.radians(el)))
        rows.append([float(slab), float(x0), float(z0), ce, se, 1.0])
    return np.array(rows)
