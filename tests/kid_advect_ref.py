"""The numpy restatement of include/kidmp_kinematic.h: `advect` in binary64 with the operations in the header's order
(numpy rounds every array operation once and never contracts), and `update` in the arrays' own format.  The GPU tests
hold the kernels to these functions bit for bit; tests/test_kid_advect_abi.py checks the scheme's properties on them."""
import numpy as np

FIELDS = ("theta", "qv", "qc", "qr", "nr", "qi", "ni", "qs", "qg")
WARM = FIELDS[:5]


def faces(w, rho, dz, dt):
    """What every member of a column shares: M [ncol, nz+1], c [ncol, nz+1], den [nz] and `up` (w >= 0)."""
    w = np.asarray(w, dtype=np.float64)
    rho, dz = np.asarray(rho, dtype=np.float64), np.asarray(dz, dtype=np.float64)
    nz = rho.shape[0]
    w = np.atleast_2d(w)
    assert w.shape[1] == nz + 1 and dz.shape == (nz,)
    rf = np.empty(nz + 1)
    rf[0], rf[nz] = rho[0], rho[nz - 1]
    rf[1:nz] = 0.5 * (rho[:nz - 1] + rho[1:])
    M = rf[None, :] * w
    up = w >= 0.0
    f = np.arange(nz + 1)
    u = np.clip(np.where(up, f[None, :] - 1, f[None, :]), 0, nz - 1)      # the boundary faces use dz[0] and dz[nz-1]
    c = (np.abs(w) * dt) / dz[u]
    return M, c, rho * dz, up


def advect(state, w, rho, dz, dt, keys=None):
    """state: dict name -> [ncol, nz] (any float dtype: widened); w [nz+1] or [ncol, nz+1].  Returns a dict with "adv",
    "div", "sum" (dicts of float64 [ncol, nz]), "courant" [ncol], and F [member][ncol, nz+1], M, den for the property tests."""
    dt = float(dt)
    M, c, den, up = faces(w, rho, dz, dt)
    nz = den.shape[0]
    out = {"adv": {}, "div": {}, "sum": {}, "F": {}, "M": M, "den": den, "c": c}
    for k in keys if keys is not None else [k for k in FIELDS if state.get(k) is not None]:
        q = np.asarray(state[k], dtype=np.float64)
        ncol = q.shape[0]
        Mk, ck, upk = (np.broadcast_to(a, (ncol, nz + 1)) for a in (M, c, up))
        qf = np.empty((ncol, nz + 1))
        qf[:, 0], qf[:, nz] = q[:, 0], q[:, nz - 1]
        f = np.arange(1, nz)[None, :]                                       # interior faces
        upi = upk[:, 1:nz]
        iu, idn, iuu = np.where(upi, f - 1, f), np.where(upi, f, f - 1), np.where(upi, f - 2, f + 1)
        inside = (iuu >= 0) & (iuu < nz)
        rows = np.arange(ncol)[:, None]
        qu, qd, quu = q[rows, iu], q[rows, idn], q[rows, np.clip(iuu, 0, nz - 1)]
        dq = qd - qu
        b = qu - quu
        bd = b * dq
        lim = inside & (bd > 0.0)
        s = np.zeros_like(bd)
        np.divide(2.0 * bd, b + dq, out=s, where=lim)
        qf[:, 1:nz] = qu + (0.5 * (1.0 - ck[:, 1:nz])) * s
        F = Mk * qf
        adv = -((F[:, 1:] - F[:, :-1]) / den[None, :])
        div = q * ((Mk[:, 1:] - Mk[:, :-1]) / den[None, :])
        out["adv"][k], out["div"][k], out["sum"][k], out["F"][k] = adv, div, adv + div, F
    ncol = next(iter(out["sum"].values())).shape[0] if out["sum"] else c.shape[0]
    out["courant"] = np.ascontiguousarray(np.broadcast_to(c.max(axis=1), (ncol,)))   # a shared profile: every column's
    return out


def update(state, dt, *tendencies, clip=True, keys=None):
    """X + ((t1 + t2) + t3)*dt in the arrays' own format, then the clip of everything but theta.  Returns new arrays."""
    out = {}
    for k in keys if keys is not None else [k for k in FIELDS if state.get(k) is not None]:
        x = state[k]
        T = x.dtype.type
        t = [np.zeros_like(x) if (i >= len(tendencies) or tendencies[i] is None or tendencies[i].get(k) is None) else tendencies[i][k]
             for i in range(3)]
        assert all(a.dtype == x.dtype for a in t)
        y = x + ((t[0] + t[1]) + t[2]) * T(dt)
        assert y.dtype == x.dtype
        if clip and k != "theta":
            y = np.where(y < 0, T(0), y)
        out[k] = y
    return out
