"""The numpy restatement of include/kidmp_slab.h: the z part is tests/kid_advect_ref.py's `advect`, the x part is written
with np.roll along x in the header's order of operations (numpy rounds every array operation once and never contracts).
The GPU tests hold the kernel to `advect_slab` bit for bit; tests/test_kid_slab_abi.py checks the scheme's properties on
it.  `streamfunction_flow` restates kid_amd.slab.streamfunction_flow."""
import numpy as np

import kid_advect_ref as ref

FIELDS, WARM = ref.FIELDS, ref.WARM


def _per_column(a, nslab, nx):
    """[nx, n] (one flow for every slab) or [nslab*nx, n] -> [nslab, nx, n] in binary64."""
    a = np.asarray(a, dtype=np.float64)
    assert a.ndim == 2 and a.shape[0] in (nx, nslab * nx), a.shape
    if a.shape[0] == nx:
        a = np.broadcast_to(a[None], (nslab,) + a.shape)
    return np.ascontiguousarray(a.reshape(nslab, nx, a.shape[-1]))


def advect_slab(state, u, w, rho, dz, dx, dt, nx, keys=None):
    """state: dict name -> [ncol, nz] (any float dtype: widened), ncol = nslab*nx; u [nx, nz] or [ncol, nz] at the left
    faces, w [nx, nz+1] or [ncol, nz+1].  Returns "adv", "div", "sum" (dicts of float64 [ncol, nz]), "courant" [ncol], and
    for the property tests Fz [member][ncol, nz+1], Fx [member][ncol, nz] (at the left faces), Mz, Mx, cz, cx, den, denx."""
    dt, dx = float(dt), float(dx)
    keys = list(keys) if keys is not None else [k for k in FIELDS if state.get(k) is not None]
    ncol, nz = np.asarray(state[keys[0]]).shape
    assert ncol % nx == 0 and nx >= 3
    nslab = ncol // nx
    rho = np.asarray(rho, dtype=np.float64)
    u3, w3 = _per_column(u, nslab, nx), _per_column(w, nslab, nx)
    assert u3.shape[-1] == nz and w3.shape[-1] == nz + 1
    z = ref.advect(state, w3.reshape(ncol, nz + 1), rho, dz, dt, keys)
    Mx = rho * u3
    cx = (np.abs(u3) * dt) / dx
    pos = u3 >= 0.0
    denx = rho * dx
    dMx = (np.roll(Mx, -1, axis=1) - Mx) / denx
    out = {"adv": {}, "div": {}, "sum": {}, "Fz": z["F"], "Fx": {}, "Mz": z["M"], "Mx": Mx.reshape(ncol, nz), "cz": z["c"],
           "cx": cx.reshape(ncol, nz), "den": z["den"], "denx": denx}
    for k in keys:
        q = np.asarray(state[k], dtype=np.float64).reshape(nslab, nx, nz)
        left, left2, right = np.roll(q, 1, axis=1), np.roll(q, 2, axis=1), np.roll(q, -1, axis=1)     # cells i-1, i-2, i+1
        qu, qd, quu = np.where(pos, left, q), np.where(pos, q, left), np.where(pos, left2, right)
        dq = qd - qu
        b = qu - quu
        bd = b * dq
        s = np.zeros_like(bd)
        np.divide(2.0 * bd, b + dq, out=s, where=bd > 0.0)
        qf = qu + (0.5 * (1.0 - cx)) * s
        Fx = Mx * qf
        advx = -((np.roll(Fx, -1, axis=1) - Fx) / denx)
        divx = q * dMx
        adv = z["adv"][k] + advx.reshape(ncol, nz)
        div = z["div"][k] + divx.reshape(ncol, nz)
        out["adv"][k], out["div"][k], out["sum"][k], out["Fx"][k] = adv, div, adv + div, Fx.reshape(ncol, nz)
    cz = np.broadcast_to(z["c"], (ncol, nz + 1))
    both = np.maximum(cz[:, :-1], cz[:, 1:]) + np.maximum(cx, np.roll(cx, -1, axis=1)).reshape(ncol, nz)
    out["courant"] = both.max(axis=1)
    return out


def streamfunction_flow(psi, rho, dz, dx, nx=None):
    """psi [nx, nz+1] (or [ncol, nz+1] with nx given) at the left, lower cell corners -> (u [.., nz], w [.., nz+1])."""
    psi, rho, dz = (np.asarray(a, dtype=np.float64) for a in (psi, rho, dz))
    nz = rho.shape[0]
    rf = np.concatenate([rho[:1], 0.5 * (rho[:-1] + rho[1:]), rho[-1:]])
    u = (-(psi[:, 1:] - psi[:, :-1]) / dz) / rho
    p3 = psi.reshape(-1, nx or psi.shape[0], nz + 1)
    w = ((np.roll(p3, -1, axis=1) - p3) / float(dx)).reshape(psi.shape) / rf
    return np.ascontiguousarray(u), np.ascontiguousarray(w)
