"""The numpy restatement of include/kidmp_advection.h's KIDMP_ADVECT_ULTIMATE: `advect` and `advect_slab` with the return
shape of tests/kid_advect_ref.py's `advect` and tests/kid_slab_ref.py's `advect_slab`, built on their `faces` and
`_per_column`; only the value at an interior face differs (`face_value`: Leonard's universal limiter on the QUICKEST face
value), in binary64 with the operations in the header's order (numpy rounds every array operation once and never
contracts).  The GPU tests hold the kernels to these functions bit for bit; tests/test_kid_ultimate_abi.py checks the
scheme's properties on them.  Beyond the shared keys the results hold "branch" (and "branch_x"): for every member the masks
of the faces that took each branch of the limiter, so that a bit test can show that it missed none."""
import numpy as np

import kid_advect_ref as ref
import kid_slab_ref as sref

FIELDS, WARM = ref.FIELDS, ref.WARM
# What a face value can come out as.  BRANCHES: the first-order fallback and, for a rising (dq > 0) and a falling face,
# the two clamps that bound the QUICKEST value from the downwind side: Leonard's reference value ref and the downwind cell.
# OTHER: QUICKEST itself, and the clamp at the upwind cell, which QUICKEST reaches through rounding only (in exact
# arithmetic qq - q[u] has the sign of dq for c < 1, and for c > 1 ref lies on the other side of q[u] and wins).
BRANCHES = ("upwind", "rising_reference", "rising_downwind", "falling_reference", "falling_downwind")
OTHER = ("rising_quickest", "falling_quickest", "rising_upwind_cell", "falling_upwind_cell")


def face_value(qu, qd, quu, c, inside=True):
    """(qf, masks) of faces with upwind, downwind and second upwind cells qu, qd, quu and Courant number c >= +0.0;
    `inside`: quu exists.  c == 0 gives rc = +inf and ref = +-inf (b != 0 where it is used)."""
    hc = 0.5 * (1.0 - c)
    g = (1.0 - c * c) / 6.0
    with np.errstate(divide="ignore"):
        rc = 1.0 / c
    dq = qd - qu
    b = qu - quu
    bd = b * dq
    lim = inside & (bd > 0.0)
    curv = dq - b
    qq = (qu + hc * dq) - g * curv
    with np.errstate(invalid="ignore", over="ignore"):            # 0*inf where the face falls back to upwind anyway
        reference = quu + b * rc
    rising = dq > 0.0
    t_is_qq = np.where(rising, qq > qu, qq < qu)
    t = np.where(t_is_qq, qq, qu)
    h_is_ref = np.where(rising, reference < qd, reference > qd)
    h = np.where(h_is_ref, reference, qd)
    takes_t = np.where(rising, t < h, t > h)
    qf = np.where(lim, np.where(takes_t, t, h), qu)
    masks = {"upwind": ~lim | np.zeros(qf.shape, dtype=bool)}
    for name, side in (("rising", lim & rising), ("falling", lim & ~rising)):
        masks[name + "_quickest"] = side & takes_t & t_is_qq
        masks[name + "_upwind_cell"] = side & takes_t & ~t_is_qq
        masks[name + "_reference"] = side & ~takes_t & h_is_ref
        masks[name + "_downwind"] = side & ~takes_t & ~h_is_ref
    return qf, masks


def advect(state, w, rho, dz, dt, keys=None):
    """As kid_advect_ref.advect: "adv", "div", "sum" (dicts of float64 [ncol, nz]), "courant" [ncol], F, M, den, c; and
    "branch" [member][name][ncol, nz-1], the masks of the interior faces 1 .. nz-1."""
    dt = float(dt)
    M, c, den, up = ref.faces(w, rho, dz, dt)
    nz = den.shape[0]
    out = {"adv": {}, "div": {}, "sum": {}, "F": {}, "M": M, "den": den, "c": c, "branch": {}}
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
        qf[:, 1:nz], out["branch"][k] = face_value(q[rows, iu], q[rows, idn], q[rows, np.clip(iuu, 0, nz - 1)], ck[:, 1:nz], inside)
        F = Mk * qf
        adv = -((F[:, 1:] - F[:, :-1]) / den[None, :])
        div = q * ((Mk[:, 1:] - Mk[:, :-1]) / den[None, :])
        out["adv"][k], out["div"][k], out["sum"][k], out["F"][k] = adv, div, adv + div, F
    ncol = next(iter(out["sum"].values())).shape[0] if out["sum"] else c.shape[0]
    out["courant"] = np.ascontiguousarray(np.broadcast_to(c.max(axis=1), (ncol,)))   # a shared profile: every column's
    return out


def advect_slab(state, u, w, rho, dz, dx, dt, nx, keys=None):
    """As kid_slab_ref.advect_slab, the z part `advect` above and the x part with `face_value`; "branch" holds the z masks,
    "branch_x" [member][name][ncol, nz] those of the left faces."""
    dt, dx = float(dt), float(dx)
    keys = list(keys) if keys is not None else [k for k in FIELDS if state.get(k) is not None]
    ncol, nz = np.asarray(state[keys[0]]).shape
    assert ncol % nx == 0 and nx >= 3
    nslab = ncol // nx
    rho = np.asarray(rho, dtype=np.float64)
    u3, w3 = sref._per_column(u, nslab, nx), sref._per_column(w, nslab, nx)
    assert u3.shape[-1] == nz and w3.shape[-1] == nz + 1
    z = advect(state, w3.reshape(ncol, nz + 1), rho, dz, dt, keys)
    Mx = rho * u3
    cx = (np.abs(u3) * dt) / dx
    pos = u3 >= 0.0
    denx = rho * dx
    dMx = (np.roll(Mx, -1, axis=1) - Mx) / denx
    out = {"adv": {}, "div": {}, "sum": {}, "Fz": z["F"], "Fx": {}, "Mz": z["M"], "Mx": Mx.reshape(ncol, nz), "cz": z["c"],
           "cx": cx.reshape(ncol, nz), "den": z["den"], "denx": denx, "branch": z["branch"], "branch_x": {}}
    for k in keys:
        q = np.asarray(state[k], dtype=np.float64).reshape(nslab, nx, nz)
        left, left2, right = np.roll(q, 1, axis=1), np.roll(q, 2, axis=1), np.roll(q, -1, axis=1)     # cells i-1, i-2, i+1
        qf, masks = face_value(np.where(pos, left, q), np.where(pos, q, left), np.where(pos, left2, right), cx)
        Fx = Mx * qf
        advx = -((np.roll(Fx, -1, axis=1) - Fx) / denx)
        divx = q * dMx
        adv = z["adv"][k] + advx.reshape(ncol, nz)
        div = z["div"][k] + divx.reshape(ncol, nz)
        out["adv"][k], out["div"][k], out["sum"][k], out["Fx"][k] = adv, div, adv + div, Fx.reshape(ncol, nz)
        out["branch_x"][k] = {n: m.reshape(ncol, nz) for n, m in masks.items()}
    cz = np.broadcast_to(z["c"], (ncol, nz + 1))
    both = np.maximum(cz[:, :-1], cz[:, 1:]) + np.maximum(cx, np.roll(cx, -1, axis=1)).reshape(ncol, nz)
    out["courant"] = both.max(axis=1)
    return out
