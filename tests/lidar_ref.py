"""The lidar operator of include/kidmp_lidar.h in numpy: a restatement of the header's definitions on the profiles of
size_spectra_ref.parameters and the loaded droplet number of size_spectra_ref.cloud, with serial np.cumsum for the optical
depths.  The definitions are this library's own (the reference holds no lidar operator): this file pins them, and parity
with an instrument simulator is not pinned."""
import numpy as np

import size_spectra_ref as ssr

NAMES = ("ext_c", "ext_i", "ext_r", "ext_s", "ext_g", "ext", "bsc", "bsc_mol", "tau_up", "tau_dn", "att_up", "att_dn", "sr_up", "sr_dn")
LOCAL = NAMES[:8]                                     # need no neighbouring level
SUMMARY_NAMES = ("tau_part", "tau_mol", "z_base_up", "z_lost_up", "z_top_dn", "z_lost_dn", "n_up", "n_dn")
TAU_PART, TAU_MOL, Z_BASE_UP, Z_LOST_UP, Z_TOP_DN, Z_LOST_DN, N_UP, N_DN = range(8)
INPUTS = ssr.INPUTS
SPECIES = ssr.SPECIES                                 # the order of s_ratio: c, i, r, s, g
K_B = 1.380649e-23
EXP_MAX = ssr.EXP_MAX
U = 2.0 ** -53
R_GAS = 287.04


def cfg(s_ratio=(18.8, 25.0, 18.8, 25.0, 25.0), eta=0.7, c_mol=6.2446e-32, beta_detect=2.0e-5, trans_lost=2.5e-3):
    """A configuration as a dict; the defaults are those of a NULL kidmp_lidar_cfg (no test rests on them)."""
    return dict(s_ratio=tuple(float(x) for x in s_ratio), eta=float(eta), c_mol=float(c_mol), beta_detect=float(beta_detect),
                trans_lost=float(trans_lost))


def E(x):
    """EXP(-x), exact +0.0 past 700."""
    return ssr._exp_neg(np.asarray(x, dtype=np.float64))


def g(x):
    """(1 - EXP(-x))/x for x >= 0, the mean of EXP(-x') over [0, x], without cancellation: EXP(-x/2)*sinh(x/2)/(x/2) below
    1 (numpy's sinh is good to an ulp at small arguments), as written from 1 on with the 700 rule in E; g(0) = 1."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        y = 0.5 * np.where(x < 1.0, x, 0.0)
        small = np.exp(-y) * np.where(y > 1e-150, np.sinh(y) / np.where(y > 1e-150, y, 1.0), 1.0)
        large = (1.0 - E(x)) / np.where(x < 1.0, 1.0, x)
    return np.where(x < 1.0, small, large)


def _dz(dz, shape):
    dz = np.asarray(dz, dtype=np.float64)
    return np.broadcast_to(dz, shape) if dz.ndim == 1 else dz


def _below(a):
    """Exclusive serial prefix sum along the levels: sum_{k' < k} a(k')."""
    s = np.cumsum(a, axis=-1)
    return np.concatenate([np.zeros_like(s[..., :1]), s[..., :-1]], axis=-1)


def _above(a):
    return _below(a[..., ::-1])[..., ::-1]


def extinctions(c, st, warm=False, aero=False, Nt_c=None):
    """ext_c .. ext_g [..., nz] (+0.0 where the species is absent) and has_x, from the size spectra's parameters."""
    par = ssr.parameters(c, st, warm, aero, Nt_c)
    t, p = np.asarray(st["t"], dtype=np.float64), np.asarray(st["p"], dtype=np.float64)
    rho = 0.622 * p / (R_GAS * t * (np.maximum(1e-10, np.asarray(st["qv"], dtype=np.float64)) + 0.622))
    _, nc, nu, _, _ = ssr.cloud(c, rho, np.asarray(st["qc"], dtype=np.float64),
                                np.asarray(st["nc"], dtype=np.float64) if aero else np.zeros_like(rho), aero, Nt_c)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for x in "irg":
            lam, n0 = par["lam_" + x], par["n0_" + x]
            out["ext_" + x] = np.where(par["has_" + x], np.pi * n0 / (lam * lam * lam), 0.0)
        lamc = par["lam_c"]
        out["ext_c"] = np.where(par["has_c"], (0.5 * np.pi) * nc * ((nu + 1) * (nu + 2)).astype(np.float64) / (lamc * lamc), 0.0)
        out["ext_s"] = np.where(par["has_s"], (0.5 * np.pi) * par["smob"], 0.0)
    for x in SPECIES:
        out["has_" + x] = par["has_" + x]
    out["par"] = par
    return out


def profiles(c, st, dz, cf, warm=False, aero=False, Nt_c=None):
    """The fourteen profiles of NAMES and what the bounds of the GPU test read: dtau, dtau_mol, tau_incl_up / _dn
    (tau + dtau), tau_column and taum_column [..., 1], attm_up / _dn, taum_up / _dn, ext_mol, has_x."""
    o = extinctions(c, st, warm, aero, Nt_c)
    t, p = np.asarray(st["t"], dtype=np.float64), np.asarray(st["p"], dtype=np.float64)
    S = cf["s_ratio"]
    o["ext"] = (((o["ext_c"] + o["ext_i"]) + o["ext_r"]) + o["ext_s"]) + o["ext_g"]
    o["bsc"] = (((o["ext_c"] / S[0] + o["ext_i"] / S[1]) + o["ext_r"] / S[2]) + o["ext_s"] / S[3]) + o["ext_g"] / S[4]
    o["bsc_mol"] = cf["c_mol"] * (p / (K_B * t))
    o["ext_mol"] = (8.0 * np.pi / 3.0) * o["bsc_mol"]
    if dz is None:
        return o
    dz = _dz(dz, t.shape)
    o["dz"] = dz
    o["dtau"] = (cf["eta"] * o["ext"] + o["ext_mol"]) * dz
    o["dtau_mol"] = o["ext_mol"] * dz
    o["tau_up"], o["tau_dn"] = _below(o["dtau"]), _above(o["dtau"])
    o["taum_up"], o["taum_dn"] = _below(o["dtau_mol"]), _above(o["dtau_mol"])
    o["tau_column"] = np.sum(o["dtau"], axis=-1, keepdims=True)
    o["taum_column"] = np.sum(o["dtau_mol"], axis=-1, keepdims=True)
    gl, gm = g(2.0 * o["dtau"]), g(2.0 * o["dtau_mol"])
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        for d in ("up", "dn"):
            o["tau_incl_" + d] = o["tau_" + d] + o["dtau"]
            o["att_" + d] = (o["bsc"] + o["bsc_mol"]) * E(2.0 * o["tau_" + d]) * gl
            o["attm_" + d] = o["bsc_mol"] * E(2.0 * o["taum_" + d]) * gm
            o["sr_" + d] = o["att_" + d] / o["attm_" + d]
            o["trans_" + d] = E(2.0 * o["tau_incl_" + d])
    return o


def levels(o, cf):
    """[ncol, 4] int: the levels of slots 2..5 (-1: none), and the counts n_up, n_dn [ncol]."""
    nz = o["att_up"].shape[-1]
    det_up, det_dn = o["att_up"] >= cf["beta_detect"], o["att_dn"] >= cf["beta_detect"]
    lost_up, lost_dn = o["trans_up"] < cf["trans_lost"], o["trans_dn"] < cf["trans_lost"]
    first = lambda m: np.where(m.any(axis=1), m.argmax(axis=1), -1)                 # noqa: E731
    last = lambda m: np.where(m.any(axis=1), nz - 1 - m[:, ::-1].argmax(axis=1), -1)   # noqa: E731
    return np.stack([first(det_up), first(lost_up), last(det_dn), last(lost_dn)], axis=1), det_up.sum(axis=1), det_dn.sum(axis=1)


def summary(o, cf):
    """[ncol, 8] of the header, from profiles() of a [ncol, nz] state; and the chosen levels [ncol, 4]."""
    k, n_up, n_dn = levels(o, cf)
    ncol = k.shape[0]
    out = np.full((ncol, 8), np.nan)
    zb = _below(o["dz"])                                                             # bottom faces
    zt = zb + o["dz"]
    out[:, TAU_PART] = np.cumsum(o["ext"] * o["dz"], axis=-1)[:, -1]
    out[:, TAU_MOL] = np.cumsum(o["dtau_mol"], axis=-1)[:, -1]
    for slot, col, face in ((Z_BASE_UP, 0, zb), (Z_LOST_UP, 1, zt), (Z_TOP_DN, 2, zt), (Z_LOST_DN, 3, zb)):
        some = k[:, col] >= 0
        out[some, slot] = face[np.nonzero(some)[0], k[some, col]]
    out[:, N_UP], out[:, N_DN] = n_up, n_dn
    return out, k


def threshold(values, quantile=0.5, gap=1e-6):
    """A threshold that no value lies near: the geometric mean of the two adjacent distinct sorted positive values closest to
    `quantile` whose ratio exceeds 1 + gap.  None if there is no such pair."""
    v = np.unique(np.asarray(values, dtype=np.float64).ravel())
    v = v[np.isfinite(v) & (v > 1e-290)]
    if v.size < 2:
        return None
    ok = np.nonzero(v[1:] / v[:-1] > 1.0 + gap)[0]
    if ok.size == 0:
        return None
    i = ok[np.abs(ok - quantile * (v.size - 1)).argmin()]
    return float(np.sqrt(v[i]) * np.sqrt(v[i + 1]))


def with_thresholds(o, cf, quantile=0.5):
    """cf with beta_detect and trans_lost chosen from the reference's own values, so that no level lies within a bound of a
    threshold; (cf, clear) where clear tells whether both could be chosen."""
    beta = threshold(np.concatenate([o["att_up"].ravel(), o["att_dn"].ravel()]), quantile)
    lost = threshold(np.concatenate([o["trans_up"].ravel(), o["trans_dn"].ravel()]), quantile)
    ok = beta is not None and lost is not None
    return dict(cf, beta_detect=beta if beta is not None else cf["beta_detect"], trans_lost=lost if lost is not None else cf["trans_lost"]), ok
