"""include/kidmp_specproc.h restated in numpy, operation for operation: the window, the weights and their norm, the
broadened signal with its ascending sums, what leaves the grid, detection and the moments.  Every array is [ncol, nz] (one
value per column and level) and the loops over bins and offsets are Python's, so each product and each sum rounds once in
the stated order.  The only difference from the kernel is the exponential (numpy's here, fastmath.h's there) and log10.
"""
import numpy as np

NAMES = ("spec", "lost_below", "lost_above", "dbz", "vm", "sw", "skew", "kurt", "v_lo", "v_hi", "nbins")
MAX_HALF = 256
EXP_MAX = 700.0


def bits(a):
    a = np.asarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def window(sigma, inv_dv, cut):
    """(s, H) of sigma [...]: H = 0 where !(sigma > 0)."""
    sigma = np.asarray(sigma, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        pos = sigma > 0.0
        s = np.where(pos, sigma * inv_dv, 0.0)
        h = np.ceil(cut * s)
        H = np.where(pos, np.where(h > MAX_HALF, MAX_HALF, h), 0.0).astype(np.int64)
    return s, H


def weights(s, H):
    """g [Hmax+1, ...] (g[0] = 1; g[d] is meaningful where d <= H) and G."""
    hmax = int(H.max()) if H.size else 0
    g = np.zeros((hmax + 1,) + H.shape)
    g[0] = 1.0
    G = np.ones(H.shape)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for d in range(1, hmax + 1):
            r = float(d) / s
            t = 0.5 * (r * r)
            gd = np.where(t <= EXP_MAX, np.exp(-np.where(t <= EXP_MAX, t, 0.0)), 0.0)
            on = d <= H
            g[d] = np.where(on, gd, 0.0)
            G = np.where(on, G + (gd + gd), G)
    return g, G


def tails(g, H):
    """T [Hmax+2, ...]: T[m] = sum_{d = m .. H} g_d from d = H down; T[m] = 0 beyond H."""
    hmax = g.shape[0] - 1
    T = np.zeros((hmax + 2,) + H.shape)
    t = np.zeros(H.shape)
    for d in range(hmax, 0, -1):
        t = np.where(d <= H, t + g[d], t)
        T[d] = t
    return T


def kernel_variance(g, G, H):
    """sum_d d**2 g_d / G over d = -H .. H of the discrete kernel, in bins**2."""
    acc = np.zeros(H.shape)
    for d in range(1, g.shape[0]):
        acc = acc + np.where(d <= H, 2.0 * d * d * g[d], 0.0)
    return acc / G


def _per_level(a, ncol, nz, what):
    if a is None:
        return None
    a = np.asarray(a, dtype=np.float64)
    assert a.shape in ((nz,), (ncol, nz)), (what, a.shape)
    return np.broadcast_to(a, (ncol, nz))


def process(spec, v0, dv, sigma=None, noise=None, cut=4.0, snr_min=1.0, add_noise=False, parts=False):
    """The operator on spec [ncol, nv, nz] (float64).  Returns a dict over NAMES; with parts=True also H, G, g, T, B (the
    signal before add_noise), det (the detection mask [ncol, nv, nz]) and margin (the smallest |B - thr|/max(|B|, |thr|)
    over all bins, 0 where both are 0)."""
    x = np.asarray(spec, dtype=np.float64)
    ncol, nv, nz = x.shape
    inv_dv = 1.0 / dv
    sig = _per_level(sigma, ncol, nz, "sigma")
    n = _per_level(noise, ncol, nz, "noise")
    nk = np.zeros((ncol, nz)) if n is None else n
    s, H = window(np.zeros((ncol, nz)) if sig is None else sig, inv_dv, cut)
    g, G = weights(s, H)
    hmax = g.shape[0] - 1
    B = np.empty_like(x)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for j in range(nv):
            acc = np.zeros((ncol, nz))
            for i in range(max(0, j - hmax), min(nv - 1, j + hmax) + 1):
                d = abs(j - i)
                acc = np.where(d <= H, acc + g[d] * x[:, i, :], acc)
            B[:, j, :] = np.where(H > 0, acc / G, x[:, j, :])
        T = tails(g, H)
        nb = np.minimum(H, nv)
        below, above = np.zeros((ncol, nz)), np.zeros((ncol, nz))
        for i in range(min(hmax, nv)):
            below = np.where(i < nb, below + x[:, i, :] * T[i + 1], below)
        for i in range(max(0, nv - hmax), nv):
            above = np.where(i >= nv - nb, above + x[:, i, :] * T[nv - i], above)
        below = np.where(H > 0, below / G, 0.0)
        above = np.where(H > 0, above / G, 0.0)
        thr = snr_min * nk
        det = B > thr[:, None, :]
        z, m1 = np.zeros((ncol, nz)), np.zeros((ncol, nz))
        v_lo, v_hi = np.zeros((ncol, nz)), np.zeros((ncol, nz))
        nbins = np.zeros((ncol, nz), dtype=np.int32)
        for j in range(nv):
            v = v0 + float(j) * dv
            dj = det[:, j, :]
            z = np.where(dj, z + B[:, j, :], z)
            m1 = np.where(dj, m1 + v * B[:, j, :], m1)
            v_lo = np.where(dj & (nbins == 0), v, v_lo)
            v_hi = np.where(dj, v, v_hi)
            nbins = nbins + dj.astype(np.int32)
        some = nbins > 0
        vm = np.where(some, m1 / np.where(some, z, 1.0), 0.0)
        vm = np.where(vm < v_lo, v_lo, np.where(vm > v_hi, v_hi, vm))
        c2, c3, c4 = np.zeros((ncol, nz)), np.zeros((ncol, nz)), np.zeros((ncol, nz))
        for j in range(nv):
            e = (v0 + float(j) * dv) - vm
            q = e * e
            dj = det[:, j, :]
            c2 = np.where(dj, c2 + q * B[:, j, :], c2)
            c3 = np.where(dj, c3 + (q * e) * B[:, j, :], c3)
            c4 = np.where(dj, c4 + (q * q) * B[:, j, :], c4)
        zs = np.where(some, z, 1.0)
        var = c2 / zs
        sw = np.where(some & (var > 0.0), np.sqrt(np.where(var > 0.0, var, 0.0)), 0.0)
        wide = sw != 0.0
        s1 = np.where(wide, sw, 1.0)
        skew = np.where(wide, (c3 / zs) / ((s1 * s1) * s1), 0.0)
        kurt = np.where(wide, (c4 / zs) / ((s1 * s1) * (s1 * s1)), 0.0)
        dbz = np.where(some, 10.0 * np.log10(np.where(z > 1e-22, z, 1e-22) * 1e18), -40.0)
        out = {"spec": B + nk[:, None, :] if add_noise else B.copy(), "lost_below": below, "lost_above": above, "dbz": dbz, "vm": vm, "sw": sw,
               "skew": skew, "kurt": kurt, "v_lo": v_lo, "v_hi": v_hi, "nbins": nbins}
        if parts:
            scale = np.maximum(np.abs(B), np.abs(thr)[:, None, :])
            gap = np.abs(B - thr[:, None, :])
            margin = np.where(scale > 0.0, gap / np.where(scale > 0.0, scale, 1.0), 0.0)
            out.update(H=H, G=G, g=g, T=T, B=B, det=det, margin=float(margin.min()) if margin.size else 1.0, s=s)
    return out
