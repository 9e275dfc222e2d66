"""Hand-built columns for the bright-band tests: rain below a layer of snow and graupel, the temperature crossing 273.15
between the levels k0 - 1 and k0.  Every kind of column is one situation of include/kidmp_brightband.h:

  0  the melting level near the middle, snow and graupel thinning out over the six levels below it
  1  k0 = 1: one melting level
  2  k0 = nz - 1
  3  only snow at k0, graupel below it: graupel stays dry
  4  more snow below than at k0 (rs[k] > rs[k0]): the 0.05 floor
  5  cold everywhere, no rain: no melting level
  6  k0 = nz - 1 and every level below it warm, rainy, snowy and with graupel: 2 (nz - 1) active pairs
  7  warm rain alone: no melting level
  8  k0 high up (level 130 where the column has it) and the only snow below it in the levels 3 .. 40: the melting level in a
     higher level group than the active levels
"""
import numpy as np

INPUTS = ("t", "p", "qv", "qr", "nr", "qs", "qg")
KINDS = 9


def target_k0(nz, kind, rng):
    if kind == 1:
        return 1
    if kind in (2, 6):
        return nz - 1
    if kind == 8:
        return max(1, min(nz - 1, 130))
    return max(1, min(nz - 1, nz // 2 + int(rng.integers(-2, 3))))


def column(nz, kind, rng):
    """One column [nz] per input and the melting level it is built to have (-1: none)."""
    st = {n: np.zeros(nz) for n in INPUTS}
    k = np.arange(nz)
    k0 = target_k0(nz, kind, rng)
    st["p"][:] = 9.5e4 * np.exp(-1.2 * k / nz)
    st["qv"][:] = 4.0e-3 * np.exp(-3.0 * k / nz)
    st["t"][:] = 273.15 + (k0 - 0.5 - k) * min(0.6, 40.0 / nz)
    if kind == 5:
        st["t"][:] = 268.0 - 0.1 * k
        st["qs"][:] = 6.0e-4 * rng.uniform(0.5, 1.5, nz)
        st["qg"][:] = 3.0e-4 * rng.uniform(0.5, 1.5, nz)
        return st, -1
    below = k < k0
    st["qr"][below] = 1.0e-3 * rng.uniform(0.5, 1.5, int(below.sum()))
    st["nr"][below] = 1.0e4 * rng.uniform(0.5, 2.0, int(below.sum()))
    if kind == 7:
        st["t"][:] = 290.0 - 0.05 * k
        return st, -1
    st["qs"][~below] = 8.0e-4 * rng.uniform(0.7, 1.3, int((~below).sum()))
    st["qg"][~below] = 5.0e-4 * rng.uniform(0.7, 1.3, int((~below).sum()))
    depth = k0 if kind == 6 else min(k0, 6)
    melt = (k >= k0 - depth) & below
    thin = 1.0 - (k0 - k[melt]) / (depth + 1.0)
    st["qs"][melt] = st["qs"][k0] * (1.6 if kind == 4 else thin)
    st["qg"][melt] = st["qg"][k0] * thin
    if kind == 3:
        st["qg"][k0] = 0.0
    if kind == 8:
        st["qs"][below] = 0.0
        st["qg"][below] = 0.0
        st["qs"][3:min(41, k0)] = 4.0e-4 * rng.uniform(0.2, 0.9, max(0, min(41, k0) - 3))
    return st, k0


def batch(nz, ncol, seed, kinds=None):
    """A state [ncol, nz] whose column c is of kind kinds[c % len(kinds)], and the melting levels it is built to have."""
    rng = np.random.Generator(np.random.PCG64(seed))
    kinds = tuple(range(KINDS)) if kinds is None else kinds
    cols = [column(nz, kinds[c % len(kinds)], rng) for c in range(ncol)]
    return {n: np.ascontiguousarray(np.stack([c[0][n] for c in cols])) for n in INPUTS}, np.array([c[1] for c in cols], dtype=np.int32)
