"""The inputs of the spectrum processor's tests (tests/test_specproc_abi.py, tests/test_gpu_specproc.py): shapes, widths
that put the half-width H of the broadening window at every edge of the kernel, and seeded spectra.

The kernel walks the velocity axis in tiles of TILE output bins and keeps the first KEPT + 1 weights of a level in LDS,
forming the others where they are used: H = TILE - 1, TILE, TILE + 1 and KEPT, KEPT + 1 are the edges of its paths, beside
H = 0, 1, H >= nv and the cap 256.
"""
import numpy as np

NZS = (2, 65, 120, 256)
NVS = (1, 2, 25, 64, 256)
NCOLS = (1, 3, 5)
TILE, KEPT, CAP = 8, 16, 256
DV = 0.125
V0 = -3.0
CUT = 4.0
# sigma/dv with cut = 4 -> H
RATIOS = {0: 0.0, 1: 0.25, 7: 1.75, 8: 2.0, 9: 2.25, 15: 3.75, 16: 4.0, 17: 4.25, 31: 7.75, 32: 8.0, 33: 8.25, 70: 17.5, 255: 63.75, 256: 64.0, "cap": 100.0}


def expected_half(ratio, cut=CUT):
    return 0 if not ratio > 0 else int(min(np.ceil(cut * ratio), CAP))


def window_cases():
    """(inv_dv, cut, snr_min, sigmas, pairs) for the host program: every edge of H with dv = 1/8 and cut = 4, other cuts,
    values that are no width at all, and (B, noise) pairs around the detection threshold."""
    nan, inf = float("nan"), float("inf")
    edge = [r * DV for r in RATIOS.values()] + [np.nextafter(2.0 * DV, 0.0), np.nextafter(2.0 * DV, 1.0), np.nextafter(64.0 * DV, 1.0)]
    odd = [0.0, -0.0, -1.0, nan, -inf, inf, 5e-324, 1e-310, 1e-300, 1e300, 0.3, 0.7, 1.1, 2.9, 13.37]
    pairs = [(1.0, 1.0), (np.nextafter(1.0, 2.0), 1.0), (0.0, 0.0), (5e-324, 0.0), (-1.0, 0.0), (nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, inf),
             (2.0, 1.0), (3.0, 1.5), (np.nextafter(3.0, 4.0), 1.5), (1e-30, 1e-31), (1.0, -1.0), (0.0, -0.0)]
    return [(1.0 / DV, CUT, 1.0, edge + odd, pairs),
            (1.0 / DV, 1.0, 2.0, edge + odd, pairs),
            (1.0 / 0.05, 2.5, 0.0, odd + [0.01, 0.05, 0.5, 5.0], pairs),
            (3.0, 300.0, 1.0, [0.1, 1.0, 5e-324, inf], pairs),              # t beyond 700: weights that are exact zeros
            (1.0 / DV, 1e-3, 0.5, edge + odd, pairs)]


def spectrum(ncol, nv, nz, seed, floor=1e-4):
    """A strictly positive spectrum [ncol, nv, nz] in m6 m-3 per bin: per column and level one or two Gaussian peaks of
    random place, width and height on a floor of `floor` times the largest peak, so that no bin is an exact zero."""
    rng = np.random.Generator(np.random.PCG64(seed))
    j = np.arange(nv, dtype=np.float64)[None, :, None]
    x = np.zeros((ncol, nv, nz))
    for _ in range(2):
        mu = rng.uniform(-0.1, 1.1, (ncol, 1, nz)) * nv
        wd = rng.uniform(0.4, 0.15 * nv + 0.5, (ncol, 1, nz))
        amp = 10.0 ** rng.uniform(-16.0, -12.0, (ncol, 1, nz))
        x += amp * np.exp(-0.5 * ((j - mu) / wd) ** 2)
    x += floor * 1e-12 * rng.uniform(0.5, 1.5, (ncol, nv, nz))
    return np.ascontiguousarray(x)


def sigma_profile(nz, halves, ncol=None, seed=0):
    """sigma [nz] (or [ncol, nz]) in m/s whose levels take the half-widths `halves` (keys of RATIOS) in turn."""
    r = np.array([RATIOS[h] for h in halves], dtype=np.float64)
    if ncol is None:
        return DV * r[np.arange(nz) % len(r)]
    rng = np.random.Generator(np.random.PCG64(seed))
    return DV * r[rng.integers(0, len(r), (ncol, nz))]


def inside_spectrum(ncol, nv, nz, lo, hi, seed):
    """A spectrum that is exactly zero outside bins [lo, hi] and positive inside."""
    x = spectrum(ncol, nv, nz, seed)
    x[:, :lo, :] = 0.0
    x[:, hi + 1:, :] = 0.0
    return x
