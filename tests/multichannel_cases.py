"""States and configurations of the multi-channel tests (tests/test_gpu_multichannel.py,
tests/test_fortran_multichannel_gpu.py, tests/test_multichannel_abi.py), fixed here for all of them.

The states are those of tests/radiometer_cases.py and tests/mie_radar_cases.py: seven columns.  The sixteen configurations
are illustrative, as the ones they are built from are: the W-band and Ka-band configurations of tests/mie_radar_cases.py,
the library's default (10 cm), and thirteen more on a geometric ladder of wavelengths between 3.19 mm and 10 cm,
    lambda_k = 3.19e-3 * (0.10/3.19e-3)**(k/14),   k = 1..13,
whose eps_w, eps_i and kw2 are interpolated linearly in ln(lambda) between the two of the three anchors that enclose
lambda_k (W and Ka, or Ka and 10 cm).  rho_w is 1000 and rho_i 917 on the ladder; no table of record stands behind any of
it.  Every configuration has the same rho_w, so the rows that do not depend on the wavelength are equal across the set.
"""
import math

import numpy as np

import mie_radar_cases as mc
import radiometer_cases as rc

NCH_MAX = 16
NZS = (2, 65, 129, 256)                                     # one to four level groups


def _default():
    k = math.sqrt(0.176)
    return dict(wavelength=0.10, eps_w=complex(79.5, 24.9), eps_i=complex((1.0 + 2.0 * k) / (1.0 - k), 0.0), rho_w=1000.0, rho_i=900.0, kw2=0.93)


def _between(a, b, lam):
    f = (math.log(lam) - math.log(a["wavelength"])) / (math.log(b["wavelength"]) - math.log(a["wavelength"]))
    mix = lambda k: a[k] + f * (b[k] - a[k])   # noqa: E731
    return dict(wavelength=lam, eps_w=mix("eps_w"), eps_i=mix("eps_i"), rho_w=1000.0, rho_i=917.0, kw2=mix("kw2"))


def configs():
    """The sixteen configurations as keyword dicts of kid_amd.MieCfg: W, Ka, the default, then the ladder ascending."""
    w, ka, d = dict(mc.CFGS["w"]), dict(mc.CFGS["ka"]), _default()
    out = [w, ka, d]
    for k in range(1, 14):
        lam = w["wavelength"] * (d["wavelength"] / w["wavelength"]) ** (k / 14.0)
        out.append(_between(w, ka, lam) if lam < ka["wavelength"] else _between(ka, d, lam))
    assert len(out) == NCH_MAX and len({c["wavelength"] for c in out}) == NCH_MAX
    return out


def rcfgs(nch=NCH_MAX):
    """A closure per channel, all distinct: keyword dicts of kid_amd.RadiometerCfg."""
    return [dict(mu=0.4 + 0.6 * c / 15.0, emissivity=0.5 + 0.03 * c, t_cosmic=2.725 + 0.01 * c) for c in range(nch)]


def k_gas_per_channel(k_gas, nch=NCH_MAX):
    """[nch, nz] from the state's [nz]: every channel its own gas profile."""
    return np.ascontiguousarray(np.stack([k_gas * (1.0 + 0.25 * c) for c in range(nch)]))


def caller_grids():
    """A caller's grid triple with nb = (65, 1, 130): the 64-bin block of the bin loop is crossed once and twice."""
    edges = {"r": (5e-5, 6e-3, 65), "s": (2e-4, 2e-2, 1), "g": (2.5e-4, 4e-2, 130)}
    grids = {}
    for x, (lo, hi, nb) in edges.items():
        e = np.exp(np.linspace(np.log(lo), np.log(hi), nb + 1))
        grids[x] = (np.ascontiguousarray(np.sqrt(e[:-1] * e[1:])), np.ascontiguousarray(e[1:] - e[:-1]))
    return grids


GRIDS = {"scheme": None, "caller": caller_grids()}


def radiometer_state(nz):
    """(st, dz, k_gas [nz], t_sfc) of tests/radiometer_cases.py."""
    return rc.state(nz)


def radar_state(nz):
    """(st, dz, w, k_gas [nz]) of tests/mie_radar_cases.py."""
    return mc.state(nz)


def channel_counts(tile, most=NCH_MAX, beyond=True):
    """The channel counts the tests run at one tile: below it, at it, one past it, past two tiles (beyond) and the most."""
    n = [1, 2, tile, tile + 1] + ([2 * tile + 1] if beyond else []) + [most]
    return sorted({min(v, most) for v in n})
