"""Hand-built states and configurations of the cloud-radar tests (tests/test_gpu_mie_radar.py,
tests/test_fortran_mie_gpu.py), fixed here for both files."""
import numpy as np

import bright_band_cases as bc
import lidar_cases as lc
import mie_radar_ref as ref

# illustrative permittivities of water and ice near 94 and 35 GHz at about 10 C; not taken from a table of record
CFGS = {"w": dict(wavelength=3.19e-3, eps_w=complex(7.7, 14.2), eps_i=complex(3.17, 0.01), rho_w=1000.0, rho_i=917.0, kw2=0.75),
        "ka": dict(wavelength=8.6e-3, eps_w=complex(21.5, 30.5), eps_i=complex(3.17, 0.004), rho_w=1000.0, rho_i=917.0, kw2=0.88)}


def state(nz, seed=7):
    """(st, dz, w, k_gas): seven columns [7, nz] -- five kinds of tests/bright_band_cases.py (mixed-phase with a melting
    level, warm rain, cold snow and graupel without rain, every level below the top rainy and snowy and with graupel, snow
    alone at the melting level) with cloud water added to the first, a dry column, and one column with every species at
    every level."""
    rng = np.random.Generator(np.random.PCG64(seed + nz))
    five, _ = bc.batch(nz, 5, seed + nz, kinds=(0, 7, 5, 6, 3))
    st = {k: np.zeros((7, nz)) for k in ref.INPUTS}
    for k in bc.INPUTS:
        st[k][:5] = five[k]
        st[k][5:] = five[k][0]
    on = rng.uniform(size=nz) < 0.5
    st["qc"][0] = np.where(on, 3.0e-4 * rng.uniform(0.2, 2.0, nz), 0.0)
    for k in ("qc", "qr", "nr", "qs", "qg"):
        st[k][5] = 0.0                                                            # the dry column
    st["t"][6] = np.linspace(275.0, 262.0, nz)                                    # every species at every level
    st["qc"][6] = 2.0e-4 * rng.uniform(0.5, 1.5, nz)
    st["qr"][6] = 8.0e-4 * rng.uniform(0.5, 1.5, nz)
    st["nr"][6] = 2.0e4 * rng.uniform(0.5, 2.0, nz)
    st["qs"][6] = 6.0e-4 * rng.uniform(0.5, 1.5, nz)
    st["qg"][6] = 4.0e-4 * rng.uniform(0.5, 1.5, nz)
    dz = lc.uneven_dz(nz, seed=seed + nz, lo=30.0, hi=300.0)
    w = rng.uniform(-3.0, 3.0, (7, nz))
    k_gas = 1.0e-5 * rng.uniform(0.5, 5.0, nz)
    return st, dz, w, k_gas
