"""Hand-built states and configurations of the radiometer tests (tests/test_gpu_radiometer.py,
tests/test_fortran_radiometer_gpu.py, tests/test_radiometer_abi.py), fixed here for all of them.  Built on the seeded
mixed-phase columns of tests/mie_radar_cases.py."""
import numpy as np

import mie_radar_cases as mc
import radiometer_ref as ref

# the two tables: an absorbing one (the illustrative W-band permittivities of tests/test_mie_abi.py) that is run with a gas
# profile, and the default configuration (10 cm, Im(eps_i) = 0: snow and graupel scatter and do not absorb) run without
TABLES = {"absorbing": dict(mc.CFGS["w"]), "default": {}}
USES_GAS = {"absorbing": True, "default": False}
# the streams, the surface and the sky of the parity tests: nothing at its default but the cosmic background
RCFG = dict(mu=0.6, emissivity=0.85, t_cosmic=2.725)
NZS = (2, 33, 64, 65, 128, 129, 200, 256)
KINDS = ("clear", "snow", "rain", "cloud", "graupel")


def _pattern(st, c, start):
    """Column c: level k holds KINDS[(k + start) % 5] alone."""
    nz = st["t"].shape[1]
    for k in ("qc", "qr", "nr", "qs", "qg"):
        st[k][c] = 0.0
    kind = (np.arange(nz) + start) % 5
    st["t"][c] = np.where(kind == 1, 255.0, np.where(kind == 4, 260.0, 285.0))
    st["qs"][c] = np.where(kind == 1, 5.0e-4, 0.0)
    st["qr"][c] = np.where(kind == 2, 6.0e-4, 0.0)
    st["nr"][c] = np.where(kind == 2, 1.5e4, 0.0)
    st["qc"][c] = np.where(kind == 3, 3.0e-4, 0.0)
    st["qg"][c] = np.where(kind == 4, 5.0e-4, 0.0)


def state(nz, seed=7):
    """(st, dz, k_gas, t_sfc): seven columns [7, nz] -- five of tests/mie_radar_cases.py (mixed-phase with cloud water, warm
    rain, cold snow and graupel, every level rainy, snowy and with graupel, every species at every level) and two whose
    levels hold, in turn, nothing, snow alone, rain alone, cloud water alone and graupel alone; the second starts the turn
    at rain, so that two levels already show four kinds."""
    base, dz, _, k_gas = mc.state(nz, seed)
    st = {k: np.ascontiguousarray(v[[0, 1, 2, 3, 6, 5, 5]]) for k, v in base.items()}
    _pattern(st, 5, 0)
    _pattern(st, 6, 2)
    rng = np.random.Generator(np.random.PCG64(seed + 1000 + nz))
    t_sfc = np.ascontiguousarray(st["t"][:, 0] + rng.uniform(-4.0, 6.0, 7))
    return st, dz, k_gas, t_sfc


def branches(ta, b):
    """How many levels take the conservative branch, the non-scattering one and the identity."""
    return int(((ta == 0) & (b > 0)).sum()), int(((b == 0) & (ta > 0)).sum()), int(((ta == 0) & (b == 0)).sum())


def cfg_of(name):
    """The configuration of a table as tests/radiometer_ref.py takes it."""
    from kid_amd import MieCfg
    c = MieCfg(**TABLES[name])
    return ref.cfg_of(c.wavelength, c.eps_w, c.eps_i, c.rho_w, c.rho_i, c.kw2)
