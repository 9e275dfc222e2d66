"""Inputs of the calc_effectRad / column-output tests (tests/test_effrad_cpu.py, tests/test_gpu_column_outputs.py): the
batch of test_effective_radii_match_oracle, hand-built columns that reach the branches that batch leaves out, and random
columns for the nz sweep.  Everything is generated here; nothing is stored."""
import numpy as np

import cases

R_GAS = 287.04
R1, R2 = 1e-12, 1e-6
PRESETS = (2.49e-6, 4.99e-6, 9.99e-6)
NAMES = ("t", "p", "qv", "qc", "nc", "qi", "ni", "qr", "nr", "qs", "qg")      # what the outputs read
RADII_IN = ("t", "p", "qv", "qc", "nc", "qi", "ni", "qs")
T0, P0, QV0 = 260.0, 6.0e4, 1.0e-3                                           # the base sounding of the hand-built columns


def rho_of(t, p=P0, qv=QV0):
    return 0.622 * p / (R_GAS * t * (qv + 0.622))


def ladder(x, n=9):
    """x and its n neighbours in binary64 on either side, ascending."""
    lo, hi = [x], [x]
    for _ in range(n):
        lo.append(np.nextafter(lo[-1], 0.0))
        hi.append(np.nextafter(hi[-1], 1.0))
    return np.array(lo[:0:-1] + [x] + hi[1:])


def batch():
    """config 3 x 48, config 5 x 48 and the edge cases: the batch of test_effective_radii_match_oracle."""
    parts = (cases.config3(48), cases.config5(48), cases.edge_cases())
    return {k: np.ascontiguousarray(np.concatenate([s[k] for s in parts])) for k in NAMES}


def _column(nz, **kw):
    c = {k: np.zeros(nz) for k in NAMES}
    c["t"][:], c["p"][:], c["qv"][:] = T0, P0, QV0
    c["nc"][:] = 1.0e8
    for k, v in kw.items():
        c[k][:] = v
    return c


def hand_built(nz=120):
    """dict name -> one column (dict of [nz] arrays); `stack` makes a batch of them.  What each reaches is
    asserted with the oracle alone in tests/test_effrad_cpu.py."""
    rho = rho_of(T0)
    cols = {}
    cols["qc_sweep"] = _column(nz, qc=np.logspace(-12, -0.5, nz))
    cols["nc_sweep"] = _column(nz, qc=1e-3, nc=np.resize([50., 1e3, 1e7, 1e8, 1e9, 2e10, 1e11], nz))   # aerosol-aware
    cols["qi_sweep"] = _column(nz, qi=np.logspace(-12, -2, nz), ni=1e5)
    cols["ni_sweep"] = _column(nz, qi=1e-5, ni=np.logspace(-8, 12, nz))
    for T in (215.0, 245.0, 268.0, 273.1, 280.0):
        cols["qs_sweep_%g" % T] = _column(nz, t=T, qs=np.logspace(-12, -1, nz))
    for T in (273.0, 273.06, 290.0):
        cols["rs_sweep_%g" % T] = _column(nz, t=T, qs=np.logspace(-9, -4.5, nz) / rho_of(T))
    cols["ladder_qc"] = _column(nz, qc=np.resize(ladder(R1), nz) / rho)
    cols["ladder_qi"] = _column(nz, qi=np.resize(ladder(R1), nz) / rho, ni=1e5)
    cols["ladder_qs"] = _column(nz, qs=np.resize(ladder(R1), nz) / rho)
    cols["ladder_ni"] = _column(nz, qi=1e-6, ni=np.resize(ladder(R2), nz) / rho)
    return cols


def stack(cols):
    cols = list(cols.values()) if isinstance(cols, dict) else list(cols)
    return {k: np.ascontiguousarray(np.stack([c[k] for c in cols])) for k in NAMES}


def random_state(nz, ncol, seed):
    """_random_state of test_gpu_reflectivity.py (rain, snow and graupel switched on and off per level, supercooled rain)
    extended by cloud water, cloud ice and their numbers, switched the same way."""
    rng = np.random.Generator(np.random.PCG64(seed))
    z = np.linspace(0.0, 14000.0, nz)[None, :]
    t = 302.0 - 6.5e-3 * z + rng.uniform(-3, 3, (ncol, 1))
    p = 1.0e5 * np.exp(-z / 8000.0) * np.ones((ncol, 1))
    qv = 0.016 * np.exp(-z / 2500.0) * rng.uniform(0.5, 1.2, (ncol, nz))

    def species(lo, hi, frac):
        q = np.exp(rng.uniform(np.log(lo), np.log(hi), (ncol, nz)))
        return np.where(rng.uniform(size=(ncol, nz)) < frac, q, 0.0)
    qr = species(1e-9, 8e-3, 0.6)
    nr = np.exp(rng.uniform(np.log(1.0), np.log(1e6), (ncol, nz)))
    qs = species(1e-7, 4e-3, 0.5)
    qg = species(1e-7, 1.2e-2, 0.5)
    qc = species(1e-9, 3e-3, 0.5)
    nc = np.exp(rng.uniform(np.log(1e1), np.log(1e11), (ncol, nz)))
    qi = species(1e-10, 1e-3, 0.5)
    ni = species(1e-2, 1e8, 0.8)
    st = dict(t=t, p=p, qv=qv, qc=qc, nc=nc, qi=qi, ni=ni, qr=qr, nr=nr, qs=qs, qg=qg)
    return {k: np.ascontiguousarray(v) for k, v in st.items()}
