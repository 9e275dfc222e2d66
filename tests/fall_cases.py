"""Inputs shared by tests/test_fall_speeds_abi.py and tests/test_gpu_fall_speeds.py.  Everything is generated here; nothing
is stored."""
import numpy as np

import cases
import effrad_cases as ec

KEYS = ("t", "p", "qv", "qr", "nr", "qi", "ni", "qs", "qg")
NSTEP_SEEDS = (1301, 1302, 1303)                      # the states of the nstep tests, fixed here for both files
NSTEP_NCOL, NSTEP_NZ, NSTEP_DT = 64, 120, 10.0


def only(st):
    return {k: np.ascontiguousarray(st[k]) for k in KEYS}


def scan_state(nz, ncol, seed):
    """Each species present at each level with probability 1/2 (inheritance across lane, row and chunk boundaries).  The
    last three columns: every species only at the top level; rain only at level 0; none at all."""
    rng = np.random.Generator(np.random.PCG64(seed))
    z = np.linspace(0.0, 12000.0, nz)[None, :]
    t = 290.0 - 6.0e-3 * z + rng.uniform(-3, 3, (ncol, 1))             # T_0 is crossed inside the column
    p = 1.0e5 * np.exp(-z / 8000.0) * np.ones((ncol, 1))
    qv = 0.014 * np.exp(-z / 2500.0) * rng.uniform(0.5, 1.2, (ncol, nz))

    def species(lo, hi):
        q = np.exp(rng.uniform(np.log(lo), np.log(hi), (ncol, nz)))
        return np.where(rng.uniform(size=(ncol, nz)) < 0.5, q, 0.0)
    st = dict(t=t, p=p, qv=qv, qr=species(1e-9, 8e-3), nr=np.exp(rng.uniform(np.log(1.0), np.log(1e6), (ncol, nz))),
              qi=species(1e-10, 1e-3), ni=np.exp(rng.uniform(np.log(1e-2), np.log(1e8), (ncol, nz))),
              qs=species(1e-7, 4e-3), qg=species(1e-7, 1.2e-2))
    st = {k: np.ascontiguousarray(v) for k, v in st.items()}
    assert ncol >= 4
    q = ("qr", "qi", "qs", "qg")
    for k in q:
        st[k][-3:] = 0.0                                                 # -1: none
        st[k][-3, nz - 1] = 5.0e-4                                       # -3: every species only at the top level
    st["qr"][-2, 0] = 1.0e-3                                             # -2: rain only at level 0
    return st


def nstep_state(seed):
    """Random mixed-phase columns with config 5's stretched dz (a shared profile: every column of config 5 has the same)."""
    st = only(ec.random_state(NSTEP_NZ, NSTEP_NCOL, seed))
    dz = np.ascontiguousarray(cases.config5(2)["dz"][0])
    return st, dz
