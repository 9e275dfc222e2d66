"""Hand-built columns of the lidar tests (tests/test_lidar_abi.py, tests/test_gpu_lidar.py), fixed here for both files."""
import numpy as np

import column_summary_ref as csr
import lidar_ref as ref
import size_spectra_ref as ssr

K_B = ref.K_B
PI_GAP = abs(np.pi / ssr.PI - 1.0)                     # the scheme's ten-digit PI (M:35) is in am_r, and so in re_qc


def empty(ncol, nz, t=280.0, p=8.0e4, qv=4.0e-3):
    st = {k: np.zeros((ncol, nz)) for k in ref.INPUTS}
    st["t"][:], st["p"][:], st["qv"][:] = t, p, qv
    return st


def uneven_dz(nz, seed=5, lo=20.0, hi=400.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.exp(rng.uniform(np.log(lo), np.log(hi), nz))


def one_species(x, nz=37, seed=11):
    """One column that holds species x alone on most levels, of moderate optical depth (the telescoping identity)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    st = empty(1, nz, t=268.0 if x in "isg" else 284.0)
    on = rng.uniform(size=nz) < 0.8
    q = np.where(on, np.exp(rng.uniform(np.log(1e-5), np.log(1e-3), nz)), 0.0)
    if x == "c":
        st["qc"][0] = q * 0.1
    elif x == "i":
        st["qi"][0], st["ni"][0] = q * 0.1, 1.0e5
    elif x == "r":
        st["qr"][0], st["nr"][0] = q * 3.0, 3.0e4
    elif x == "s":
        st["qs"][0] = q
    else:
        st["qg"][0] = q * 3.0
    return st


def liquid_columns(ncol=8, nz=40, seed=23):
    """Liquid-only columns with qv >= 1e-10 for the comparison with column_summary's TAU_C; the columns 1, 4 and 6 hold a
    level with so little cloud water that calc_effectRad clamps its radius, and are to be found and left out."""
    rng = np.random.Generator(np.random.PCG64(seed))
    st = empty(ncol, nz)
    st["t"][:] = np.linspace(292.0, 274.0, nz)
    st["p"][:] = np.linspace(1.0e5, 6.5e4, nz)
    on = rng.uniform(size=(ncol, nz)) < 0.5
    st["qc"][:] = np.where(on, np.exp(rng.uniform(np.log(2e-5), np.log(2e-3), (ncol, nz))), 0.0)
    for c in (1, 4, 6):
        st["qc"][c, 5 + c] = 3.0e-9
    st["nc"][:] = 1.0e8
    return st, uneven_dz(nz, seed + 1)


def g_column():
    """(st, dz, c_mol): clear air whose ext_mol is 1 m-1 to rounding, and layer depths that run 2*dtau from 1e-300 to 1e3 in
    ascending order; the depth below the last level stays under 350, so that E does not hide g there."""
    x = np.concatenate([np.logspace(-300, -20, 29), np.logspace(-19, -1, 37), [0.3, 0.9999999, 1.0, 1.0000001, 3.0, 10.0, 30.0, 100.0, 300.0, 1000.0]])
    st = empty(1, x.size, t=250.0, p=5.0e4)
    c_mol = 1.0 / ((8.0 * np.pi / 3.0) * (5.0e4 / (K_B * 250.0)))
    return st, 0.5 * x, c_mol


def opaque_column(nz=60):
    """(st, dz): cloud water on every level, about 14 optical depths per level: 2 tau passes 700 near level 24."""
    st = empty(1, nz, t=285.0, p=9.0e4)
    st["qc"][:] = 1.0e-3
    st["nc"][:] = 1.0e8
    return st, np.full(nz, 200.0)


def select_liquid(oracle):
    """(st, dz, columns, terms of TAU_C): liquid_columns() and the columns where calc_effectRad forms an unclamped re_qc on every
    level that holds cloud water (and qv >= 1e-10 everywhere), so that TAU_C and sum ext_c dz state the same number."""
    st, dz = liquid_columns()
    re_qc, formed = csr.oracle_re_qc(oracle, st)
    has = st["qc"] > ssr.R1
    unclamped = (re_qc > 2.51e-6) & (re_qc < 50.0e-6)
    ok = (~has | (formed & unclamped)).all(axis=1) & (st["qv"] >= 1e-10).all(axis=1)
    return st, dz, np.nonzero(ok)[0], csr.terms(st, dz, re_qc, formed)[csr.TAU_C]
