"""Inputs of the ULTIMATE tests, shared by tests/test_kid_ultimate_abi.py (which asserts on the reference's masks that
they reach every branch of the limiter) and tests/test_gpu_kid_ultimate.py (which holds the kernels to the reference on
them).  The fields and the flow are generated as in tests/test_gpu_kid_advect.py and tests/test_gpu_kid_slab.py: values
over many decades with about a third exact zeros, w of both signs with a sign change inside each column; then interior
faces with w = +0.0, w = -0.0, a Courant number of exactly 1 and one of 1.5 are planted.  No test lives here."""
import numpy as np

import kid_advect_ref as ref

f32, f64 = np.float32, np.float64
DT, DX = 4.0, 150.0
PLANTS = ("c>1", "+0", "-0", "c=1")


def fields(rng, ncol, nz):
    """All nine members: values over many decades, about a third of the cells exactly zero (theta never)."""
    st = {}
    for k in ref.FIELDS:
        hi = 7.0 if k in ("nr", "ni") else -2.0
        st[k] = 10.0 ** rng.uniform(hi - 9.0, hi, (ncol, nz)) * (rng.random((ncol, nz)) < 0.65)
    st["theta"] = 290.0 + 40.0 * np.linspace(0.0, 1.0, nz)[None, :] ** 2 + rng.normal(0.0, 0.5, (ncol, nz))
    return {k: np.ascontiguousarray(v) for k, v in st.items()}


def profiles(rng, nz):
    return (np.ascontiguousarray(1.2 * np.exp(-np.linspace(0.0, 1.1, nz)) * rng.uniform(0.97, 1.03, nz)),
            np.ascontiguousarray(rng.uniform(20.0, 60.0, nz)))


def w_faces(rng, ncol, nz):
    """[ncol, nz+1], both signs and a sign change inside every column (nz = 2: between the one interior face and the top)."""
    f = np.linspace(0.0, 1.0, nz + 1)[None, :]
    w = rng.uniform(0.5, 3.0, (ncol, 1)) * np.sin(2.0 * np.pi * rng.integers(1, 3, (ncol, 1)) * f + rng.uniform(0.1, 3.0, (ncol, 1)))
    w += rng.normal(0.0, 0.2, w.shape)
    w[:, 0] = 0.0
    flip = nz // 2 + 1
    w[:, flip] = -np.abs(w[:, flip]) - 0.1
    w[:, flip - 1] = np.abs(w[:, flip - 1]) + 0.1
    return np.ascontiguousarray(w)


def planted_faces(nz, col):
    """{face: plant} of column `col`.  From nz = 8 on every column holds all four, away from the sign change at faces
    nz/2 and nz/2 + 1; below that the columns from the third on hold one each at face 1, in turn."""
    if nz >= 8:
        return {2: "c>1", nz - 1: "+0", nz - 2: "-0", 3: "c=1"}
    return {1: PLANTS[(col - 2) % 4]} if col >= 2 else {}


def plant(w, dz, dt, dtype):
    """Plants the faces of planted_faces into w (binary64, modified in place) so that they are what they claim in `dtype`:
    the sign of a planted face alternates with every second column, c = (|w|*dt)/dz[u] is exactly 1 where it says so (0.25
    and dt = 4 are powers of two: both products are exact in either format) and 1.5 up to rounding otherwise."""
    ncol, nz = w.shape[0], w.shape[1] - 1
    dzr = dz.astype(dtype).astype(f64)
    for col in range(ncol):
        sign = 1.0 if (col // 2) % 2 == 0 else -1.0
        for face, what in planted_faces(nz, col).items():
            u = face - 1 if sign > 0 else face
            w[col, face] = {"c>1": sign * 0.375 * dzr[u], "c=1": sign * 0.25 * dzr[u], "+0": 0.0, "-0": -0.0}[what]
    assert dt == 4.0
    return w


def case(ncol, nz, seed=0, dtype=f64):
    """(state, w, rho, dz) of `dtype`; a binary32 case is the binary64 one rounded.  Column c of member qv is made monotone
    across the planted c > 1 and c = 1 faces (rising with the level in even columns, falling in odd ones), so that the
    limiter, not the upwind fallback, meets them."""
    rng = np.random.Generator(np.random.PCG64(19000 + 1000 * seed + nz))
    st, w = fields(rng, ncol, nz), w_faces(rng, ncol, nz)
    rho, dz = profiles(rng, nz)
    plant(w, dz, DT, dtype)
    if nz >= 8:
        ramp = 1.0e-3 * np.array([1.0, 2.0, 4.0, 5.0, 9.0, 9.5])             # levels 0 .. 5: faces 2 and 3 see monotone cells
        for col in range(ncol):
            st["qv"][col, :6] = ramp if col % 2 == 0 else ramp[::-1]
    return {k: v.astype(dtype) for k, v in st.items()}, w.astype(dtype), rho.astype(dtype), dz.astype(dtype)


def slab_flow(rng, ncol, nx, nz):
    """u [ncol, nz], w [ncol, nz+1]: random sizes, the signs a chequerboard that changes inside every row (along x) and
    inside every column (along z) for any nx >= 3 and nz >= 2; w = 0 at the ground."""
    i = (np.arange(ncol) % nx)[:, None]
    k, f = np.arange(nz)[None, :], np.arange(nz + 1)[None, :]
    u = rng.uniform(0.2, 3.0, (ncol, nz)) * np.where((i + (k + 1) // 2) % 2 == 0, 1.0, -1.0)
    w = rng.uniform(0.2, 3.0, (ncol, nz + 1)) * np.where((i + f // 2) % 2 == 0, 1.0, -1.0)
    w[:, 0] = 0.0
    return np.ascontiguousarray(u), np.ascontiguousarray(w)


def slab_case(nslab, nx, nz, seed=0, dtype=f64):
    """(state, u, w, rho, dz) of `dtype` with a flow per slab: the chequerboard flow with the planted z faces of `plant`,
    and in x one face per row of levels with u = +0.0, -0.0 or cx = 1.5 (levels 0, 1, 2 mod 4 of cell 1 of every slab)."""
    rng = np.random.Generator(np.random.PCG64(26000 + 1000 * seed + 7 * nx + nz))
    ncol = nslab * nx
    st = fields(rng, ncol, nz)
    u, w = slab_flow(rng, ncol, nx, nz)
    rho, dz = profiles(rng, nz)
    plant(w, dz, DT, dtype)
    k = np.arange(nz)
    for s in range(nslab):
        u[s * nx + 1, k % 4 == 0] = 0.0
        u[s * nx + 1, k % 4 == 1] = -0.0
        u[s * nx + 1, k % 4 == 2] = (1.0 if s % 2 == 0 else -1.0) * 0.375 * DX        # cx = 1.5 exactly (DX = 150, dt = 4)
    return {k: v.astype(dtype) for k, v in st.items()}, u.astype(dtype), w.astype(dtype), rho.astype(dtype), dz.astype(dtype)
