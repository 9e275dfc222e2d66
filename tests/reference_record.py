"""Running the reference Fortran built from source (oracle/_ref/{p64,native}/ref_driver, `make -C oracle ref`) and
reading the fixtures recorded from it (tests/golden/reference_*.npz, written by tests/golden/make_reference_goldens.py).

Only the generator and the `slow` freshness test run the driver; every other test reads the committed fixtures.  The file
formats are those of the header of oracle/ref_driver.f90.
"""
import fcntl
import os
import struct
import subprocess
import tempfile

import numpy as np

from cases import KEYS
from parity import OUT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NRATES = 36
TABLES = ("tcg_racg tmr_racg tcr_gacr tmg_gacr tnr_racg tnr_gacr tcs_racs1 tmr_racs1 tcs_racs2 tmr_racs2 tcr_sacr1 "
          "tms_sacr1 tcr_sacr2 tms_sacr2 tnr_racs1 tnr_racs2 tnr_sacr1 tnr_sacr2 tpi_qcfz tni_qcfz tpi_qrfz tpg_qrfz "
          "tni_qrfz tnr_qrfz tps_iaus tni_iaus tpi_ide t_Efrw t_Efsw tnc_wev").split()
# the constants of kidmp_tables.hip::const_dir that the reference module leaves PUBLIC (the others are PRIVATE there and
# cannot be read without changing its source)
CONSTS = ("t1_qr_qc t1_qr_qi t2_qr_qi t1_qg_qc t1_qs_qc t1_qs_qi t1_qr_ev t2_qr_ev t1_qs_sd t2_qs_sd t1_qg_sd t2_qg_sd "
          "t1_qs_me t2_qs_me t1_qg_me t2_qg_me").split()
DIAG = ("dbz", "re_qc", "re_qi", "re_qs")
TREES = dict(p64=np.float64, native=np.float32)


def tree_dir(tree):
    return os.path.join(ROOT, "oracle", "_ref", tree)


def have_driver(tree):
    return os.path.exists(os.path.join(tree_dir(tree), "ref_driver"))


def _drive(d, payload):
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(payload)
        subprocess.run([os.path.join(d, "ref_driver"), fin, fout], cwd=d, check=True, stdout=subprocess.DEVNULL)
        with open(fout, "rb") as f:
            return f.read()


def _run(tree, payload):
    """One ref_driver process in its tree.  A mixed-phase thompson_init keeps the reference's racg / racs tables in
    run_data/*.data: it creates the file, computes for a minute and a half and only then writes it, while any other
    mixed-phase process that finds the file reads it at once (M:3717-3729, M:3864-3895).  So until one such run has
    finished in a tree (marked by run_data/complete) these runs go one at a time, under a lock that also holds between
    processes, and files a run left unfinished are removed first; afterwards they may run side by side.  A warm-rain
    init touches none of these files (M:773)."""
    d = tree_dir(tree)
    data = os.path.join(d, "run_data")                       # where the reference keeps its racg / racs table files
    os.makedirs(data, exist_ok=True)
    iiwarm = struct.unpack_from("<2i", payload)[1] != 0
    done = os.path.join(data, "complete")
    if iiwarm or os.path.exists(done):
        return _drive(d, payload)
    with open(os.path.join(d, "run_data.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)                     # (released when the file is closed)
        if not os.path.exists(done):
            for f in os.listdir(data):
                os.remove(os.path.join(data, f))
            out = _drive(d, payload)
            open(done, "w").close()
            return out
    return _drive(d, payload)


def _header(tree, mode, iiwarm, dt, set_Nc=100.0, l_sediment=True):
    return struct.pack("<4i2d", mode, int(iiwarm), int(l_sediment), np.dtype(TREES[tree]).itemsize, set_Nc, dt)


def run_step(tree, iiwarm, blocks, dt, set_Nc=100.0, l_sediment=True):
    """blocks: list of (st, aerosol_aware), st a dict of [ncol, nz] arrays with cases.KEYS.  One process, one
    thompson_init.  Returns per block a dict: the 12 OUT profiles [ncol, nz], ppt [ncol, 4], rates [ncol, 36, nz], and
    dbz / re_qc / re_qi / re_qs [ncol, nz] on the stepped state, the same with suffix "_in" on the input state."""
    real = TREES[tree]
    buf = [_header(tree, 1, iiwarm, dt, set_Nc, l_sediment)]
    for st, aero in blocks:
        ncol, nz = st["qv"].shape
        buf.append(struct.pack("<3i", ncol, nz, int(aero)))
        buf.append(np.stack([np.asarray(st[k], dtype=real) for k in KEYS]).tobytes())
    buf.append(struct.pack("<3i", 0, 0, 0))
    raw = np.frombuffer(_run(tree, b"".join(buf)), dtype="<f8")
    out, pos = [], 0

    def take(*shape):
        nonlocal pos
        n = int(np.prod(shape))
        a = raw[pos:pos + n].reshape(shape).copy()
        pos += n
        return a
    for st, _ in blocks:
        ncol, nz = st["qv"].shape
        r = dict(zip(OUT, take(12, ncol, nz)))
        r["ppt"] = take(ncol, 4)
        r["rates"] = take(ncol, NRATES, nz)
        for sfx in ("", "_in"):
            r.update({k + sfx: v for k, v in zip(DIAG, take(4, ncol, nz))})
        out.append(r)
    assert pos == raw.size, (pos, raw.size)
    return out


def run_tables(tree):
    """{name: array indexed like the Fortran, 0-based} for TABLES, and {name: float} for CONSTS, of a mixed-phase init."""
    raw = _run(tree, _header(tree, 2, False, 10.0))
    pos, tabs = 0, {}
    for name in TABLES:
        nd, *dims = struct.unpack_from("<5i", raw, pos)
        pos += 20
        n = int(np.prod(dims))
        tabs[name] = np.frombuffer(raw, dtype="<f8", count=n, offset=pos).reshape(dims[:nd], order="F").copy()
        pos += 8 * n
    consts = dict(zip(CONSTS, np.frombuffer(raw, dtype="<f8", count=len(CONSTS), offset=pos)))
    assert pos + 8 * len(CONSTS) == len(raw)
    return tabs, {k: float(v) for k, v in consts.items()}


def run_adapter(tree, iiwarm, c, dt=None):
    """The reference's mphys_thompson09_interfacen on the inputs `c` (keys of kat_cases.kat_b(); arrays in the flattened
    Fortran order of Oracle.kid_interface; the advective / divergence tendencies default to zero).  Returns dth, dqv
    [nz*nx], dhy [nz*nx*10] and the save_dg log as a list of (form, name, k, i, value)."""
    real = TREES[tree]
    nz, nx = int(c["nz"]), int(c["nx"])
    parts = [_header(tree, 3, iiwarm, c["dt"] if dt is None else dt), struct.pack("<2i2d", nx, nz, c["p0"], c["r_on_cp"])]
    for k, n in (("theta", 1), ("dtheta_adv", 1), ("dtheta_div", 1), ("exner", 1), ("dz", 0), ("qv", 1), ("dqv_adv", 1),
                 ("dqv_div", 1), ("hydro", 10), ("dhydro_adv", 10), ("dhydro_div", 10)):
        a = np.asarray(c[k] if k in c else np.zeros(nz * nx * n), dtype=real).ravel()
        assert a.size == (nz * nx * n if n else nz), (k, a.size)
        parts.append(a.tobytes())
    raw = _run(tree, b"".join(parts))
    m = nz * nx
    f = np.frombuffer(raw, dtype="<f8", count=12 * m)
    dth, dqv, dhy = f[:m].copy(), f[m:2 * m].copy(), f[2 * m:].copy()
    pos = 8 * 12 * m
    (nlog,) = struct.unpack_from("<i", raw, pos)
    pos += 4
    log = []
    for _ in range(nlog):
        form, name, k, i, v = struct.unpack_from("<8s40s2id", raw, pos)
        pos += 64
        log.append((form.decode().strip(), name.decode().strip(), k, i, v))
    assert pos == len(raw)
    return dth, dqv, dhy, log


def load(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}
