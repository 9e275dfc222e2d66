"""calc_refl10cm through the Fortran drop-in (-m gpu): tests/fortran/kid_refl_driver.f90 -> module_mp_thompson09n ->
kidmp_reflectivity_host (8-byte default REAL) / kidmp32_reflectivity_host (4-byte), against tests/refl_oracle.py."""
import os
import subprocess

import numpy as np
import pytest

import refl_oracle as ro

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = ro.constants(o)
    o.close()
    return c


def _column(nz, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    z = np.linspace(0.0, 14000.0, nz)
    t = 300.0 - 6.5e-3 * z
    p = 1.0e5 * np.exp(-z / 8000.0)
    qv = 0.016 * np.exp(-z / 2500.0)
    def sp(lo, hi):
        q = np.exp(rng.uniform(np.log(lo), np.log(hi), nz))
        return np.where(rng.uniform(size=nz) < 0.6, q, 0.0)
    return dict(t=t, p=p, qv=qv, qr=sp(1e-8, 6e-3), nr=np.exp(rng.uniform(0.0, np.log(1e6), nz)), qs=sp(1e-7, 3e-3),
                qg=sp(1e-7, 1e-2))


def _run(build, col, tmp_path):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_refl_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    nz = col["t"].size
    f = tmp_path / ("col_%s.txt" % build)
    with open(f, "w") as fh:
        fh.write("%d\n" % nz)
        for k in range(nz):
            fh.write(" ".join(repr(float(col[n][k])) for n in ("t", "p", "qv", "qr", "nr", "qs", "qg")) + "\n")
    out = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    d = [float(line.split()[2]) for line in out.stdout.splitlines() if line.startswith("DBZ")]
    assert len(d) == nz
    return np.array(d)


@pytest.mark.parametrize("nz", [120, 65])
def test_fortran_calc_refl10cm_real8(consts, tmp_path, nz):
    col = _column(nz, nz)
    want = ro.calc_refl10cm(consts, col["qv"], col["qr"], col["nr"], col["qs"], col["qg"], col["t"], col["p"])
    got = _run("build", col, tmp_path)
    assert np.max(np.abs(got - want)) <= 3e-13


def test_fortran_calc_refl10cm_real4(consts, tmp_path):
    col = {k: v.astype(np.float32).astype(np.float64) for k, v in _column(120, 3).items()}   # what a REAL*4 KiD holds
    want = ro.calc_refl10cm(consts, col["qv"], col["qr"], col["nr"], col["qs"], col["qg"], col["t"], col["p"])
    got = _run("build32", col, tmp_path)
    # binary64 inside, the result rounded to binary32 once: within half an ulp of binary32 at |dBZ| < 128
    assert np.max(np.abs(got - want)) <= 4e-6


def _exe(build):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_refl_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


@pytest.mark.parametrize("warm", [False, True])
def test_fortran_calc_refl10cm_batch_several_columns(consts, tmp_path, warm):
    """calc_refl10cm_batch on ncol > 1 columns; warm: qs and qg left out of the call (zero)."""
    cols = [_column(120, 40 + i) for i in range(5)]
    if warm:
        for c in cols:
            c["qs"][:] = 0.0
            c["qg"][:] = 0.0
    f = tmp_path / "batch.txt"
    with open(f, "w") as fh:
        fh.write("120 %d\n" % len(cols))
        for c in cols:
            for k in range(120):
                fh.write(" ".join(repr(float(c[n][k])) for n in ("t", "p", "qv", "qr", "nr", "qs", "qg")) + "\n")
    args = [_exe("build"), "batch", str(f)] + (["warm"] if warm else [])
    out = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.zeros((len(cols), 120))
    n = 0
    for line in out.stdout.splitlines():
        if line.startswith("DBZ"):
            _, k, i, v = line.split()
            got[int(i) - 1, int(k) - 1] = float(v)
            n += 1
    assert n == 120 * len(cols)
    st = {k: np.stack([c[k] for c in cols]) for k in cols[0]}
    assert np.max(np.abs(got - ro.of_state(consts, st))) <= 3e-13


def _adapter(build, nx, case, refl, arith, aero, cwd):
    os.makedirs(cwd, exist_ok=True)
    out = subprocess.run([_exe(build), "adapter", str(nx), case, str(refl), arith, str(aero)], capture_output=True,
                         text=True, timeout=600, cwd=str(cwd))
    assert out.returncode == 0, out.stdout + out.stderr
    log = []
    for line in open(os.path.join(str(cwd), "dg_dump.txt")):
        p = line.split()
        log.append(dict(form=p[0], name=p[1], k=int(p[2]), i=int(p[3]), v=float(p[4]), units=" ".join(p[5:-1]), dim=p[-1]))
    state_text = open(os.path.join(str(cwd), "post_state.txt")).read()
    post = np.loadtxt(os.path.join(str(cwd), "post_state.txt")).reshape(nx, 120, 16)
    return log, state_text, post


# (build, arithmetic, case, is_aerosol_aware): both default REAL kinds (build: kidmp_batch_step_host_out; build32 with
# 'p32n': kidmp32_batch_step_host_out), the warm and the mixed-phase call forms of the adapter, and its aerosol-aware form
ADAPTER_RUNS = [("build", "p64", "warm", 0), ("build", "p64", "mixed", 0), ("build", "p64", "warm", 1),
                ("build32", "p32n", "warm", 0), ("build32", "p32n", "mixed", 0)]


@pytest.mark.parametrize("build,arith,case,aero", ADAPTER_RUNS)
def test_adapter_radar_reflectivity_switch(consts, tmp_path, build, arith, case, aero):
    nx = 3
    log_off, state_off, _ = _adapter(build, nx, case, 0, arith, aero, tmp_path / "off")
    log_on, state_on, post = _adapter(build, nx, case, 1, arith, aero, tmp_path / "on")
    # off: no dBZ entry.  on: the same calls, then dBZ last (after the precipitation diagnostics), nothing else changed
    assert not any(e["name"] == "dBZ" for e in log_off)
    n = 120 * nx
    assert log_on[:-n] == log_off
    dbz_log = log_on[-n:]
    assert all(e["name"] == "dBZ" and e["form"] == "2d" and e["units"] == "dBZ" and e["dim"] == "z,x" for e in dbz_log)
    assert [(e["k"], e["i"]) for e in dbz_log] == [(k, i) for i in range(1, nx + 1) for k in range(1, 121)]   # (nz, nx)
    assert state_on == state_off                 # post-step state and d*_mphys unchanged by the switch
    got = np.array([e["v"] for e in dbz_log]).reshape(nx, 120)
    st = {k: post[:, :, j] for j, k in enumerate(("t", "p", "qv", "qr", "nr", "qs", "qg"))}
    want = ro.of_state(consts, st)
    # REAL 8: the binary64 kernel; REAL 4: binary32 state in, binary64 inside, the result rounded to binary32 once
    tol = 3e-13 if build == "build" else 4e-6
    assert np.max(np.abs(got - want)) <= tol
    if case == "mixed":
        assert (post[:, :, 6] > 1e-6).any() and (post[:, :, 5] > 1e-6).any()    # graupel and snow took part
