"""calc_effectRad through the Fortran drop-in (-m gpu): tests/fortran/kid_effrad_driver.f90 -> module_mp_thompson09n ->
kidmp_effective_radii_host (8-byte default REAL) / kidmp32_effective_radii_host (4-byte), and the adapter's
l_effective_radii switch (kidmp[32]_batch_step_host_out), against Oracle.calc_effectRad and tests/refl_oracle.py.

Bounds: REAL 8 is the binary64 kernel, 1e-12 relative (test_effective_radii_match_oracle); REAL 4 holds the binary64
result rounded to binary32 once, i.e. within 2**-24 relative of it."""
import os
import subprocess

import numpy as np
import pytest

import effrad_cases as ec
import refl_oracle as ro

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND_RE = 1e-12
BOUND_RE32 = 2.0 ** -24 + BOUND_RE
IN = ec.RADII_IN
SENTINELS = (-1.0, -2.0, -3.0)


@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = ro.constants(o)
    o.close()
    return c


def _exe(build):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_effrad_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


def _write(path, st, start):
    ncol, nz = st["t"].shape
    with open(path, "w") as fh:
        fh.write("%d %d\n" % (nz, ncol) if ncol > 1 else "%d\n" % nz)
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(st[n][i, k])) for n in IN) + " " + " ".join(repr(v) for v in start) + "\n")


def _read(stdout, ncol, nz):
    got = np.full((3, ncol, nz), np.nan)
    for line in stdout.splitlines():
        if line.startswith("RE"):
            p = line.split()
            k, i = (int(p[1]), int(p[2])) if ncol > 1 else (int(p[1]), 1)
            got[:, i - 1, k - 1] = [float(v) for v in p[-3:]]
    assert np.all(np.isfinite(got))
    return got


def _rel(got, want):
    return max(float(np.max(np.abs(g - w) / np.abs(w))) for g, w in zip(got, want))


@pytest.mark.parametrize("build,nz", [("build", 120), ("build", 65), ("build32", 120), ("build32", 65)])
def test_fortran_calc_effectrad_one_column(oracle_warm, tmp_path, build, nz):
    """The reference's dummy list, INOUT: started from sentinels, the levels without the species keep them."""
    st = {k: v[3:4] for k, v in ec.random_state(nz, 4, 50 + nz).items()}
    if build == "build32":
        st = {k: v.astype(np.float32).astype(np.float64) for k, v in st.items()}      # what a REAL*4 KiD holds
    f = tmp_path / "col.txt"
    _write(f, st, SENTINELS)
    out = subprocess.run([_exe(build), str(f)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = _read(out.stdout, 1, nz)
    want = oracle_warm.calc_effectRad(st, preset=SENTINELS)
    for g, w, s in zip(got, want, SENTINELS):
        assert np.array_equal(g == s, w == s) and (g == s).any() and (g != s).any()
    worst = _rel(got, want)
    print("Fortran calc_effectRad %s nz=%d: max rel |dre| = %.3e" % (build, nz, worst))
    assert worst <= (BOUND_RE if build == "build" else BOUND_RE32)


@pytest.mark.parametrize("mode", ["full", "nonc", "warm"])
def test_fortran_calc_effectrad_batch(oracle_warm, tmp_path, mode):
    """calc_effectRad_batch on ncol > 1 columns, with every optional array, without nc, and in a warm run without nc, qi,
    ni and qs (the radii of the absent species stay as they came)."""
    st = {k: v for k, v in ec.random_state(120, 5, 60).items()}
    if mode == "warm":
        for k in ("qi", "ni", "qs"):
            st[k][:] = 0.0
    f = tmp_path / "batch.txt"
    _write(f, st, ec.PRESETS)
    out = subprocess.run([_exe("build"), "batch", str(f), mode], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = _read(out.stdout, 5, 120)
    want = oracle_warm.calc_effectRad(st)        # not aerosol-aware: nc is never read
    worst = _rel(got, want)
    print("Fortran calc_effectRad_batch %s: max rel |dre| = %.3e" % (mode, worst))
    assert worst <= BOUND_RE
    if mode == "warm":
        assert np.all(got[1] == ec.PRESETS[1]) and np.all(got[2] == ec.PRESETS[2])


def _adapter(build, nx, case, refl, radii, arith, aero, cwd):
    os.makedirs(cwd, exist_ok=True)
    out = subprocess.run([_exe(build), "adapter", str(nx), case, str(refl), str(radii), arith, str(aero)],
                         capture_output=True, text=True, timeout=600, cwd=str(cwd))
    assert out.returncode == 0, out.stdout + out.stderr
    log = []
    for line in open(os.path.join(str(cwd), "dg_dump.txt")):
        p = line.split()
        log.append(dict(form=p[0], name=p[1], k=int(p[2]), i=int(p[3]), v=float(p[4]), units=" ".join(p[5:-1]), dim=p[-1]))
    state_text = open(os.path.join(str(cwd), "post_state.txt")).read()
    post = np.loadtxt(os.path.join(str(cwd), "post_state.txt")).reshape(nx, 120, 13)
    return log, state_text, post


# (build, arithmetic, case, is_aerosol_aware): both default REAL kinds, the warm, the mixed-phase and the aerosol-aware
# call forms of the adapter
ADAPTER_RUNS = [("build", "p64", "warm", 0), ("build", "p64", "mixed", 0), ("build", "p64", "mixed", 1),
                ("build", "p64", "warm", 1), ("build32", "p32n", "warm", 0), ("build32", "p32n", "mixed", 0)]


@pytest.mark.parametrize("build,arith,case,aero", ADAPTER_RUNS)
def test_adapter_effective_radii_switch(request, consts, tmp_path, build, arith, case, aero):
    nx, nz = 3, 120
    n = nz * nx
    o = request.getfixturevalue("oracle_mixed_aero" if aero else "oracle_warm")
    log_off, state_off, _ = _adapter(build, nx, case, 0, 0, arith, aero, tmp_path / "off")
    log_re, state_re, post = _adapter(build, nx, case, 0, 1, arith, aero, tmp_path / "radii")
    log_both, state_both, _ = _adapter(build, nx, case, 1, 1, arith, aero, tmp_path / "both")
    log_dbz, _, _ = _adapter(build, nx, case, 1, 0, arith, aero, tmp_path / "dbz")
    names = ("re_cloud", "re_ice", "re_snow")
    assert not any(e["name"] in names for e in log_off) and not any(e["name"] in names for e in log_dbz)
    # on: exactly 3 * nz * nx entries after the existing ones, after dBZ if that is on too; nothing else changes
    assert log_re[:-3 * n] == log_off and log_both[:-3 * n] == log_dbz and log_dbz[:-n] == log_off
    assert log_both[-3 * n:] == log_re[-3 * n:]
    assert state_re == state_off and state_both == state_off
    st = {k: post[:, :, j] for j, k in enumerate(("t", "p", "qv", "qc", "nc", "qi", "ni", "qr", "nr", "qs", "qg"))}
    want = o.calc_effectRad({k: np.ascontiguousarray(st[k]) for k in IN})
    worst = 0.0
    for j, name in enumerate(names):
        part = log_re[-3 * n + j * n: -3 * n + (j + 1) * n] if j < 2 else log_re[-n:]
        assert all(e["name"] == name and e["form"] == "2d" and e["units"] == "m" and e["dim"] == "z,x" for e in part)
        assert [(e["k"], e["i"]) for e in part] == [(k, i) for i in range(1, nx + 1) for k in range(1, nz + 1)]
        got = np.array([e["v"] for e in part]).reshape(nx, nz)
        worst = max(worst, float(np.max(np.abs(got - want[j]) / want[j])))
    print("adapter l_effective_radii %s %s %s aero=%d: max rel |dre| = %.3e" % (build, arith, case, aero, worst))
    assert worst <= (BOUND_RE if build == "build" else BOUND_RE32)
    assert (want[0] != ec.PRESETS[0]).any()                                    # cloud water took part
    if case == "mixed":
        assert (want[1] != ec.PRESETS[1]).any() and (want[2] != ec.PRESETS[2]).any()
    dbz = np.array([e["v"] for e in log_both[-4 * n:-3 * n]]).reshape(nx, nz)
    assert all(e["name"] == "dBZ" for e in log_both[-4 * n:-3 * n])
    err = float(np.max(np.abs(dbz - ro.of_state(consts, {k: st[k] for k in ("t", "p", "qv", "qr", "nr", "qs", "qg")}))))
    assert err <= (3e-13 if build == "build" else 4e-6)                        # the bounds of test_fortran_refl_gpu.py
