"""column_summary_batch through the Fortran drop-in (-m gpu): tests/fortran/kid_summary_driver.f90 -> module_mp_thompson09n ->
kidmp_column_summary_host (8-byte default REAL) / kidmp32_column_summary_host (4-byte), against the numpy reference of
tests/column_summary_ref.py on the oracles' profiles.

Bounds: those of test_gpu_column_summary.py.  They are the same for the 4-byte build, whose inputs are rounded to binary32
before either side sees them: the entry widens them on load and its output is binary64."""
import os
import subprocess

import numpy as np
import pytest

import column_summary_ref as ref
import effrad_cases as ec
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


def _state(nz, ncol, seed, build, warm=False):
    st = ec.random_state(nz, ncol, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    st["dz"] = np.exp(rng.uniform(np.log(10.0), np.log(400.0), nz))
    if warm:
        for k in ("qi", "ni", "qs", "qg"):
            st[k][:] = 0.0
    if build == "build32":
        st = {k: v.astype(np.float32).astype(np.float64) for k, v in st.items()}      # what a REAL*4 KiD holds
    return st


def _run(build, st, tmp_path, *mode):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_summary_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    ncol, nz = st["t"].shape
    f = tmp_path / "state.txt"
    with open(f, "w") as fh:
        fh.write("%d %d\n" % (nz, ncol))
        fh.write("".join("%r\n" % float(v) for v in st["dz"]))
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(st[n][i, k])) for n in ref.INPUTS) + "\n")
    out = subprocess.run([exe, str(f)] + [str(a) for a in mode], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.full((ncol, 16), -7.0)
    seen = 0
    for line in out.stdout.splitlines():
        if line.startswith("SUM"):
            p = line.split()
            got[int(p[1]) - 1, int(p[2])] = float(p[3])
            seen += 1
    assert seen == 16 * ncol
    return got


def _check(got, st, consts, oracle, what, cfg=ref.DEFAULT_CFG):
    nz = st["t"].shape[1]
    dbz = ref.oracle_dbz(consts, st)
    re, formed = ref.oracle_re_qc(oracle, st)
    want, mag, _ = ref.summary(st, st["dz"], dbz, re, formed, cfg)
    skip = ref.undecidable(dbz, cfg[0])
    assert not skip.any()
    worst = ref.check(got, want, mag, nz, extra_tau=ref.BOUND_RE, db_bound=ref.BOUND_DB)
    print("Fortran column_summary_batch %s: worst error %.3g of its bound, max |ddBZ| = %.3g"
          % (what, worst, np.max(np.abs(got[:, [7, 10]] - want[:, [7, 10]]))))
    return want


@pytest.mark.parametrize("build", ["build", "build32"])
@pytest.mark.parametrize("nz,ncol", [(120, 5), (65, 1)])
def test_fortran_column_summary_batch(oracle_mixed, consts, tmp_path, build, nz, ncol):
    st = _state(nz, ncol, 70 + nz, build)
    want = _check(_run(build, st, tmp_path), st, consts, oracle_mixed, "%s nz=%d" % (build, nz))
    assert np.isfinite(want[:, ref.Z_FREEZE]).all() and (want[:, ref.TAU_C] > 0).all() and (want[:, ref.IWP] > 0).all()


def test_fortran_column_summary_batch_thresholds(oracle_mixed, consts, tmp_path):
    st = _state(120, 5, 190, "build")
    cfg = (5.0, 3.0e-4, 260.0)
    _check(_run("build", st, tmp_path, "cfg", *cfg), st, consts, oracle_mixed, "thresholds", cfg)


def test_fortran_column_summary_batch_warm_without_the_optional_arguments(oracle_warm, consts, tmp_path):
    st = _state(120, 5, 191, "build", warm=True)
    got = _run("build", st, tmp_path, "warm")
    _check(got, st, consts, oracle_warm, "warm")
    assert np.array_equal(got[:, 3:6].view(np.uint64), np.zeros((5, 3), dtype=np.uint64))       # +0.0
