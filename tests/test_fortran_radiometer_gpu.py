"""The radiometer through the Fortran drop-in (-m gpu): tests/fortran/kid_radiometer_driver.f90 -> module_mp_thompson09n's
radiometer_batch -> kidmp_radiometer_table_create and kidmp_radiometer_host (8-byte default REAL) / kidmp32_radiometer_host
(4-byte).  Everything is an equality of bits against the Python host entry on the same arrays."""
import os
import subprocess

import numpy as np
import pytest

import radiometer_cases as rc
import radiometer_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = ref.NAMES[:6]


def _exe(build):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_radiometer_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


def _batch(build, cfg, rcfg, st, dz, k_gas, t_sfc, tmp_path, *mode):
    ncol, nz = st["t"].shape
    f = tmp_path / "state.txt"
    with open(f, "w") as fh:
        fh.write("%d %d\n" % (nz, ncol))
        ew, ei = complex(cfg.eps_w), complex(cfg.eps_i)
        fh.write(" ".join(repr(float(v)) for v in (cfg.wavelength, ew.real, ew.imag, ei.real, ei.imag, cfg.rho_w, cfg.rho_i)) + "\n")
        fh.write(" ".join(repr(float(rcfg[k])) for k in ("mu", "emissivity", "t_cosmic")) + "\n")
        for k in range(nz):
            fh.write("%r %r\n" % (float(dz[k]), float(k_gas[k])))
        for i in range(ncol):
            fh.write("%r\n" % float(t_sfc[i]))
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(st[n][i, k])) for n in ref.INPUTS) + "\n")
    out = subprocess.run([_exe(build), str(f)] + list(mode), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict({n: np.full((ncol, nz), -7.0) for n in PROFILES}, **{n: np.full(ncol, -7.0) for n in ref.SUMMARY})
    seen = 0
    for line in out.stdout.splitlines():
        p = line.split()
        if p and p[0] == "RAD":
            i, k = int(p[2]) - 1, int(p[3]) - 1
            if p[1] in ref.SUMMARY:
                got[p[1]][i] = float(p[4])
            else:
                got[p[1]][i, k] = float(p[4])
            seen += 1
    assert seen == 6 * ncol * nz + 3 * ncol
    return got


def _bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


@pytest.mark.parametrize("build", ["build", "build32"])
@pytest.mark.parametrize("nz, name", [(129, "absorbing"), (65, "default")])
def test_fortran_radiometer_batch_equals_the_python_host_entry(gpu_mixed, tmp_path, build, nz, name):
    from kid_amd import MieCfg, RadiometerCfg
    dtype = np.float64 if build == "build" else np.float32
    full, dz, k_gas, t_sfc = rc.state(nz)
    st = {k: np.ascontiguousarray(full[k][2:7].astype(dtype)) for k in ref.INPUTS}
    dz, k_gas, t_sfc = dz.astype(dtype), k_gas.astype(dtype), np.ascontiguousarray(t_sfc[2:7].astype(dtype))
    cfg = MieCfg(**rc.TABLES[name])
    got = _batch(build, cfg, rc.RCFG, st, dz, k_gas, t_sfc, tmp_path)
    with gpu_mixed.radiometer_table(cfg) as t:
        want = gpu_mixed.radiometer_host(t, st, dz, k_gas, t_sfc, RadiometerCfg(**rc.RCFG), want=ref.NAMES)
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n].astype(dtype)), _bits(want[n])), (build, n)
    assert (want["tau_abs"] > 0).all() and (want["tb_toa"] > rc.RCFG["t_cosmic"]).all() and (want["k_bsc"] > 0).any()


def test_fortran_radiometer_batch_warm_without_the_optional_arguments(gpu_warm, tmp_path):
    from kid_amd import MieCfg
    full, dz, k_gas, t_sfc = rc.state(64)
    st = {k: np.ascontiguousarray(full[k][:4]) for k in ref.INPUTS}
    cfg = MieCfg(**dict(rc.TABLES["absorbing"], rho_w=1000.0, rho_i=900.0))   # what the shim leaves at the library's defaults
    got = _batch("build", cfg, rc.RCFG, st, dz, k_gas, t_sfc[:4], tmp_path, "warm")
    with gpu_warm.radiometer_table(cfg) as t:
        want = gpu_warm.radiometer_host(t, {k: st[k] for k in ("t", "p", "qv", "qr", "nr")}, dz, want=ref.NAMES)
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n]), _bits(want[n])), n
