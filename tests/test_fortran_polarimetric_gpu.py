"""The polarimetric radar through the Fortran drop-in (-m gpu): tests/fortran/kid_polarimetric_driver.f90 ->
module_mp_thompson09n's polarimetric_batch -> kidmp_pol_table_create and kidmp_polarimetric_host (8-byte default REAL) /
kidmp32_polarimetric_host (4-byte).  Everything is an equality of bits against the Python host entry on the same arrays."""
import math
import os
import subprocess

import numpy as np
import pytest

import polarimetric_ref as ref
from mie_radar_cases import state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a configuration that differs from the defaults in every member: illustrative values, not taken from a table of record
MIE = dict(wavelength=0.055, eps_w=complex(72.0, 35.0), eps_i=complex(3.17, 0.003), rho_w=998.0, rho_i=917.0)
POL = dict(axis_r=(1.0, 0.01, -0.03, 0.004, -0.0002), axis_r_min=0.4, axis_s=0.6, axis_g=0.9, sigma=(0.1, 0.5, math.radians(30.0)))


def _exe(build):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_polarimetric_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


def _batch(build, mie, pol, quad, st, tmp_path, *mode):
    ncol, nz = st["t"].shape
    f = tmp_path / "state.txt"
    with open(f, "w") as fh:
        fh.write("%d %d\n" % (nz, ncol))
        ew, ei = complex(mie["eps_w"]), complex(mie["eps_i"])
        fh.write(" ".join(repr(float(v)) for v in (mie["wavelength"], ew.real, ew.imag, ei.real, ei.imag, mie["rho_w"], mie["rho_i"])) + "\n")
        fh.write(" ".join(repr(float(v)) for v in tuple(pol["axis_r"]) + (pol["axis_r_min"], pol["axis_s"], pol["axis_g"]) + tuple(pol["sigma"]))
                 + " %d\n" % (1 if quad else 0))
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(st[n][i, k])) for n in ref.INPUTS) + "\n")
    out = subprocess.run([_exe(build), str(f)] + list(mode), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {n: np.full((ncol, nz), -7.0) for n in ref.NAMES}
    seen = 0
    for line in out.stdout.splitlines():
        p = line.split()
        if p and p[0] == "POL":
            got[p[1]][int(p[2]) - 1, int(p[3]) - 1] = float(p[4])
            seen += 1
    assert seen == 13 * ncol * nz
    return got


def _bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


@pytest.mark.parametrize("build, quad", [("build", False), ("build32", False), ("build", True)])
def test_fortran_polarimetric_batch_equals_the_python_host_entry(gpu_mixed, tmp_path, build, quad):
    from kid_amd import MieCfg, PolCfg
    dtype = np.float64 if build == "build" else np.float32
    full = state(120)[0]
    st = {k: np.ascontiguousarray(full[k][2:7].astype(dtype)) for k in ref.INPUTS}
    got = _batch(build, MIE, POL, quad, st, tmp_path)
    with gpu_mixed.pol_table(MieCfg(**MIE), PolCfg(force_quadrature=quad, **POL)) as t:
        assert t.get("g")[3] == (not quad)
        want = gpu_mixed.polarimetric_host(t, st, want=ref.NAMES)
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n].astype(dtype)), _bits(want[n])), (build, n)
    assert (want["zdr_r"] > 0.1).any() and (want["kdp"] > 0).any() and (want["rhohv"] < 1.0).any()


def test_fortran_polarimetric_batch_warm_without_the_optional_arguments(gpu_warm, tmp_path):
    full = state(64)[0]
    st = {k: np.ascontiguousarray(full[k][:4]) for k in ref.INPUTS}
    got = _batch("build", MIE, POL, False, st, tmp_path, "warm")            # the file's configuration is not passed on
    with gpu_warm.pol_table() as t:
        want = gpu_warm.polarimetric_host(t, {k: st[k] for k in ("t", "p", "qv", "qr", "nr")}, want=ref.NAMES)
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n]), _bits(want[n])), n
    assert (_bits(got["kdp_s"]) == 0).all() and (_bits(got["zdr_g"]) == 0).all()
