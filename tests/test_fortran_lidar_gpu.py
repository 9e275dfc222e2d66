"""The lidar operator through the Fortran drop-in (-m gpu): tests/fortran/kid_lidar_driver.f90 -> module_mp_thompson09n's
lidar_profiles_batch -> kidmp_lidar_profiles_host (8-byte default REAL) / kidmp32_lidar_profiles_host (4-byte).
Everything is an equality of bits against the Python host entry on the same arrays (a NaN equals a NaN)."""
import os
import subprocess

import numpy as np
import pytest

import effrad_cases as ec
import lidar_cases as lc
import lidar_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_CFG = ref.cfg(s_ratio=(17.0, 29.0, 21.0, 33.0, 27.0), eta=0.5, c_mol=4.0e-32, beta_detect=1.0e-7, trans_lost=0.125)


def _exe(build):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_lidar_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


def _batch(build, st, dz, tmp_path, *mode):
    ncol, nz = st["t"].shape
    f = tmp_path / "state.txt"
    with open(f, "w") as fh:
        fh.write("%d %d\n" % (nz, ncol))
        for k in range(nz):
            fh.write("%r\n" % float(dz[k]))
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(st[n][i, k])) for n in ref.INPUTS) + "\n")
    out = subprocess.run([_exe(build), str(f)] + list(mode), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {n: np.full((ncol, nz), -7.0) for n in ref.NAMES}
    got["summary"] = np.full((ncol, 8), -7.0)
    seen = 0
    for line in out.stdout.splitlines():
        p = line.split()
        if p and p[0] == "LIDAR":
            got[p[1]][int(p[2]) - 1, int(p[3]) - 1] = float(p[4])
            seen += 1
    assert seen == len(ref.NAMES) * ncol * nz + 8 * ncol
    return got


def _equal(a, b):
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)   # noqa: E731
    return a.dtype == b.dtype and a.shape == b.shape and ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all()


@pytest.mark.parametrize("build", ["build", "build32"])
@pytest.mark.parametrize("nz,ncol", [(120, 5), (65, 2)])
def test_fortran_lidar_profiles_batch_equals_the_python_host_entry(gpu_mixed, tmp_path, build, nz, ncol):
    dtype = np.float64 if build == "build" else np.float32
    full = ec.random_state(nz, ncol, 280 + nz)
    st = {k: np.ascontiguousarray(full[k].astype(dtype)) for k in ref.INPUTS}
    dz = np.ascontiguousarray(lc.uneven_dz(nz, 281 + nz, 5.0, 60.0).astype(dtype))
    got = _batch(build, st, dz, tmp_path)
    want = gpu_mixed.lidar_profiles_host(st, dz, DRIVER_CFG, ref.NAMES, True)
    for n in ref.NAMES:
        assert _equal(got[n].astype(dtype), want[n]), (build, n)
    assert _equal(got["summary"], want["summary"]), build
    assert all((want[n] > 0).any() for n in ref.NAMES) and np.isfinite(want["summary"][:, :2]).all()


def test_fortran_lidar_profiles_batch_warm_without_the_optional_arguments(gpu_warm, tmp_path):
    full = ec.random_state(120, 3, 291)
    st = {k: np.ascontiguousarray(full[k]) for k in ref.INPUTS}
    dz = lc.uneven_dz(120, 292, 5.0, 60.0)
    got = _batch("build", st, dz, tmp_path, "warm")
    want = gpu_warm.lidar_profiles_host({k: st[k] for k in ("t", "p", "qv", "qc", "qr", "nr")}, dz, None, ref.NAMES, True)
    for n in ref.NAMES:
        assert _equal(got[n], want[n]), n
    assert _equal(got["summary"], want["summary"])
    for n in ("ext_i", "ext_s", "ext_g"):
        assert not got[n].view(np.uint64).any(), n                                # +0.0
    assert (got["ext_c"] > 0).any() and (got["ext_r"] > 0).any()
