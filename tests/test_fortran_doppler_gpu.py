"""The Doppler moments through the Fortran drop-in (-m gpu): tests/fortran/kid_doppler_driver.f90 -> module_mp_thompson09n's
doppler_moments_batch -> kidmp_doppler_moments_host (8-byte default REAL) / kidmp32_doppler_moments_host (4-byte).
Everything is an equality of bits against the Python host entry on the same arrays."""
import os
import subprocess

import numpy as np
import pytest

import doppler_ref as ref
import effrad_cases as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exe(build):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_doppler_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


def _batch(build, st, w, tmp_path, *mode):
    ncol, nz = st["t"].shape
    f = tmp_path / "state.txt"
    with open(f, "w") as fh:
        fh.write("%d %d\n" % (nz, ncol))
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(st[n][i, k])) for n in ref.INPUTS) + " %r\n" % float(w[i, k]))
    out = subprocess.run([_exe(build), str(f)] + list(mode), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {n: np.full((ncol, nz), -7.0) for n in ref.NAMES}
    seen = 0
    for line in out.stdout.splitlines():
        p = line.split()
        if p and p[0] == "DOPPLER":
            got[p[1]][int(p[2]) - 1, int(p[3]) - 1] = float(p[4])
            seen += 1
    assert seen == len(ref.NAMES) * ncol * nz
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("build", ["build", "build32"])
@pytest.mark.parametrize("nz,ncol", [(120, 5), (65, 2)])
def test_fortran_doppler_moments_batch_equals_the_python_host_entry(gpu_mixed, tmp_path, build, nz, ncol):
    dtype = np.float64 if build == "build" else np.float32
    full = ec.random_state(nz, ncol, 180 + nz)
    st = {k: np.ascontiguousarray(full[k].astype(dtype)) for k in ref.INPUTS}
    rng = np.random.Generator(np.random.PCG64(181 + nz))
    w = np.ascontiguousarray(rng.uniform(-5.0, 5.0, (ncol, nz)).astype(dtype))
    got = _batch(build, st, w, tmp_path)
    want = gpu_mixed.doppler_moments_host(st, w)
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n].astype(dtype)), _bits(want[n])), (build, n)
    assert all((want[n] > 0).any() for n in ref.NAMES)


def test_fortran_doppler_moments_batch_warm_without_the_optional_arguments(gpu_warm, tmp_path):
    full = ec.random_state(120, 3, 191)
    st = {k: np.ascontiguousarray(full[k]) for k in ref.INPUTS}
    got = _batch("build", st, np.ones((3, 120)), tmp_path, "warm")
    want = gpu_warm.doppler_moments_host({k: st[k] for k in ("t", "p", "qv", "qr", "nr")})
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n]), _bits(want[n])), n
    assert not _bits(got["vz_s"]).any() and not _bits(got["vz_g"]).any() and (got["vz_r"] > 0).any()     # +0.0
    assert (got["dbz_s"] == -40.0).all() and (got["dbz_g"] == -40.0).all()
