"""The Doppler spectrum through the Fortran drop-in (-m gpu): tests/fortran/kid_dspectrum_driver.f90 ->
module_mp_thompson09n's doppler_spectrum_batch -> kidmp_doppler_spectrum_host (8-byte default REAL) /
kidmp32_doppler_spectrum_host (4-byte).  Everything is an equality of bits against the Python host entry on the same
arrays."""
import os
import subprocess

import numpy as np
import pytest

import doppler_spectrum_ref as ref
import effrad_cases as ec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = ("below", "above")


def _exe(build):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_dspectrum_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


def _batch(build, st, w, v0, dv, nv, grid_s, tmp_path, *mode):
    ncol, nz = st["t"].shape
    f = tmp_path / "state.txt"
    with open(f, "w") as fh:
        nbs = 0 if grid_s is None else len(grid_s[0])
        fh.write("%d %d %d %r %r %d\n" % (nz, ncol, nv, float(v0), float(dv), nbs))
        for b in range(nbs):
            fh.write("%r %r\n" % (float(grid_s[0][b]), float(grid_s[1][b])))
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(st[n][i, k])) for n in ref.INPUTS) + " %r\n" % float(w[i, k]))
    out = subprocess.run([_exe(build), str(f)] + list(mode), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {n: np.full((ncol, nz) if n in PROFILES else (ncol, nv, nz), -7.0) for n in ref.NAMES}
    seen = 0
    for line in out.stdout.splitlines():
        p = line.split()
        if p and p[0] == "DSPEC":
            i, k, j = int(p[2]) - 1, int(p[3]) - 1, int(p[4]) - 1
            if p[1] in PROFILES:
                got[p[1]][i, k] = float(p[5])
            else:
                got[p[1]][i, j, k] = float(p[5])
            seen += 1
    assert seen == (4 * nv + 2) * ncol * nz
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("build", ["build", "build32"])
@pytest.mark.parametrize("nz,ncol,nv,nbs", [(120, 3, 24, 0), (65, 2, 33, 37)])
def test_fortran_doppler_spectrum_batch_equals_the_python_host_entry(gpu_mixed, tmp_path, build, nz, ncol, nv, nbs):
    dtype = np.float64 if build == "build" else np.float32
    full = ec.random_state(nz, ncol, 280 + nz)
    st = {k: np.ascontiguousarray(full[k].astype(dtype)) for k in ref.INPUTS}
    rng = np.random.Generator(np.random.PCG64(281 + nz))
    w = np.ascontiguousarray(rng.uniform(-6.0, 6.0, (ncol, nz)).astype(dtype))
    grid_s = None
    if nbs:
        edges = np.geomspace(1e-4, 3e-2, nbs + 1)
        grid_s = (np.ascontiguousarray(np.sqrt(edges[:-1] * edges[1:])), np.ascontiguousarray(edges[1:] - edges[:-1]))
    v0, dv = -2.5, 14.0 / nv
    got = _batch(build, st, w, v0, dv, nv, grid_s, tmp_path)
    want = gpu_mixed.doppler_spectrum_host(st, v0, dv, nv, w, None if grid_s is None else {"s": grid_s}, ref.NAMES)
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n].astype(dtype)), _bits(want[n])), (build, n)
    assert all((want[n] > 0).any() for n in ref.NAMES)


def test_fortran_doppler_spectrum_batch_warm_without_the_optional_arguments(gpu_warm, tmp_path):
    full = ec.random_state(120, 2, 291)
    st = {k: np.ascontiguousarray(full[k]) for k in ref.INPUTS}
    got = _batch("build", st, np.ones((2, 120)), 0.0, 0.5, 24, None, tmp_path, "warm")
    want = gpu_warm.doppler_spectrum_host({k: st[k] for k in ("t", "p", "qv", "qr", "nr")}, 0.0, 0.5, 24, want=ref.NAMES)
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n]), _bits(want[n])), n
    assert not _bits(got["snow"]).any() and not _bits(got["graupel"]).any() and (got["rain"] > 0).any()     # +0.0
    assert np.array_equal(_bits(got["rain"]), _bits(got["total"]))
