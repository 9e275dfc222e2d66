"""The size spectra through the Fortran drop-in (-m gpu): tests/fortran/kid_spectra_driver.f90 -> module_mp_thompson09n's
size_spectra_batch -> kidmp_size_spectra_host (8-byte default REAL) / kidmp32_size_spectra_host (4-byte).  Everything is
an equality of bits: size_spectra_batch against the Python host entry on the same arrays."""
import os
import subprocess

import numpy as np
import pytest

import effrad_cases as ec
import size_spectra_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ref.SPECIES + ref.PARAMS


def _exe(build):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_spectra_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


def _run(build, st, grid, tmp_path, *mode):
    """grid: None or (D, dD) for rain.  Returns name -> array, [ncol, nz] or [ncol, nb, nz], as float64."""
    ncol, nz = st["t"].shape
    nb = 0 if grid is None else len(grid[0])
    f = tmp_path / "state.txt"
    with open(f, "w") as fh:
        fh.write("%d %d %d\n" % (nz, ncol, nb))
        for b in range(nb):
            fh.write("%r %r\n" % (float(grid[0][b]), float(grid[1][b])))
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(st[n][i, k])) for n in ref.INPUTS) + "\n")
    out = subprocess.run([_exe(build), str(f)] + list(mode), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {n: np.full((ncol, nz), -7.0) for n in ref.PARAMS}
    got.update({x: np.full((ncol, nb if x == "r" and nb else 100, nz), -7.0) for x in ref.SPECIES})
    for line in out.stdout.splitlines():
        p = line.split()
        if p and p[0] == "PAR":
            got[p[1]][int(p[2]) - 1, int(p[3]) - 1] = float(p[4])
        elif p and p[0] == "BIN":
            got[p[1]][int(p[2]) - 1, int(p[3]) - 1, int(p[4]) - 1] = float(p[5])
    assert all((a != -7.0).all() for a in got.values())
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("build", ["build", "build32"])
@pytest.mark.parametrize("nz,ncol,nb", [(65, 2, 7), (120, 1, 0)])
def test_fortran_size_spectra_batch_equals_the_python_host_entry(gpu_mixed, tmp_path, build, nz, ncol, nb):
    dtype = np.float64 if build == "build" else np.float32
    st = {k: np.ascontiguousarray(ec.random_state(nz, ncol, 60 + nz)[k].astype(dtype)) for k in ref.INPUTS}
    grid = None
    if nb:
        edges = np.exp(np.linspace(np.log(1e-4), np.log(6e-3), nb + 1))
        grid = (np.ascontiguousarray(np.sqrt(edges[:-1] * edges[1:])), np.ascontiguousarray(np.diff(edges)))
    got = _run(build, st, grid, tmp_path)
    want = gpu_mixed.size_spectra_host(st, ALL, None if grid is None else {"r": grid})
    for n in ALL:
        assert got[n].shape == want[n].shape and np.array_equal(_bits(got[n].astype(dtype)), _bits(want[n])), (build, n)
    assert all((want[n] > 0).any() for n in ALL)


def test_fortran_size_spectra_batch_warm_without_the_optional_arguments(gpu_warm, tmp_path):
    st = {k: np.ascontiguousarray(ec.random_state(64, 2, 93)[k]) for k in ref.INPUTS}
    got = _run("build", st, None, tmp_path, "warm")
    want = gpu_warm.size_spectra_host({k: st[k] for k in ("t", "p", "qv", "qc", "qr", "nr")}, ALL)
    for n in ALL:
        assert np.array_equal(_bits(got[n]), _bits(want[n])), n
    assert not any(_bits(got[n]).any() for n in ("i", "s", "g", "lam_i", "smob", "n0_g")) and (got["c"] > 0).any()   # +0.0
