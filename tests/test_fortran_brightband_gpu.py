"""The bright band through the Fortran drop-in (-m gpu): tests/fortran/kid_brightband_driver.f90 ->
module_mp_thompson09n's bright_band_batch -> kidmp_bright_band_host (8-byte default REAL) / kidmp32_bright_band_host
(4-byte).  Everything is an equality of bits against the Python host entry on the same arrays."""
import os
import subprocess

import numpy as np
import pytest

import bright_band_cases as bc
import bright_band_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exe(build):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_brightband_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


def _batch(build, st, topology, grid_g, tmp_path, *mode):
    ncol, nz = st["t"].shape
    f = tmp_path / "state.txt"
    with open(f, "w") as fh:
        nbg = 0 if grid_g is None else len(grid_g[0])
        fh.write("%d %d %d %d\n" % (nz, ncol, topology, nbg))
        for b in range(nbg):
            fh.write("%r %r\n" % (float(grid_g[0][b]), float(grid_g[1][b])))
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(st[n][i, k])) for n in ref.INPUTS) + "\n")
    out = subprocess.run([_exe(build), str(f)] + list(mode), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict({n: np.full((ncol, nz), -7.0) for n in ref.PROFILES}, k0=np.full(ncol, -7, dtype=np.int32))
    seen = 0
    for line in out.stdout.splitlines():
        p = line.split()
        if p and p[0] == "BBAND":
            i, k = int(p[2]) - 1, int(p[3]) - 1
            if p[1] == "k0":
                got["k0"][i] = int(p[4])
            else:
                got[p[1]][i, k] = float(p[4])
            seen += 1
    assert seen == 7 * ncol * nz + ncol
    return got


def _bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


@pytest.mark.parametrize("build", ["build", "build32"])
@pytest.mark.parametrize("nz,ncol,topology,nbg", [(120, 9, 0, 0), (65, 5, 1, 37)])
def test_fortran_bright_band_batch_equals_the_python_host_entry(gpu_mixed, tmp_path, build, nz, ncol, topology, nbg):
    from kid_amd import BrightBandCfg
    dtype = np.float64 if build == "build" else np.float32
    full, _ = bc.batch(nz, ncol, 300 + nz)
    st = {k: np.ascontiguousarray(full[k].astype(dtype)) for k in ref.INPUTS}
    grid_g = None
    if nbg:
        edges = np.geomspace(2e-4, 4e-2, nbg + 1)
        grid_g = (np.ascontiguousarray(np.sqrt(edges[:-1] * edges[1:])), np.ascontiguousarray(edges[1:] - edges[:-1]))
    got = _batch(build, st, topology, grid_g, tmp_path)
    want = gpu_mixed.bright_band_host(st, BrightBandCfg(topology=topology), None if grid_g is None else {"g": grid_g}, ref.NAMES)
    for n in ref.PROFILES:
        assert np.array_equal(_bits(got[n].astype(dtype)), _bits(want[n])), (build, n)
    assert np.array_equal(got["k0"], want["k0"]) and (want["k0"] >= 0).any()
    assert (want["enh_s"] > 1.0).any() and (want["enh_g"] > 1.0).any()


def test_fortran_bright_band_batch_warm_without_the_optional_arguments(gpu_warm, tmp_path):
    full, _ = bc.batch(120, 4, 311)
    st = {k: np.ascontiguousarray(full[k]) for k in ref.INPUTS}
    got = _batch("build", st, 0, None, tmp_path, "warm")
    want = gpu_warm.bright_band_host({k: st[k] for k in ("t", "p", "qv", "qr", "nr")}, want=ref.NAMES)
    for n in ref.PROFILES:
        assert np.array_equal(_bits(got[n]), _bits(want[n])), n
    assert (got["k0"] == -1).all() and (got["enh_s"] == 1.0).all() and not _bits(got["fmelt_s"]).any()
