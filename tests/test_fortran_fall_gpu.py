"""The fall speeds through the Fortran drop-in (-m gpu): tests/fortran/kid_fall_driver.f90 -> module_mp_thompson09n's
fall_speeds_batch -> kidmp_fall_speeds_host (8-byte default REAL) / kidmp32_fall_speeds_host (4-byte), and the adapter's
l_precip_flux.  Everything is an equality of bits: fall_speeds_batch against the Python host entry on the same arrays,
the save_dg record with the switch off against kid_mini_driver's, and 'total_ppt_level' with the switch on against
dt * flux_total of the post-step state the adapter left."""
import os
import subprocess

import numpy as np
import pytest

import effrad_cases as ec
import fall_cases as fc
import fall_speeds_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 10.0                                                   # `dt` of tests/fortran/kid_stubs.f90


def _exe(build, name="kid_fall_driver"):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, name)
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


def _batch(build, st, boost, dz, dt, tmp_path, *mode):
    ncol, nz = st["t"].shape
    f = tmp_path / "state.txt"
    with open(f, "w") as fh:
        fh.write("%d %d %r\n" % (nz, ncol, dt))
        fh.write("".join("%r\n" % float(v) for v in dz))
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(st[n][i, k])) for n in ref.INPUTS) + " %r\n" % float(boost[i, k]))
    out = subprocess.run([_exe(build), "batch", str(f)] + list(mode), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {n: np.full((ncol, nz), -7.0) for n in ref.NAMES}
    nstep = np.full((ncol, 4), -7, dtype=np.int32)
    seen = 0
    for line in out.stdout.splitlines():
        p = line.split()
        if p and p[0] == "FALL":
            got[p[1]][int(p[2]) - 1, int(p[3]) - 1] = float(p[4])
            seen += 1
        elif p and p[0] == "NSTEP":
            nstep[int(p[1]) - 1] = [int(x) for x in p[2:6]]
    assert seen == 11 * ncol * nz and (nstep != -7).all()
    return got, nstep


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("build", ["build", "build32"])
@pytest.mark.parametrize("nz,ncol", [(120, 5), (65, 2)])
def test_fortran_fall_speeds_batch_equals_the_python_host_entry(gpu_mixed, tmp_path, build, nz, ncol):
    dtype = np.float64 if build == "build" else np.float32
    st = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in fc.only(ec.random_state(nz, ncol, 80 + nz)).items()}
    rng = np.random.Generator(np.random.PCG64(81 + nz))
    dz = np.exp(rng.uniform(np.log(10.0), np.log(400.0), nz)).astype(dtype)
    boost = np.ascontiguousarray(rng.uniform(1.0, 1.5, (ncol, nz)).astype(dtype))
    got, nstep = _batch(build, st, boost, dz, DT, tmp_path)
    want = gpu_mixed.fall_speeds_host(st, boost, dz, DT)
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n].astype(dtype)), _bits(want[n])), (build, n)
    assert np.array_equal(nstep, want["nstep"])
    assert all((want[n] > 0).any() for n in ref.NAMES) and want["nstep"].max() > 1


def test_fortran_fall_speeds_batch_warm_without_the_optional_arguments(gpu_warm, tmp_path):
    st = fc.only(ec.random_state(120, 3, 91))
    dz = np.full(120, 40.0)
    got, nstep = _batch("build", st, np.ones((3, 120)), dz, DT, tmp_path, "warm")
    want = gpu_warm.fall_speeds_host({k: st[k] for k in ("t", "p", "qv", "qr", "nr")}, None, dz, DT)
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n]), _bits(want[n])), n
    assert np.array_equal(nstep, want["nstep"]) and (nstep[:, 1:] == 1).all()
    assert not _bits(got["vt_s"]).any() and not _bits(got["flux_g"]).any()                 # +0.0


def _kid(tmp_path, sub, exe, args):
    d = tmp_path / sub
    d.mkdir()
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600, cwd=str(d))
    assert out.returncode == 0, out.stdout + out.stderr
    return d


@pytest.mark.parametrize("case", ["mixed", "warm"])
def test_l_precip_flux(request, tmp_path, case):
    nx, nsteps, step = 3, 3, 3
    mini = _kid(tmp_path, "mini", _exe("build", "kid_mini_driver"), [nx, nsteps, case, step])
    off = _kid(tmp_path, "off", _exe("build"), ["kid", nx, nsteps, case, step, 0])
    on = _kid(tmp_path, "on", _exe("build"), ["kid", nx, nsteps, case, step, 1])
    rec = {k: open(d / "dg_dump.txt").read().splitlines() for k, d in (("mini", mini), ("off", off), ("on", on))}
    assert rec["off"] == rec["mini"] and len(rec["mini"]) > 120 * nx                          # the switch off: today's record
    assert len(rec["on"]) == len(rec["off"])
    differ = [(a, b) for a, b in zip(rec["off"], rec["on"]) if a != b]
    assert differ and all(a.split()[1] == "total_ppt_level" == b.split()[1] for a, b in differ)
    for a, b in differ:                                                                         # name, indices, units, dim unchanged
        pa, pb = a.split(), b.split()
        assert pa[:4] == pb[:4] and pa[5:] == pb[5:] and float(pa[4]) == 0.0
    # its values: dt * flux_total of the post-step state
    post = np.loadtxt(on / "post_state.txt").reshape(nx, 120, 9)
    st = {k: np.ascontiguousarray(post[:, :, j]) for j, k in enumerate(ref.INPUTS)}
    m = request.getfixturevalue("gpu_warm" if case == "warm" else "gpu_mixed")
    want = DT * m.fall_speeds_host(st, want=("flux_total",))["flux_total"]
    got = np.full((nx, 120), -7.0)
    for line in rec["on"]:
        p = line.split()
        if p[1] == "total_ppt_level":
            assert p[0] == "2d" and p[-1] == "z,x"
            got[int(p[3]) - 1, int(p[2]) - 1] = float(p[4])
    assert np.array_equal(_bits(got), _bits(want)) and (got > 0).any()


def test_l_precip_flux_needs_one_device(tmp_path):
    """kidmp_ndevices > 1 with the switch set stops with the message the other one-GPU diagnostics use, before anything is
    initialised (no second device is asked for)."""
    out = subprocess.run([_exe("build"), "kid", "3", "1", "mixed", "0", "1", "2"], capture_output=True, text=True, timeout=120,
                         cwd=str(tmp_path))
    assert out.returncode != 0
    assert "mphys_thompson09n: l_precip_flux is not available with kidmp_ndevices > 1" in out.stdout
