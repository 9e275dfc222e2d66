"""The cloud radar through the Fortran drop-in (-m gpu): tests/fortran/kid_mie_driver.f90 -> module_mp_thompson09n's
mie_radar_batch -> kidmp_mie_table_create and kidmp_mie_radar_host (8-byte default REAL) / kidmp32_mie_radar_host (4-byte).
Everything is an equality of bits against the Python host entry on the same arrays."""
import os
import subprocess

import numpy as np
import pytest

import mie_radar_ref as ref
from mie_radar_cases import CFGS, state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = ref.NAMES[:-1]


def _exe(build):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_mie_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


def _batch(build, cfg, st, dz, w, k_gas, tmp_path, *mode):
    ncol, nz = st["t"].shape
    f = tmp_path / "state.txt"
    with open(f, "w") as fh:
        fh.write("%d %d\n" % (nz, ncol))
        ew, ei = complex(cfg["eps_w"]), complex(cfg["eps_i"])
        fh.write(" ".join(repr(float(v)) for v in (cfg["wavelength"], ew.real, ew.imag, ei.real, ei.imag, cfg["rho_w"], cfg["rho_i"], cfg["kw2"])) + "\n")
        for k in range(nz):
            fh.write("%r %r\n" % (float(dz[k]), float(k_gas[k])))
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(a[i, k])) for a in [st[n] for n in ref.INPUTS] + [w]) + "\n")
    out = subprocess.run([_exe(build), str(f)] + list(mode), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = dict({n: np.full((ncol, nz), -7.0) for n in PROFILES}, pia_total=np.full(ncol, -7.0))
    seen = 0
    for line in out.stdout.splitlines():
        p = line.split()
        if p and p[0] == "MIE":
            i, k = int(p[2]) - 1, int(p[3]) - 1
            if p[1] == "pia_total":
                got["pia_total"][i] = float(p[4])
            else:
                got[p[1]][i, k] = float(p[4])
            seen += 1
    assert seen == 13 * ncol * nz + ncol
    return got


def _bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


@pytest.mark.parametrize("build", ["build", "build32"])
@pytest.mark.parametrize("nz, name", [(120, "w"), (65, "ka")])
def test_fortran_mie_radar_batch_equals_the_python_host_entry(gpu_mixed, tmp_path, build, nz, name):
    from kid_amd import MieCfg
    dtype = np.float64 if build == "build" else np.float32
    full, dz, w, k_gas = state(nz)
    st = {k: np.ascontiguousarray(full[k][:5].astype(dtype)) for k in ref.INPUTS}
    dz, w, k_gas = dz.astype(dtype), np.ascontiguousarray(w[:5].astype(dtype)), k_gas.astype(dtype)
    got = _batch(build, CFGS[name], st, dz, w, k_gas, tmp_path)
    with gpu_mixed.mie_table(MieCfg(**CFGS[name])) as t:
        want = gpu_mixed.mie_radar_host(t, st, dz, w, k_gas, want=ref.NAMES)
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n].astype(dtype)), _bits(want[n])), (build, n)
    assert (want["pia_total"] > 0).all() and (np.abs(want["mie_r"] - 1.0) > 0.1).any()


def test_fortran_mie_radar_batch_warm_without_the_optional_arguments(gpu_warm, tmp_path):
    from kid_amd import MieCfg
    full, dz, w, k_gas = state(64)
    st = {k: np.ascontiguousarray(full[k][:4]) for k in ref.INPUTS}
    cfg = dict(CFGS["ka"], rho_w=1000.0, rho_i=900.0, kw2=0.93)               # what the shim leaves at the library's defaults
    got = _batch("build", cfg, st, dz, np.ascontiguousarray(w[:4]), k_gas, tmp_path, "warm")
    with gpu_warm.mie_table(MieCfg(**cfg)) as t:
        want = gpu_warm.mie_radar_host(t, {k: st[k] for k in ("t", "p", "qv", "qr", "nr")}, dz, want=ref.NAMES)
    for n in ref.NAMES:
        assert np.array_equal(_bits(got[n]), _bits(want[n])), n
    assert (got["mie_s"] == 1.0).all() and (got["mie_g"] == 1.0).all()
