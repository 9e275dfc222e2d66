"""The adapter's l_device_adapter through the Fortran drop-in (-m gpu): tests/fortran/kid_devadapter_driver.f90 calls
mphys_thompson09_interfacen with the switch on, which hands KiD's fields to mp_thompson_kid_interface ->
kidmp[32]_kid_interface_host -> gather, step and back-out on the GPU.  The oracle side, the metric and the bound are
those of tests/test_fortran_gpu.py (the case of its forcing test: nx = 3, forcing=1, warm and mixed)."""
import os
import subprocess

import numpy as np
import pytest

from test_fortran_gpu import _check_mphys, _oracle_adapter

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kid_amd", "fortran", "build", "kid_devadapter_driver")
EXE32 = os.path.join(ROOT, "kid_amd", "fortran", "build32", "kid_devadapter_driver")
_ENV = dict(os.environ, OMP_NUM_THREADS="8")
P64 = np.array([1.530434, 2.218719e-2, 2.694135e-3, 1.060568e6])       # reference P64 end state of KAT-B
NATIVE = np.array([1.530434, 2.218541e-2, 2.693803e-3, 1.060634e6])    # reference native P32n end state


def _run(exe, cwd, nx, nsteps, case, *opts, check=True):
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    out = subprocess.run([exe, str(nx), str(nsteps), case] + list(opts), capture_output=True, text=True, timeout=900,
                         cwd=str(cwd), env=_ENV)
    if check:
        assert out.returncode == 0, out.stdout + out.stderr
    vals = {}
    for line in out.stdout.splitlines():
        p = line.split()
        if p and p[0] in ("KATB", "KATBN"):
            vals[p[0]] = np.array([float(x) for x in p[1:5]])
    return vals, out


@pytest.mark.parametrize("case", ["warm", "mixed"])
def test_device_adapter_forcing_terms_match_oracle(tmp_path, oracle_warm, oracle_mixed, case):
    nx = 3
    _run(EXE, tmp_path, nx, 6, case, "adapter=1", "forcing=1", "mphys=5")
    d = np.loadtxt(os.path.join(str(tmp_path), "mphys_dump.txt")).reshape(nx, 120, 38)
    assert np.abs(d[:, :, 11]).max() > 1e-4 and np.abs(d[:, :, 13]).max() > 1e-8 and np.abs(d[:, :, 15:29]).max() > 1e-9
    oracle = oracle_warm if case == "warm" else oracle_mixed
    got, want = _check_mphys(d, _oracle_adapter(oracle, d, nx), nx, case)
    assert np.abs(got[2]).max() > 0 and np.abs(got[3]).max() > 0          # cloud and rain tendencies are there
    if case == "warm":
        assert np.all(d[:, :, 34:38] == 0.0)                              # no frozen-species tendency out of a warm run
    # the host loops give the same tendencies to the bound (not the bits: p is formed by another pow)
    off = tmp_path / "off"
    off.mkdir()
    _run(EXE, off, nx, 6, case, "adapter=0", "forcing=1", "mphys=5")
    d0 = np.loadtxt(os.path.join(str(off), "mphys_dump.txt")).reshape(nx, 120, 38)
    _check_mphys(d0, _oracle_adapter(oracle, d0, nx), nx, case + " (switch off)")


def _names(path):
    return [(p[0], p[1], p[2], p[3]) + tuple(p[5:]) for p in (line.split() for line in open(path))]


@pytest.mark.parametrize("case,nx,opts", [("warm", 1, ()), ("mixed", 3, ()), ("mixed", 3, ("radar=1", "radii=1")), ("warm", 2, ("rates=0",))])
def test_save_dg_sequence_is_the_same_with_the_switch(tmp_path, case, nx, opts):
    """Every save_dg call of a step -- form, name, indices, units, dim, in order -- with the switch on and off."""
    seq = {}
    for sw in ("0", "1"):
        d = tmp_path / sw
        d.mkdir()
        _run(EXE, d, nx, 4, case, "adapter=" + sw, "forcing=1", "dump=3", *opts)
        seq[sw] = _names(os.path.join(str(d), "dg_dump.txt"))
    assert len(seq["1"]) > 0 and seq["0"] == seq["1"]
    if "radar=1" in opts:
        assert any(e[1] == "dBZ" for e in seq["1"]) and any(e[1] == "re_snow" for e in seq["1"])


def test_kat_b_360_steps_with_the_switch(tmp_path):
    got, _ = _run(EXE, tmp_path, 1, 360, "warm", "adapter=1")
    print("KAT-B, l_device_adapter, 8-byte REAL:", got["KATB"])
    for g, r in zip(got["KATB"], P64):
        assert abs(g / r - 1) < 1e-6, got["KATB"]


def test_columns_are_independent_with_the_switch(tmp_path):
    small, _ = _run(EXE, tmp_path, 5, 6, "warm", "adapter=1")
    big, _ = _run(EXE, tmp_path, 3000, 6, "warm", "adapter=1")          # several pipeline chunks
    assert np.array_equal(big["KATB"], big["KATBN"]) and np.array_equal(big["KATB"], small["KATB"])


def test_kat_b_native_real4_build_with_the_switch(tmp_path):
    """KiD's default 4-byte REAL with kidmp_arith = p32n: the bound the project asserts for the p32n kernel through the
    host adapter (tests/test_fortran_gpu.py), 2.5e-5 of the reference's native digits."""
    assert os.path.exists(EXE32), "build32 not built (__graft_entry__.build())"
    got, _ = _run(EXE32, tmp_path, 1, 360, "warm", "adapter=1", "arith=p32n")
    off, _ = _run(EXE32, tmp_path, 1, 360, "warm", "adapter=0", "arith=p32n")
    print("KAT-B, 4-byte REAL, p32n: switch on", got["KATB"], "relative to native", got["KATB"] / NATIVE - 1,
          "; switch off", off["KATB"], off["KATB"] / NATIVE - 1)
    assert np.all(np.abs(got["KATB"] / NATIVE - 1) < 2.5e-5), got["KATB"]


def test_the_switch_refuses_what_it_cannot_do(tmp_path):
    _, out = _run(EXE, tmp_path, 2, 2, "warm", "adapter=1", "devices=0,0", check=False)
    assert out.returncode != 0 and "l_device_adapter is not available with kidmp_ndevices > 1" in out.stdout + out.stderr
    # arrays go to the library as they are: the 4-byte build cannot feed the binary64 entry, nor the 8-byte build kidmp32_*
    _, out = _run(EXE, tmp_path, 1, 2, "warm", "adapter=1", "arith=p32n", check=False)
    assert out.returncode != 0 and "default REAL" in out.stdout + out.stderr
    _, out = _run(EXE32, tmp_path, 1, 2, "warm", "adapter=1", check=False)
    assert out.returncode != 0 and "default REAL" in out.stdout + out.stderr
