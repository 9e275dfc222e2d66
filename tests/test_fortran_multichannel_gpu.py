"""Several channels through the Fortran drop-in (-m gpu): tests/fortran/kid_multichannel_driver.f90 -> module_mp_thompson09n's
radiometer_multi_batch and mie_radar_multi_batch -> the table entries and kidmp[32]_radiometer_multi_host /
kidmp[32]_mie_radar_multi_host (8-byte default REAL in build/, 4-byte in build32/).  Everything is an equality of bits
against the Python host entries on the same arrays; three channels (the W-band, Ka-band and 10-cm configurations of
tests/multichannel_cases.py), a closure and a gas profile per channel."""
import os
import subprocess

import numpy as np
import pytest

import multichannel_cases as mcc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = ("t", "p", "qv", "qc", "qr", "nr", "qs", "qg")
RAD_NAMES = ("k_abs", "k_bsc", "refl", "trans", "tb_up", "tb_down", "tb_toa", "tb_ground", "tau_abs")
MIE_NAMES = ("dbz", "dbz_up", "dbz_down", "dbz_r", "dbz_s", "dbz_g", "mie_r", "mie_s", "mie_g", "ext", "pia_up", "pia_down", "vd", "pia_total")
PER_COLUMN = ("tb_toa", "tb_ground", "tau_abs", "pia_total")
NCH = 3


def _exe(build):
    exe = os.path.join(ROOT, "kid_amd", "fortran", build, "kid_multichannel_driver")
    assert os.path.exists(exe), "build the Fortran shim first (__graft_entry__.build())"
    return exe


def _batch(build, cfgs, rcfgs, st, dz, kgs, t_sfc, w, tmp_path, *mode):
    """The driver's results: ({name: [nch, ncol, nz] or [nch, ncol]} of the radiometer, the same of the radar)."""
    ncol, nz = st["t"].shape
    nch = len(cfgs)
    f = tmp_path / "state.txt"
    with open(f, "w") as fh:
        fh.write("%d %d %d\n" % (nz, ncol, nch))
        for c, r in zip(cfgs, rcfgs):
            ew, ei = complex(c.eps_w), complex(c.eps_i)
            fh.write(" ".join(repr(float(v)) for v in (c.wavelength, ew.real, ew.imag, ei.real, ei.imag, c.kw2, r["mu"], r["emissivity"],
                                                       r["t_cosmic"])) + "\n")
        fh.write("%r %r\n" % (float(cfgs[0].rho_w), float(cfgs[0].rho_i)))
        for k in range(nz):
            fh.write(" ".join(repr(float(v)) for v in [dz[k]] + [kgs[c, k] for c in range(nch)]) + "\n")
        for i in range(ncol):
            fh.write("%r\n" % float(t_sfc[i]))
        for i in range(ncol):
            for k in range(nz):
                fh.write(" ".join(repr(float(v)) for v in [st[n][i, k] for n in INPUTS] + [w[i, k]]) + "\n")
    out = subprocess.run([_exe(build), str(f)] + list(mode), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    shape = lambda n: (nch, ncol) if n in PER_COLUMN else (nch, ncol, nz)   # noqa: E731
    got = {"RAD": {n: np.full(shape(n), -7.0) for n in RAD_NAMES}, "MIE": {n: np.full(shape(n), -7.0) for n in MIE_NAMES}}
    seen = 0
    for line in out.stdout.splitlines():
        p = line.split()
        if p and p[0] in got:
            c, i, k = int(p[2]) - 1, int(p[3]) - 1, int(p[4]) - 1
            if p[1] in PER_COLUMN:
                got[p[0]][p[1]][c, i] = float(p[5])
            else:
                got[p[0]][p[1]][c, i, k] = float(p[5])
            seen += 1
    assert seen == nch * ((6 + 13) * ncol * nz + (3 + 1) * ncol)
    return got["RAD"], got["MIE"]


def _bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, dtype, what):
    for n in want:
        assert np.array_equal(_bits(got[n].astype(dtype)), _bits(want[n])), what + (n,)


def _configs(**over):
    from kid_amd import MieCfg
    # one rho_i for the set: the shim's rho_w and rho_i are shared by the channels
    return [MieCfg(**dict(dict(kw, rho_i=917.0), **over)) for kw in mcc.configs()[:NCH]]


@pytest.mark.parametrize("build", ["build", "build32"])
@pytest.mark.parametrize("nz", [33, 129])
def test_fortran_multi_batches_equal_the_python_host_entries(gpu_mixed, tmp_path, build, nz):
    from kid_amd import RadiometerCfg
    m = gpu_mixed
    dtype = np.float64 if build == "build" else np.float32
    f = lambda a: np.ascontiguousarray(a.astype(dtype))   # noqa: E731
    full, dz, k_gas, t_sfc = mcc.radiometer_state(nz)
    _, _, w, _ = mcc.radar_state(nz)
    st = {k: f(full[k][2:7]) for k in INPUTS}
    dz, kgs, t_sfc, w = f(dz), f(mcc.k_gas_per_channel(k_gas, NCH)), f(t_sfc[2:7]), f(w[2:7])
    cfgs, rcfgs = _configs(), mcc.rcfgs(NCH)
    rad, mie = _batch(build, cfgs, rcfgs, st, dz, kgs, t_sfc, w, tmp_path)
    rt, mt = [m.radiometer_table(c) for c in cfgs], [m.mie_table(c) for c in cfgs]
    try:
        want = m.radiometer_multi_host(rt, st, dz, kgs, t_sfc, [RadiometerCfg(**r) for r in rcfgs], RAD_NAMES)
        _same(rad, want, dtype, (build, nz))
        assert (want["tau_abs"] > 0).all() and (want["k_bsc"] > 0).any() and not np.array_equal(want["tb_toa"][0], want["tb_toa"][1])
        want = m.mie_radar_multi_host(mt, st, dz, w, kgs, MIE_NAMES)
        _same(mie, want, dtype, (build, nz))
        assert (want["pia_total"] > 0).all() and not np.array_equal(want["dbz"][0], want["dbz"][2])
    finally:
        for t in rt + mt:
            t.close()


def test_fortran_multi_batches_warm_without_the_optional_arguments(gpu_warm, tmp_path):
    m, nz = gpu_warm, 33
    full, dz, k_gas, t_sfc = mcc.radiometer_state(nz)
    _, _, w, _ = mcc.radar_state(nz)
    st = {k: np.ascontiguousarray(full[k][:4]) for k in INPUTS}
    # what the shim leaves at the library's defaults: rho_w, rho_i, kw2 and the closures
    cfgs = _configs(rho_w=1000.0, rho_i=900.0, kw2=0.93)
    rad, mie = _batch("build", cfgs, mcc.rcfgs(NCH), st, dz, mcc.k_gas_per_channel(k_gas, NCH), t_sfc[:4], w[:4], tmp_path, "warm")
    bare = {k: st[k] for k in ("t", "p", "qv", "qr", "nr")}
    rt, mt = [m.radiometer_table(c) for c in cfgs], [m.mie_table(c) for c in cfgs]
    try:
        _same(rad, m.radiometer_multi_host(rt, bare, dz, want=RAD_NAMES), np.float64, ("warm",))
        _same(mie, m.mie_radar_multi_host(mt, bare, dz, want=MIE_NAMES), np.float64, ("warm",))
    finally:
        for t in rt + mt:
            t.close()
