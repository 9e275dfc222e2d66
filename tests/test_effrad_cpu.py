"""calc_effectRad (M:4834-4935) without a GPU: the hand-built columns of tests/effrad_cases.py reach, in the oracle, every
branch the GPU tests are meant to cover (so those cannot pass on inputs that skip one), and the library exports the new
binary32 entries (the export test of test_capi_cpu.py only sees names that begin with kidmp_)."""
import os
import re
import subprocess

import numpy as np
import pytest

import effrad_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NZ = 120


@pytest.fixture(scope="module")
def oracle_aero():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True, aerosol_aware=True)      # calc_effectRad reads constants only: no mixed-phase tables needed
    yield o
    o.close()


@pytest.fixture(scope="module")
def cols():
    return ec.hand_built(NZ)


def _radii(o, col):
    return [r[0] for r in o.calc_effectRad({k: v[None, :] for k, v in col.items()})]


def test_cloud_water_sweep_reaches_preset_and_both_clamps(oracle_warm, cols):
    re_qc = _radii(oracle_warm, cols["qc_sweep"])[0]
    qc = cols["qc_sweep"]["qc"]
    assert (re_qc == 2.49e-6).sum() >= 1 and (re_qc == 2.51e-6).sum() >= 1 and (re_qc == 50e-6).sum() >= 1
    assert ((re_qc > 2.51e-6) & (re_qc < 50e-6)).sum() >= 1
    assert qc[re_qc == 2.51e-6].max() < 1e-5 and qc[re_qc == 50e-6].min() > 1e-2


def test_droplet_number_sweep_reaches_every_inu_c_branch(oracle_aero, oracle_warm, cols):
    c = cols["nc_sweep"]
    nc = np.maximum(ec.R2, c["nc"] * ec.rho_of(ec.T0))
    assert (nc < 100).sum() >= 1 and (nc > 1e10).sum() >= 1                   # inu_c = 15, inu_c = 2
    nint = np.rint(1000e6 / nc[(nc >= 100) & (nc <= 1e10)]) + 2               # the NINT branch, below and at the cap of 15
    assert (nint < 15).sum() >= 1 and (nint >= 15).sum() >= 1 and len(set(np.minimum(nint, 15))) >= 3
    re_qc = _radii(oracle_aero, c)[0]
    assert re_qc.max() == 50e-6 and re_qc.min() == 2.51e-6 and len(set(re_qc)) >= 5
    # a context that is not aerosol-aware never leaves nc = Nt_c: one value for the whole column
    assert len(set(_radii(oracle_warm, c)[0])) == 1


def test_cloud_ice_sweeps_reach_preset_and_both_clamps(oracle_warm, cols):
    for name in ("qi_sweep", "ni_sweep"):
        re_qi = _radii(oracle_warm, cols[name])[1]
        assert (re_qi == 4.99e-6).sum() >= 1 and (re_qi == 5.01e-6).sum() >= 1 and (re_qi == 125e-6).sum() >= 1, name
        assert ((re_qi > 5.01e-6) & (re_qi < 125e-6)).sum() >= 1, name
    c = cols["ni_sweep"]
    kept = _radii(oracle_warm, c)[1] == 4.99e-6
    assert np.array_equal(kept, c["ni"] * ec.rho_of(ec.T0) <= ec.R2)          # the preset exactly where ni*rho <= R2


def test_snow_sweeps_reach_clamps_only_when_warm_enough(oracle_warm, cols):
    for T in (215.0, 245.0):
        re_qs = _radii(oracle_warm, cols["qs_sweep_%g" % T])[2]
        assert (re_qs == 9.99e-6).sum() >= 1 and not (re_qs == 10e-6).any() and not (re_qs == 999e-6).any(), T
    assert abs(_radii(oracle_warm, cols["qs_sweep_215"])[2].max() - 9.8e-5) < 1e-6
    assert abs(_radii(oracle_warm, cols["qs_sweep_245"])[2].max() - 6.1e-4) < 1e-5
    for T in (268.0, 273.1, 280.0):
        re_qs = _radii(oracle_warm, cols["qs_sweep_%g" % T])[2]
        assert (re_qs == 9.99e-6).sum() >= 1 and (re_qs == 10e-6).sum() >= 1 and (re_qs == 999e-6).sum() >= 1, T
        assert ((re_qs > 10e-6) & (re_qs < 999e-6)).sum() >= 1, T


def test_snow_temperature_is_capped_at_minus_a_tenth(oracle_warm, cols):
    """tc0 = MIN(-0.1, T - 273.15): at equal rs, 273.06 K and 290 K agree to a rounding of rho, 273.0 K differs."""
    a = _radii(oracle_warm, cols["rs_sweep_273.06"])[2]
    b = _radii(oracle_warm, cols["rs_sweep_290"])[2]
    c = _radii(oracle_warm, cols["rs_sweep_273"])[2]
    free = (a > 10e-6) & (a < 999e-6)
    assert free.sum() >= 1
    assert np.max(np.abs(a - b)[free] / a[free]) < 1e-15
    assert np.max(np.abs(a - c)[free] / a[free]) > 1e-3


def test_ladders_stand_on_both_sides_of_the_thresholds(oracle_warm, cols):
    for name, idx in (("ladder_qc", 0), ("ladder_qi", 1), ("ladder_qs", 2), ("ladder_ni", 1)):
        re = _radii(oracle_warm, cols[name])[idx]
        kept = re == ec.PRESETS[idx]
        assert kept.sum() >= 1 and (~kept).sum() >= 1, name


def test_batch_leaves_out_what_the_hand_built_columns_add(oracle_mixed):
    """Why the hand-built columns exist: the batch of test_effective_radii_match_oracle never reaches the upper clamp of
    re_qc."""
    re_qc, re_qi, re_qs = oracle_mixed.calc_effectRad(ec.batch())
    assert not (re_qc == 50e-6).any()
    for r, preset in zip((re_qc, re_qi, re_qs), ec.PRESETS):
        assert (r == preset).any() and (r != preset).any()


def test_random_state_switches_every_species():
    st = ec.random_state(64, 8, 1)
    for k in ("qc", "qi", "ni", "qr", "qs", "qg"):
        assert (st[k] == 0).any() and (st[k] > 0).any(), k


NEW_ENTRIES = ("kidmp_effective_radii_host", "kidmp32_effective_radii_device", "kidmp32_effective_radii_host",
               "kidmp_column_outputs_device", "kidmp32_column_outputs_device", "kidmp_batch_step_host_out",
               "kidmp32_batch_step_host_out")


def test_library_exports_the_new_entries():
    lib = os.path.join(ROOT, "kid_amd", "libkidmp.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    have = set(re.findall(r"\bT (kidmp(?:32)?_[a-z_0-9]+)", syms))
    hdr = open(os.path.join(ROOT, "include", "kidmp.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared in include/kidmp.h"
        assert name in have, name + " is not exported by libkidmp.so"
    declared32 = set(re.findall(r"\b(kidmp32_[a-z_0-9]+)\s*\(", hdr))
    assert declared32 <= have, sorted(declared32 - have)
