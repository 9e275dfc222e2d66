"""The mixed-phase column kernel's hand-over of pass 5's inputs through dying LDS slots.

The wave that owns a column in passes 3-4 leaves the final rho in V_RHOK, the cleaned snow input in V_VTS0 (both under
the overlay flags in their sign bits) and the cleaned ice inputs in V_RR2 / V_NR2, once it has read those slots for the
last time; pass 5 (band-mapped: another wave of the workgroup) takes them from there instead of from memory, and stores
T and qc only where block Q changed them.  These are the smallest shapes at which that can go wrong: every level-group
count and both workgroup shapes (nz <= 120: four columns per workgroup, above: one), every remainder of the last
workgroup, a dry column next to live ones, and inputs that make the shared slots matter -- levels either side of T_0
and of 270.65 K with ice present and the cloud water evaporating (the overlay flags and qcten / ncten share their slots
with the parked values), snow exactly zero and just above R1, rain falling to the ground (V_RR2 / V_NR2 live
until the end of the rain sedimentation).  HIP path against the oracle through parity.assert_parity at its own bounds.
"""
import functools

import numpy as np
import pytest

import cases
import kat_cases as kc
from parity import MAX_SENSITIVE_FRAC, branch_aware_compare, assert_parity
from rates_parity import assert_rates

T_0, R1 = 273.15, 1e-12
NZS = [2, 17, 64, 65, 120, 121, 200]          # 121 and 200: one column per workgroup, the band is the wave's own column
NCOLS = [1, 3, 4, 5]                          # the last workgroup has columns beyond ncol
SENS_CUT = 1e-11                              # parity.verdict: beyond it a level leans on the sensitivity allowance


def _resample(col, nz):
    x0 = np.linspace(0.0, 1.0, col["qv"].shape[0])
    x1 = np.linspace(0.0, 1.0, nz)
    out = {k: np.interp(x1, x0, v) for k, v in col.items()}
    out["dz"] = np.full(nz, 15000.0 / nz)
    return out


def _rain_to_ground(c):
    n = max(1, c["qr"].shape[0] // 6)
    c["qr"][:n] = 1e-3
    c["nr"][:n] = 5e3


def _melting_levels(c, shift=0.0):
    """Levels around T_0 with ice, snow and a trace of cloud water in subsaturated air: block Q melts ice into a level
    whose cloud water has just evaporated.  Temperatures straddle T_0 (nc overlay) and 270.65 K (qc overlay)."""
    nz = c["t"].shape[0]
    kx = int(np.argmin(np.abs(c["t"] - T_0)))
    for dk, temp in ((-1, T_0 + 0.8), (0, T_0 + 0.05), (1, T_0 - 0.05), (2, 271.0), (3, 270.6)):
        k = kx + dk
        if 0 <= k < nz:
            c["t"][k] = temp + shift
            c["qi"][k], c["ni"][k], c["qs"][k] = 5e-5, 5e4, 1e-3
            c["qc"][k] = 1e-9
            c["qv"][k] *= 0.9


@functools.lru_cache(maxsize=None)
def _columns(nz):
    a = _resample(kc.kat_a(True), nz)
    melt = {k: v.copy() for k, v in a.items()}                       # 0 T_0 crossing with ice, qc depleted; rain to the ground
    _melting_levels(melt)
    _rain_to_ground(melt)
    dry = {k: v.copy() for k, v in a.items()}                        # 1 no_micro: leaves the workgroup after pass 0
    for k in ("qc", "qi", "qr", "qs", "qg", "ni", "nr"):
        dry[k][:] = 0.0
    dry["qv"][:] = 1.0e-6
    heavy = _resample(kc.kat_c(), nz)                                # 2 no snow, no ice at all; heavy rain and graupel to the ground
    heavy["qs"][:] = 0.0
    thin = {k: v.copy() for k, v in a.items()}                       # 3 snow just above R1, and exactly zero at every third level
    thin["qs"] = np.where(thin["qs"] > 0, 1.5 * R1, 0.0)             # (not exactly R1: the ulp probes of parity.py straddle it)
    thin["qs"][::3] = 0.0
    _melting_levels(thin, shift=0.02)
    warmer = {k: v.copy() for k, v in a.items()}                     # 4 the whole column 1.3 K warmer, rain to the ground
    warmer["t"] = warmer["t"] + 1.3
    _rain_to_ground(warmer)
    return [melt, dry, heavy, thin, warmer]


LONG_STEP = (3, 1, 2, 4)                      # the dt = 60 s batch: without column 0, which the oracle itself holds less
                                              # steady over a long step (8 of its 120 levels beyond SENS_CUT)


def _batch(nz, ncol, w=None, pick=None):
    cols = [_columns(nz)[i] for i in pick] if pick else _columns(nz)[:ncol]
    st = {k: np.ascontiguousarray(np.stack([c[k] for c in cols])) for k in cases.KEYS}
    if w is not None:
        st["w"][:] = w
    return st


def _allowed(n_levels):
    return int(np.ceil(MAX_SENSITIVE_FRAC * n_levels))


def _run(m, o, st, dt, rates=False, **kw):
    got = {k: v.copy() for k, v in st.items()}
    gppt, grates = m.batch_step_host(got, dt, want_rates=rates)
    v = assert_parity(o, st, dt, got, gppt, **kw)
    print(st["qv"].shape, dt, v)
    return (got, grates) if rates else got


@pytest.mark.slow
def test_inputs_are_well_conditioned(oracle_mixed):
    """CPU, the oracle alone: the chosen inputs leave no more than MAX_SENSITIVE_FRAC of the levels to the sensitivity
    allowance of the comparison (levels whose oracle output itself moves under ulp-sized perturbations)."""
    for nz in NZS:
        for ncol, dt in [(n, 10.0) for n in NCOLS] + ([(4, 60.0)] if nz == 120 else []):
            st = _batch(nz, ncol, pick=LONG_STEP if dt > 10.0 else None)
            ref = {k: v.copy() for k, v in st.items()}
            oracle_mixed.batch_step(ref, dt)
            cmp = branch_aware_compare(oracle_mixed, st, dt, ref, depletion=1e-5 if dt > 10.0 else 0.0)
            n_sens = int((cmp["sens"] > SENS_CUT).sum())
            print(nz, ncol, dt, "sensitive levels", n_sens, "of", cmp["sens"].size, "branch levels", int((cmp["flags"] != 0).sum()))
            assert n_sens <= _allowed(cmp["sens"].size), (nz, ncol, dt, n_sens, cmp["sens"].size)


@pytest.mark.slow
def test_inputs_are_well_conditioned_aerosol_aware(oracle_mixed_aero):
    for nz in (120, 121):
        st = _batch(nz, 5, w=2.0)
        ref = {k: v.copy() for k, v in st.items()}
        oracle_mixed_aero.batch_step(ref, 10.0)
        cmp = branch_aware_compare(oracle_mixed_aero, st, 10.0, ref)
        n_sens = int((cmp["sens"] > SENS_CUT).sum())
        print(nz, "aerosol-aware: sensitive levels", n_sens, "of", cmp["sens"].size, "branch levels", int((cmp["flags"] != 0).sum()))
        assert n_sens <= _allowed(cmp["sens"].size), (nz, n_sens, cmp["sens"].size)


def test_inputs_reach_the_shared_slots():
    """The batch holds what the hand-over has to survive (checked on the inputs, no GPU)."""
    melt, dry, heavy, thin, warmer = _columns(120)
    assert ((melt["t"] > T_0) & (melt["qi"] > R1) & (melt["qc"] > R1)).any()
    assert ((melt["t"] < T_0) & (melt["t"] >= 270.65) & (melt["qi"] > R1)).any() and (melt["t"] == 270.6).any()
    assert not heavy["qs"].any() and not heavy["qi"].any() and heavy["qr"][0] > R1 and melt["qr"][0] > R1
    assert (thin["qs"] == 1.5 * R1).any() and (thin["qs"][thin["qi"] > R1] == 0.0).any()
    assert not any(dry[k].any() for k in ("qc", "qi", "qr", "qs", "qg"))


@pytest.mark.gpu
@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nz", NZS)
def test_handover_matches_oracle(gpu_mixed, oracle_mixed, nz, ncol):
    st = _batch(nz, ncol)
    got = _run(gpu_mixed, oracle_mixed, st, 10.0, max_branch_frac=0.2)
    if ncol >= 3:                                                    # the dry column: block B's zeroes, nothing else
        assert not got["qs"][1].any() and not got["qi"][1].any() and np.array_equal(got["t"][1], st["t"][1])


@pytest.mark.gpu
def test_handover_more_substeps(gpu_mixed, oracle_mixed):
    """dt = 60 s: more sedimentation substeps between the parking stores and pass 5 (depleted species are measured
    against 1e-5 of their input, as in the other long-step tests)."""
    _run(gpu_mixed, oracle_mixed, _batch(120, 4, pick=LONG_STEP), 60.0, max_branch_frac=0.2, depletion=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("nz", [120, 121])
def test_handover_rates_instantiation(gpu_mixed, oracle_mixed, nz):
    """The kernel compiled with the rate diagnostics (256 VGPRs, two waves per SIMD) takes the same hand-over, and the
    rates it stores on the way are the oracle's (rates_parity.assert_rates; every other level count:
    test_gpu_rates_shapes.py)."""
    st = _batch(nz, 5)
    _, rates = _run(gpu_mixed, oracle_mixed, st, 10.0, rates=True, max_branch_frac=0.2)
    v = assert_rates(oracle_mixed.column_step, st, 10.0, rates)
    print("rates", nz, {k: x for k, x in v.items() if k != "cmp"})


@pytest.mark.gpu
@pytest.mark.parametrize("nz", [120, 121])
def test_handover_aerosol_instantiation(gpu_mixed_aero, oracle_mixed_aero, nz):
    _run(gpu_mixed_aero, oracle_mixed_aero, _batch(nz, 5, w=2.0), 10.0, max_branch_frac=0.2)
