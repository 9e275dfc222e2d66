"""CPU, the oracle alone: the inputs of rates_cases.py leave the rate comparison of rates_parity.py room to hold.

The share of elements that assert_rates lets lean on the sensitivity allowance (rates_parity.MAX_BEYOND_FRAC) is a
condition on the inputs, checked here without a GPU: the oracle's own rates, stepped from inputs moved by 2 ulp
(the probes of parity._PERT), stay within 1e-11 of themselves on all but that share of the elements, at every level
count and for every kind of context.  And the inputs reach what they are meant to reach: every one of the 36 rows
from nz = 64 on (mixed phase, aerosol-aware), the six warm rows in the warm-rain batch, a no_micro column at DRY.
"""
import numpy as np
import pytest

import rates_cases as rc
from rates_parity import MAX_BEYOND_FRAC, NRATES, oracle_rates, rates_compare

SENS_CUT = 1e-11                     # parity.verdict: beyond it an element leans on the sensitivity allowance


def _survey(oracle, kind):
    for nz in rc.levels(kind):
        st = rc.batch(kind, nz)
        ref_in = {k: v.copy() for k, v in st.items()}
        cmp = rates_compare(oracle.column_step, st, rc.DT, np.zeros((rc.NCOL, NRATES, nz)))
        for k in st:                                          # the comparison leaves its input alone
            assert np.array_equal(st[k], ref_in[k]), k
        sens, ref = cmp["sens"], cmp["ref"]
        rows = np.any(ref != 0, axis=(0, 2))
        print("%-5s nz %3d: worst self-response %.1e, elements > 1e-11: %d, > 1e-10: %d, of %d; rows reached %d"
              % (kind, nz, sens.max(), (sens > SENS_CUT).sum(), (sens > 1e-10).sum(), sens.size, rows.sum()))
        assert np.isfinite(ref).all() and np.isfinite(sens).all(), (kind, nz)
        assert (sens > SENS_CUT).sum() <= int(np.ceil(MAX_BEYOND_FRAC * sens.size)), (kind, nz, int((sens > SENS_CUT).sum()))
        if kind == "warm":
            # (two levels, the ground and 15 km: rain evaporates and collects itself, no cloud water to convert --
            #  rows 32, 34, 35 are all the oracle produces there)
            assert not rows[:30].any() and (rows[30:].all() if nz > 2 else rows[[32, 34, 35]].all()), (nz, np.flatnonzero(rows))
        else:
            assert cmp["dry"].tolist() == [c == rc.DRY for c in range(rc.NCOL)], (kind, nz, cmp["dry"])
            assert not ref[rc.DRY].any()
            if nz >= 64:
                assert rows.all(), (kind, nz, np.flatnonzero(~rows))


@pytest.mark.slow
def test_mixed_inputs_keep_the_rates_steady_and_reach_every_row(oracle_mixed):
    _survey(oracle_mixed, "mixed")
    for nz in (2, 63, 65, 121, 129, 193, 255):              # the all-dry batch of the buffer test: no_micro everywhere
        ref, dry = oracle_rates(oracle_mixed.column_step, rc.all_dry("mixed", nz), rc.DT)
        assert dry.all() and not ref.any(), nz


@pytest.mark.slow
def test_aerosol_aware_inputs_keep_the_rates_steady_and_reach_every_row(oracle_mixed_aero):
    _survey(oracle_mixed_aero, "aero")


def test_warm_inputs_keep_the_rates_steady_and_reach_the_warm_rows(oracle_warm):
    _survey(oracle_warm, "warm")
