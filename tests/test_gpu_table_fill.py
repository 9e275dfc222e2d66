"""The ln / 2**x tables of fastmath.h are requested at kernel entry and fenced by a barrier inside pass 0.

A thread of the binary64 mixed-phase column kernel requests its entry of the 1 536 B with its first instructions, stores
it to LDS once the column's first-touch loads are issued, and the workgroup meets at a barrier between blocks B and E,
ahead of the first logarithm (the binary32-state builds still fill and synchronise at entry; the warm-rain kernel stores
ahead of the barrier before pass 1).  What can go wrong: a table read ahead of the fill, and a wave that owns no column
-- beyond ncol, or through the no_micro exit after block B -- and so skips its share of the fill or the barrier, yet takes
bands of the rate sweep and evaluates logarithms there.  An unfilled table sends most columns astray at once (DESIGN,
round 4: 214 of 256 drift columns), so plain parity shows it.  The smallest shapes at which it can show: batches whose
workgroups have waves without a column (ncol = 1, 2, 3, 5, 9), the dry no_micro column beside a plain mixed one, every
level-group count and both workgroup shapes (nz <= 120: four columns per workgroup, above: one), every compiled variant
that fills at entry or shares the code around it, and two consecutive launches on one context from the same inputs --
the second finds in LDS whatever the first left there, and must give the first one's bits.

binary64: parity.assert_parity against the oracle at its own bounds (the call of test_gpu_variants.test_other_time_steps
on the same columns), rates_parity.assert_rates for the rate diagnostics.  binary32 builds: the statistic and bounds of
test_gpu_precision on its own 64-column recipe, and the bits of a column in a small batch against its bits in that
batch, where every wave owns a column (the property of test_binary32_columns_keep_their_bits_in_a_smaller_batch).
"""
import functools

import numpy as np
import pytest

import cases
from parity import MAX_SENSITIVE_FRAC, OUT, assert_parity, branch_aware_compare
from rates_parity import assert_rates
from test_gpu_precision import _columns32, _stats, _to32
from test_gpu_variants import _resample

DT = 10.0
NCOLS = [1, 2, 3, 5, 9]                      # waves without a column in the only / the last workgroup (nz <= 120)
NZS = [33, 64, 120, 129, 200]                # NJ = 1, 1, 2, 3, 4; four columns per workgroup up to 120, one above
KINDS = ["mixed", "rates", "aero", "nd", "warm"]
FROZEN = ("qi", "ni", "qs", "qg")
SENS_CUT = 1e-11                             # parity.verdict: beyond it a level leans on the sensitivity allowance


@functools.lru_cache(maxsize=None)
def _edge_columns(nz):
    """cases.edge_cases() on nz levels: 0 plain mixed, 1 the dry no_micro column, 2.. the rest; the column of values
    near the R1 thresholds comes last (the oracle itself holds a tenth of its levels less steady than SENS_CUT: only the
    batch of nine is large enough to carry it within parity.MAX_SENSITIVE_FRAC)."""
    ec = cases.edge_cases()
    cols = [{k: v[i] for k, v in ec.items()} for i in (0, 1, 2, 4, 5, 6, 7, 8, 3)]
    return cols if nz == cases.NZ else [_resample(c, nz) for c in cols]


def _batch(kind, nz, ncol):
    cols = _edge_columns(nz)[:ncol]
    st = {k: np.ascontiguousarray(np.stack([c[k] for c in cols])) for k in cases.KEYS}
    if kind == "warm":                                        # an iiwarm context: no frozen species (test_gpu_variants)
        for k in FROZEN:
            st[k][:] = 0.0
    if kind == "aero":
        st["w"][:] = 2.0                                      # an updraft, so that activation has something to do
    return st


_PAIRS = {"mixed": ("gpu_mixed", "oracle_mixed"), "rates": ("gpu_mixed", "oracle_mixed"), "nd": ("gpu_mixed", "oracle_mixed"),
          "aero": ("gpu_mixed_aero", "oracle_mixed_aero"), "warm": ("gpu_warm", "oracle_warm")}


def _copy(st):
    return {k: np.ascontiguousarray(v.copy()) for k, v in st.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _allowed(n_levels):
    return int(np.ceil(MAX_SENSITIVE_FRAC * n_levels))


@pytest.mark.slow
@pytest.mark.parametrize("kind", ["mixed", "aero", "warm"])
def test_inputs_are_well_conditioned(request, kind):
    """CPU, the oracle alone: the chosen inputs leave no more than parity.MAX_SENSITIVE_FRAC of the levels to the
    sensitivity allowance of the comparison, so a pass below is a pass on the levels themselves."""
    o = request.getfixturevalue(_PAIRS[kind][1])
    for nz in NZS:
        for ncol in NCOLS:
            st = _batch(kind, nz, ncol)
            ref = _copy(st)
            o.batch_step(ref, DT)
            cmp = branch_aware_compare(o, st, DT, ref)
            n_sens = int((cmp["sens"] > SENS_CUT).sum())
            print(kind, nz, ncol, "sensitive levels", n_sens, "of", cmp["sens"].size, "branch levels", int((cmp["flags"] != 0).sum()))
            assert n_sens <= _allowed(cmp["sens"].size), (kind, nz, ncol, n_sens, cmp["sens"].size)
            assert (cmp["flags"] != 0).sum() <= 0.2 * cmp["flags"].size, (kind, nz, ncol)


def test_the_batches_hold_a_dry_column_beside_a_mixed_one():
    for nz in NZS:
        plain, dry = _edge_columns(nz)[:2]
        assert (plain["qc"] > 1e-12).any() and (plain["qi"] > 1e-12).any() and (plain["qr"] > 1e-12).any()
        assert not any((dry[k] > 1e-12).any() for k in ("qc", "qi", "qr", "qs", "qg"))


@pytest.mark.gpu
@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nz", NZS)
@pytest.mark.parametrize("kind", KINDS)
def test_two_launches_match_the_oracle(request, kind, nz, ncol):
    """binary64, every variant: two consecutive launches on one context from the same inputs give the same bits, and
    those are the oracle's step."""
    m, o = (request.getfixturevalue(f) for f in _PAIRS[kind])
    st = _batch(kind, nz, ncol)
    try:
        if kind == "nd":                                      # a bound per-column droplet number, at the context's own value
            m.set_column_nc(np.full(ncol, 100.0))
        first, got = _copy(st), _copy(st)
        fppt, frates = m.batch_step_host(first, DT, want_rates=kind == "rates")
        ppt, rates = m.batch_step_host(got, DT, want_rates=kind == "rates")
        for k in OUT:
            assert np.array_equal(_bits(got[k]), _bits(first[k])), k
        assert np.array_equal(_bits(ppt), _bits(fppt))
        v = assert_parity(o, st, DT, got, ppt, max_branch_frac=0.2)
        print(kind, nz, ncol, v)
        if kind == "rates":
            assert np.array_equal(_bits(rates), _bits(frates))
            rv = assert_rates(o.column_step, st, DT, rates)
            print(kind, nz, ncol, "rates", {k: x for k, x in rv.items() if k != "cmp"})
        if ncol >= 2:                                         # the dry column: block B's zeroes and nothing else
            assert not any(got[k][1].any() for k in ("qc", "qi", "qr", "qs", "qg"))
            assert np.array_equal(got["t"][1], st["t"][1]) and np.array_equal(got["qv"][1], st["qv"][1])
    finally:
        if kind == "nd":
            m.set_column_nc(None)


@pytest.mark.gpu
@pytest.mark.parametrize("nz", NZS)
def test_a_batch_of_one_dry_column(gpu_mixed, oracle_mixed, nz):
    """No wave of the workgroup reaches the sweep with a column: one leaves through no_micro, three own none."""
    dry = _edge_columns(nz)[1]
    st = {k: np.ascontiguousarray(dry[k][None].copy()) for k in cases.KEYS}
    got = _copy(st)
    ppt, _ = gpu_mixed.batch_step_host(got, DT)
    assert_parity(oracle_mixed, st, DT, got, ppt)
    assert not ppt.any() and not got["qc"].any()


# ---- the binary32 builds ----
_shared = {}


def _full32(iiwarm, nz):
    """The 64 binary32 columns of test_gpu_precision on nz levels, the second one replaced by the dry column."""
    key = ("in", bool(iiwarm), nz)
    if key not in _shared:
        st = _columns32(nz)
        dry = _to32({k: _edge_columns(nz)[1][k][None] for k in cases.KEYS})
        for k in cases.KEYS:
            st[k][1] = dry[k][0]
        if iiwarm:
            for k in FROZEN:
                st[k][:] = 0.0
        _shared[key] = st
    return _shared[key]


def _two_steps32(m, st, arith):
    """(state, ppt) after one step through the host entry of the binary32 builds, launched twice from the same inputs:
    the second launch's result, once it is known to have the first one's bits."""
    out = []
    for _ in (1, 2):
        got = _copy(st)
        ppt, _, _ = m.batch_step32_host(got, DT, arith=arith)
        out.append((got, ppt))
    for k in OUT:
        assert np.array_equal(_bits(out[0][0][k]), _bits(out[1][0][k])), k
    assert np.array_equal(_bits(out[0][1]), _bits(out[1][1]))
    return out[1]


def _stepped32(m, iiwarm, nz, arith):
    key = (bool(iiwarm), nz, arith)
    if key not in _shared:
        _shared[key] = _two_steps32(m, _full32(iiwarm, nz), arith)
    return _shared[key]


@pytest.mark.gpu
@pytest.mark.parametrize("nz", NZS)
@pytest.mark.parametrize("iiwarm", [False, True], ids=["mixed", "warm"])
def test_p32n_against_the_p32n_oracle(request, iiwarm, nz):
    """Every wave owns a column here: a table read ahead of its fill.  Bounds of test_gpu_precision, unchanged."""
    m = request.getfixturevalue("gpu_warm" if iiwarm else "gpu_mixed")
    o = request.getfixturevalue("oracle_warm" if iiwarm else "oracle_mixed")
    got, gppt = _stepped32(m, iiwarm, nz, "p32n")
    ref = _copy(_full32(iiwarm, nz))
    rppt = o.batch_step_p32n(ref, DT)
    med, q99, q9999, mx = _stats(got, ref)
    pe = float((np.abs(gppt.astype(np.float64) - rppt) / np.maximum(np.abs(rppt), 1e-8)).max())
    print("nz %3d %s p32n gpu vs p32n oracle: median %.1e q99 %.1e q99.99 %.1e max %.1e ppt %.1e"
          % (nz, "warm" if iiwarm else "mixed", med, q99, q9999, mx, pe))
    assert all(np.isfinite(got[k]).all() for k in OUT)
    assert pe < 1e-4, pe
    assert med < 3e-7 and q99 < 1e-4, (med, q99, q9999, mx)


@pytest.mark.gpu
@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nz", NZS)
@pytest.mark.parametrize("arith", ["p32n", "f32"])
@pytest.mark.parametrize("iiwarm", [False, True], ids=["mixed", "warm"])
def test_binary32_columns_keep_their_bits_beside_idle_waves(request, iiwarm, arith, nz, ncol):
    """The first ncol columns alone, launched twice: the bits they have inside the 64-column batch, where no wave is idle."""
    m = request.getfixturevalue("gpu_warm" if iiwarm else "gpu_mixed")
    fgot, fppt = _stepped32(m, iiwarm, nz, arith)
    pgot, pppt = _two_steps32(m, {k: v[:ncol] for k, v in _full32(iiwarm, nz).items()}, arith)
    for k in OUT:
        assert np.array_equal(_bits(pgot[k]), _bits(fgot[k][:ncol])), k
    assert np.array_equal(_bits(pppt), _bits(fppt[:ncol]))
    assert all(np.isfinite(pgot[k]).all() for k in OUT)
    assert fgot["qc"][0].any() or fgot["qr"][0].any()
