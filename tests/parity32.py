"""The binary32 counterpart of parity.branch_aware_compare / assert_parity: the p32n and f32 kernels held to the P32n
oracle LEVEL BY LEVEL, with an allowance only where the oracle itself says that the last bits of a special function
decide the level.

Two binary32 implementations agree to rounding amplified by the scheme, and the scheme amplifies without bound at a
few levels (a branch decided by a rounding).  Which levels those are is a property of the reference, and the oracle
alone measures it: its probe build (oracle/thompson_oracle_p32probe.c) evaluates every REAL-argument exp, log, log10,
cbrt and pow, every REAL reciprocal of mp_thompson (odt, orho, ...) and its rate-limiting quotients (a device forms them
with a reciprocal unit) in
binary64, rounds once and moves the result by N ulp -- every call up, every call down, alternating by call.
N = probe_ulps() is the largest bound the device's binary32 functions are held to (test_gpu_fastmath_edges), rounded up.  The spread of a level is the largest distance of a probe run from the unmodified oracle there.

  metric   per level, max over OUT of |x - ref| / max(|ref|, 1e4 x FLOORS[k]); the temperature against FLOORS["t"] = 1 K
           (a binary32 ulp of T is 3e-5 K: a wrong latent-heat branch shows)
  bound    every level within max(TOL32, SENS_FACTOR x spread); a level on a residue-decided test (M:3587, M:3596)
           against the better of its two forced outcomes, all variables at once; precipitation within PPT_TOL
  inputs   a level with SENS_FACTOR x spread > UNDECIDABLE could hide a branch-sized error; an input set may have at
           most MAX_UNDECIDABLE_FRAC such levels (asserted with the oracle alone in tests/test_parity32.py).  The moved
           orho = 1/rho decides what is left of a species that a process removes completely (0, or one ulp of itself, which
           is above R1 in binary32 and carries a number), so mixed-phase sets exceed that share as drawn: held_columns
           re-draws a set to the columns with the fewest undecidable levels that keep it within the cap

Perturbing the INPUTS by binary32 ulps, as parity.py does in binary64, is not the allowance here: 2 ulp of T or qv is
large against the supersaturation and moves 30-45 % of the fuzz levels by more than 1e-4.
"""
import math

import numpy as np

from oracle.oracle import PROBE_ALTERNATING, PROBE_DOWN, PROBE_UP
from parity import FLOORS, OUT

TOL32 = 1e-4                  # the 99th-percentile bound of test_gpu_precision, now a bound on every steady level
F32_TOL = 2e-3                # the f32 build's percentile bound there, made a maximum at steady levels
SENS_FACTOR = 10.0            # parity.verdict's sens_factor
UNDECIDABLE = 1e-2
MAX_UNDECIDABLE_FRAC = 0.03
PPT_TOL, PPT_FLOOR = 1e-4, 1e-8
PATTERNS = (PROBE_UP, PROBE_DOWN, PROBE_ALTERNATING)
FLOORS32 = {k: (FLOORS[k] if k == "t" else 1e4 * FLOORS[k]) for k in OUT}
f32 = np.float32


def probe_ulps():
    """N: the largest bound, rounded up, that test_gpu_fastmath_edges holds the device's binary32 functions to."""
    from test_gpu_fastmath_edges import DEVICE_ULP32, DIV_ULP32
    return int(math.ceil(max(list(DEVICE_ULP32.values()) + list(DIV_ULP32.values()))))


def _copy(st):
    return {k: np.ascontiguousarray(v.copy()) for k, v in st.items()}


def level_err32(got, ref, keys=OUT):
    """[ncol, nz]: max over the variables of |x - ref| / max(|ref|, FLOORS32[k]); a NaN in `got` is an infinite error."""
    e = None
    for k in keys:
        g, r = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        x = np.abs(g - r) / np.maximum(np.abs(r), FLOORS32[k])
        x = np.where(np.isnan(x), np.inf, x)
        e = x if e is None else np.maximum(e, x)
    return e


def element_err32(got, ref, keys=OUT):
    """The same metric element by element, all variables in one vector."""
    return np.concatenate([level_err32(got, ref, (k,)).ravel() for k in keys])


def against_record32(record, ref, keys=OUT):
    """The record, with the oracle's value at the record's NaN entries (U1: output qc and nc at level kts)."""
    return {k: np.where(np.isnan(np.asarray(record[k], dtype=np.float64)), np.asarray(ref[k], dtype=np.float64),
                        np.asarray(record[k], dtype=np.float64)) for k in keys}


def oracle_spread(oracle, st, dt, narrow=False, shift=None):
    """What the oracle alone says about one step from the binary32 batch `st` (left unchanged).  Returns a dict:
      ref, ppt_ref   the unmodified P32n oracle's step
      flags          its residue flags (bit 0: M:3587, bit 1: M:3596)
      forced         None, or the two outcomes (test forced true, forced false) when a level is flagged
      spread         [ncol, nz]: max over the three probe runs (shift ulp; with `narrow` the DOUBLE-argument special
                     functions rounded to binary32 on top) of the level metric between probe run and unmodified run; at
                     levels flagged in the base run or in the probe run, between the two runs forced to one outcome"""
    shift = probe_ulps() if shift is None else shift
    ref = _copy(st)
    ppt_ref, flags = oracle.batch_step_p32n(ref, dt, want_illcond=True)
    forced = None
    if (flags != 0).any():
        forced = []
        for force in (1, 2):
            r = _copy(st)
            oracle.batch_step_p32n(r, dt, force=force)
            forced.append(r)
    spread = np.zeros(flags.shape)
    ref_true = forced[0] if forced else None
    for pattern in PATTERNS:
        probe = (shift, pattern, narrow)
        pr = _copy(st)
        _, pflags = oracle.batch_step_p32n(pr, dt, want_illcond=True, probe=probe)
        s = level_err32(pr, ref)
        both = (flags != 0) | (pflags != 0)
        if both.any():                       # residue-decided levels: like with like, within one forced outcome
            if ref_true is None:             # flagged in a probe run only
                ref_true = _copy(st)
                oracle.batch_step_p32n(ref_true, dt, force=1)
            pt = _copy(st)
            oracle.batch_step_p32n(pt, dt, force=1, probe=probe)
            s = np.where(both, level_err32(pt, ref_true), s)
        spread = np.maximum(spread, s)
    return dict(ref=ref, ppt_ref=ppt_ref, flags=flags, forced=forced, spread=spread)


def compare32(oracle, st, dt, got, got_ppt=None, narrow=False, record=None, record_ppt=None, base=None):
    """Level-by-level comparison of `got` (a kernel's result of one step from `st`) with the P32n oracle; no level is
    left out.  `base`: an oracle_spread of the same inputs computed earlier.  With `record` the error is taken against
    that outside record (the reference Fortran's own native result); the oracle then supplies the spread, the flags and
    the two outcomes, and "record_err" holds the record itself to the two outcomes at flagged levels."""
    cmp = dict(oracle_spread(oracle, st, dt, narrow=narrow) if base is None else base)
    ref, flags, forced = cmp["ref"], cmp["flags"], cmp["forced"]
    target = ref if record is None else against_record32(record, ref)
    err = level_err32(got, target)
    record_err = None if record is None else np.zeros_like(err)
    if forced is not None:
        flagged = flags != 0
        best = np.minimum(level_err32(got, forced[0]), level_err32(got, forced[1]))
        if record is not None:
            best = np.minimum(best, err)
            record_err = np.where(flagged, np.minimum(level_err32(target, forced[0]), level_err32(target, forced[1])), 0.0)
        err = np.where(flagged, best, err)
    ppt_err = None
    if got_ppt is not None:
        pt = np.asarray(cmp["ppt_ref"] if record_ppt is None else record_ppt, dtype=np.float64)
        ppt_err = np.abs(np.asarray(got_ppt, dtype=np.float64) - pt) / np.maximum(np.abs(pt), PPT_FLOOR)
    cmp.update(err=err, target=target, ppt_err=ppt_err, record_err=record_err)
    return cmp


def shares(spread):
    """(steady, allowed, undecidable) shares of the levels: SENS_FACTOR x spread <= TOL32, up to UNDECIDABLE, beyond."""
    s = SENS_FACTOR * spread
    n = max(spread.size, 1)
    und = float((s > UNDECIDABLE).sum()) / n
    steady = float((s <= TOL32).sum()) / n
    return steady, 1.0 - steady - und, und


def held_columns(spread):
    """The columns of an input set that are held level by level: in ascending order of their number of undecidable
    levels (ties in input order), as many as keep the set within MAX_UNDECIDABLE_FRAC; returned sorted.  The oracle alone
    decides: `spread` is oracle_spread's.  A set that is within the cap keeps every column."""
    und = (SENS_FACTOR * spread > UNDECIDABLE).sum(axis=1)
    order = np.argsort(und, kind="stable")
    ok = np.cumsum(und[order]) <= MAX_UNDECIDABLE_FRAC * np.arange(1, len(order) + 1) * spread.shape[1]
    return np.sort(order[:int(np.nonzero(ok)[0].max()) + 1]) if ok.any() else order[:0]


def _restrict(cmp, got, got_ppt, cols):
    sub = dict(cmp)
    for k in ("err", "spread", "flags", "ppt_err", "record_err", "ppt_ref"):
        if sub.get(k) is not None:
            sub[k] = sub[k][cols]
    for k in ("target", "ref"):
        sub[k] = {v: a[cols] for v, a in sub[k].items()}
    return sub, {v: a[cols] for v, a in got.items()}, None if got_ppt is None else got_ppt[cols]


def verdict32(cmp, got=None, tol=TOL32):
    err, spread = cmp["err"], cmp["spread"]
    lim = np.maximum(tol, SENS_FACTOR * spread)
    ratio = err / lim
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    steady, allowed, und = shares(spread)
    v = dict(worst_ratio=float(ratio[w]) if ratio.size else 0.0, worst_at=tuple(int(i) for i in w),
             worst_err=float(err[w]) if ratio.size else 0.0, worst_spread=float(spread[w]) if ratio.size else 0.0,
             n_unmatched=int((~(err <= lim)).sum()), n_levels=int(err.size), n_flagged=int((cmp["flags"] != 0).sum()),
             steady=steady, allowed=allowed, undecidable=und)
    if got is not None:
        e = element_err32(got, cmp["target"])
        v["q9999"], v["max"] = float(np.quantile(e, 0.9999)), float(e.max())
    if cmp.get("ppt_err") is not None:
        v["max_ppt"] = float(cmp["ppt_err"].max())
    return v


def describe(v):
    s = ("worst err / max(TOL32, %g x spread) %.3g at (column, level) %s (err %.2e, spread %.2e); levels: steady %.2f %% "
         "allowed %.2f %% undecidable %.2f %%, %d flagged of %d"
         % (SENS_FACTOR, v["worst_ratio"], v["worst_at"], v["worst_err"], v["worst_spread"], 100 * v["steady"],
            100 * v["allowed"], 100 * v["undecidable"], v["n_flagged"], v["n_levels"]))
    if "q9999" in v:
        s += "; elements: q99.99 %.1e max %.1e" % (v["q9999"], v["max"])
    if "max_ppt" in v:
        s += "; ppt %.1e" % v["max_ppt"]
    return s


def assert_invariants32(got, got_ppt=None):
    """Everything finite, and the invariants of test_binary32_builds_stay_near_the_p64_result."""
    for k in OUT:
        assert np.isfinite(got[k]).all(), k
    assert (got["qv"] >= f32(1e-10)).all()
    for q in ("qc", "qi", "qr", "qs", "qg"):
        assert ((got[q] == 0) | (got[q] > f32(1e-12))).all(), q
    if got_ppt is not None:
        assert np.isfinite(got_ppt).all() and (got_ppt >= 0).all()


def assert_well_conditioned(spread, what=""):
    und = shares(spread)[2]
    assert und <= MAX_UNDECIDABLE_FRAC, (what, "undecidable levels: %.2f %% of %d" % (100 * und, spread.size))


def assert_parity32(oracle, st, dt, got, got_ppt=None, what="", record=None, record_ppt=None, base=None, select=False):
    """The assertion of the -m gpu tests of the p32n kernel.  Prints and returns the verdict.  With `select` the levels
    compared are those of held_columns (the invariants hold for every column); "columns" in the verdict names them."""
    cmp = compare32(oracle, st, dt, got, got_ppt, record=record, record_ppt=record_ppt, base=base)
    assert np.isfinite(cmp["spread"]).all(), (what, "the probe runs are not finite")
    assert_invariants32(got, got_ppt)
    cols = held_columns(cmp["spread"]) if select else np.arange(cmp["spread"].shape[0])
    assert len(cols) > 0, (what, "no column of this set can be held within the cap on undecidable levels")
    if select:
        print(what, "held columns: %d of %d" % (len(cols), cmp["spread"].shape[0]))
        cmp, got, got_ppt = _restrict(cmp, got, got_ppt, cols)
    v = verdict32(cmp, got)
    v["columns"] = cols
    if select and v["worst_at"]:
        v["worst_at"] = (int(cols[v["worst_at"][0]]), v["worst_at"][1])
    print(what, describe(v))
    assert_well_conditioned(cmp["spread"], what)
    if record is not None:                   # the record itself on the residue-decided levels: one of the two outcomes
        assert (cmp["record_err"] <= np.maximum(TOL32, SENS_FACTOR * cmp["spread"])).all(), (what, float(cmp["record_err"].max()))
    assert v["n_unmatched"] == 0, (what, "level (column, level) %s beyond its bound" % (v["worst_at"],), v)
    if got_ppt is not None:
        assert v["max_ppt"] < PPT_TOL, (what, v)
    v["cmp"] = cmp
    return v


def assert_f32_near_p32n_oracle(oracle, st, dt, got, got_ppt=None, what="", base=None, select=False):
    """The all-binary32 build against the P32n oracle: the spread taken with the narrowing mode on; every level whose
    SENS_FACTOR x spread is below F32_TOL lies within F32_TOL.  Prints the distribution of err / spread.  `select`: as in
    assert_parity32."""
    cmp = compare32(oracle, st, dt, got, got_ppt, narrow=True, base=base)
    assert np.isfinite(cmp["spread"]).all(), (what, "the probe runs are not finite")
    assert_invariants32(got, got_ppt)
    if select:
        cols = held_columns(cmp["spread"])
        assert len(cols) > 0, (what, "no column of this set can be held within the cap on undecidable levels")
        print(what, "held columns: %d of %d" % (len(cols), cmp["spread"].shape[0]))
        cmp, got, got_ppt = _restrict(cmp, got, got_ppt, cols)
    else:
        cols = np.arange(cmp["spread"].shape[0])
    err, spread = cmp["err"], cmp["spread"]
    held = SENS_FACTOR * spread < F32_TOL
    r = err[spread > 0] / spread[spread > 0]
    q = [float(np.quantile(r, x)) for x in (0.5, 0.9, 0.99, 1.0)] if r.size else [0.0] * 4
    worst = np.unravel_index(int(np.argmax(np.where(held, err, -1.0))), err.shape)
    at = (int(cols[worst[0]]), int(worst[1]))
    e = element_err32(got, cmp["target"])
    print(what, "f32 vs P32n oracle: held levels %d of %d, worst held err %.2e at (column, level) %s (spread %.2e); err / spread "
          "where spread > 0 (%d levels): median %.2g q90 %.2g q99 %.2g max %.2g; levels with spread 0: max err %.2e; elements: "
          "q99.99 %.1e max %.1e" % (held.sum(), held.size, err[worst], at, spread[worst], r.size, *q,
                                    float(err[spread == 0].max()) if (spread == 0).any() else 0.0,
                                    float(np.quantile(e, 0.9999)), float(e.max())))
    assert_invariants32(got, got_ppt)
    bad = held & ~(err <= F32_TOL)
    assert not bad.any(), (what, "level (column, level) %s" % (at,), float(err[worst]), float(spread[worst]))
    return cmp


# ---- the rate buffer: the same rule element by element ----
def rates_spread32(oracle, st, dt, shift=None):
    """(the P32n oracle's rates [ncol, 36, nz], their spread under the three probe runs in rates_parity.rates_metric)."""
    from functools import partial

    from rates_parity import oracle_rates, rates_metric
    shift = probe_ulps() if shift is None else shift
    ref = oracle_rates(oracle.column_step_p32n, st, dt)[0]
    spread = np.zeros_like(ref)
    for pattern in PATTERNS:
        pr = oracle_rates(partial(oracle.column_step_p32n, probe=(shift, pattern, False)), st, dt)[0]
        with np.errstate(invalid="ignore"):
            s = rates_metric(pr, ref)
        spread = np.maximum(spread, np.where(np.isnan(s), 0.0, s))
    return ref, spread


def assert_rates32(oracle, st, dt, rates, bound, what=""):
    """Every element of `rates` within max(bound, SENS_FACTOR x the probe's spread of that rate) of the P32n oracle's."""
    from rates_parity import rates_metric
    ref, spread = rates_spread32(oracle, st, dt)
    assert np.isfinite(spread).all(), (what, "the probe runs are not finite")
    err = rates_metric(rates, ref)
    err = np.where(np.isnan(err), np.inf, err)
    lim = np.maximum(bound, SENS_FACTOR * spread)
    ratio = err / lim
    w = tuple(int(i) for i in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    und = float((SENS_FACTOR * spread > UNDECIDABLE).mean())
    print(what, "rates: worst err / max(%g, %g x spread) %.3g at (column, row, level) %s: got %.6e oracle %.6e spread %.2e; "
          "elements beyond the plain bound %d, undecidable %.3f %% of %d"
          % (bound, SENS_FACTOR, ratio[w], w, rates[w], ref[w], spread[w], int((err > bound).sum()), 100 * und, err.size))
    assert und <= MAX_UNDECIDABLE_FRAC, (what, und)
    assert (err <= lim).all(), (what, "element (column, row, level) %s" % (w,), float(err[w]), float(spread[w]))
