"""The comparison of the 36 rate profiles (save_dg order, oracle.RATE_NAMES) with the oracle: one copy.

The element metric is the one test_gpu_parity.test_rates_match_oracle and test_gpu_goldens._check already use,
|got - ref| / max(|ref|, 1e-9 * max_k |ref[r, :]|): a rate is measured against its own size, but not below 1e-9 of
the largest value its row takes in the column, so that a rate that nearly vanishes at one level is not held to the
rounding of the levels that feed it.  A row the oracle leaves at zero everywhere has no floor at all: anything but
zero there is an infinite error.

As for the state (parity.branch_aware_compare), no element is dropped: where the ORACLE's own rate moves under the
first two ulp-sized input probes of parity._PERT, the element is held to a multiple of that measured response, and
that allowance is bounded in size (parity.ABS_CEILING) and in how many elements may lean on it (MAX_BEYOND_FRAC).
"""
import numpy as np

from parity import _PERT, ABS_CEILING, TOL

NRATES = 36
MAX_BEYOND_FRAC = 1e-3      # at most this share of a test's rate elements beyond TOL at all; tests/test_rates_inputs.py
                            # holds the oracle alone (against its 2-ulp-perturbed self) to the same share beyond 1e-11


def rates_metric(got, ref):
    """[..., 36, nz] -> the element metric, rows floored at 1e-9 of their largest |ref| over the levels."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.maximum(np.max(np.abs(ref), axis=-1, keepdims=True), 1e-300)
    with np.errstate(over="ignore"):                         # anything against an all-zero row: inf, which is the point
        return np.abs(got - ref) / np.maximum(np.abs(ref), 1e-9 * scale)


def oracle_rates(oracle_column_step, st, dt):
    """The oracle's rates [ncol, 36, nz] of one step from the [ncol, nz] batch `st` (left unchanged), and its no_micro
    verdict per column.  oracle_column_step: Oracle.column_step or Oracle.column_step_p32n, bound."""
    ncol, nz = st["qv"].shape
    ref, dry = np.zeros((ncol, NRATES, nz)), np.zeros(ncol, dtype=bool)
    for c in range(ncol):
        col = {k: np.ascontiguousarray(v[c].copy()) for k, v in st.items()}
        _, ref[c], _, dry[c] = oracle_column_step(col, dt, want_rates=True)
    return ref, dry


def rates_compare(oracle_column_step, st, dt, got_rates, nperturb=2, record=None):
    """`got_rates` [ncol, 36, nz] (the HIP result of one step from `st`) against the oracle, column by column.
    Returns a dict of [ncol, 36, nz] arrays:
      err   the element metric of got_rates against the oracle
      sens  the oracle's own response, same metric, to the first `nperturb` probes of parity._PERT (T scaled by
            1 +- 2 eps, the six mixing ratios by 1 -+ 2 eps: the probes of branch_aware_compare)
      ref   the oracle's rates
    and `dry` [ncol]: the oracle's no_micro verdict.  With `record` [ncol, 36, nz] (what the reference Fortran itself
    logged, tests/golden/reference_*.npz) `err` is taken against that record; the oracle supplies only `sens`."""
    got_rates = np.asarray(got_rates)
    ref, dry = oracle_rates(oracle_column_step, st, dt)
    assert got_rates.shape == ref.shape, (got_rates.shape, ref.shape)
    sens = np.zeros_like(ref)
    for ft, fq in _PERT[:nperturb]:
        pert = {k: np.ascontiguousarray(v.copy()) for k, v in st.items()}
        pert["t"] *= ft
        for k in ("qv", "qc", "qi", "qr", "qs", "qg"):
            pert[k] *= fq
        sens = np.maximum(sens, rates_metric(oracle_rates(oracle_column_step, pert, dt)[0], ref))
    target = ref if record is None else np.asarray(record, dtype=np.float64)
    assert target.shape == ref.shape, (target.shape, ref.shape)
    return dict(err=rates_metric(got_rates, target), sens=sens, ref=ref, dry=dry)


def rates_verdict(cmp, tol=TOL, sens_factor=10.0):
    err, sens = cmp["err"], cmp["sens"]
    lim = np.maximum(tol, sens_factor * sens)
    bad = ~(err <= lim)                                      # (a NaN is beyond every bound)
    worst = np.unravel_index(int(np.argmax(np.where(np.isnan(err), np.inf, err))), err.shape) if err.size else ()
    return dict(n_unmatched=int(bad.sum()), n_elements=int(err.size), n_beyond_tol=int((~(err <= tol)).sum()),
                max_err_any=float(np.max(np.where(np.isnan(err), np.inf, err))) if err.size else 0.0,
                max_sens=float(sens.max()) if sens.size else 0.0, n_sensitive=int((sens > 1e-11).sum()),
                worst_at=tuple(int(i) for i in worst), rows_reached=int(np.any(cmp["ref"] != 0, axis=(0, 2)).sum()))


def assert_rates(oracle_column_step, st, dt, got_rates, tol=TOL, sens_factor=10.0, ceiling=ABS_CEILING,
                 max_beyond_frac=MAX_BEYOND_FRAC, record=None):
    """The rate assertion of the -m gpu tests, parity.assert_parity restated for the rate buffer with the project's own
    constants: EVERY element within max(tol, sens_factor x the oracle's own response there), none beyond
    max(tol, ceiling) however the oracle responds, and at most max_beyond_frac of the elements beyond `tol` at all.
    Returns the verdict with the comparison under "cmp"."""
    cmp = rates_compare(oracle_column_step, st, dt, got_rates, record=record)
    v = rates_verdict(cmp, tol=tol, sens_factor=sens_factor)
    assert v["n_unmatched"] == 0, v
    assert v["max_err_any"] <= max(tol, ceiling), v
    assert v["n_beyond_tol"] <= int(np.ceil(max_beyond_frac * v["n_elements"])), v
    v["cmp"] = cmp
    return v
