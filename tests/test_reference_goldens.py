"""The CPU oracle against what the reference Fortran itself computed (tests/golden/reference_*.npz, recorded by
tests/golden/make_reference_goldens.py from the reference built from source with flang, see oracle/Makefile `ref`).

P64 (oracle/_ref/p64: -O2 -fdefault-real-8 -fdefault-double-8 -ffp-contract=off).  The bound of each family is four
times the largest relative difference MEASURED when the fixtures were recorded (metric and floors of tests/parity.py and
tests/rates_parity.py; the margin is for another host's libm); a family that measured bit-equal is held to four ulps
(4 * 2^-52 = 8.9e-16), since a bound of zero would make one rounding of another libm a failure.  Measured:

    state  (12 profiles, 36 columns of 33 / 120 / 200 levels, warm, mixed and aerosol-aware)   7.4e-13  (nr; qr 7.1e-13)
    ppt                                                                                         4.7e-16
    rates  (36 rows, two warm and four mixed columns)                                           4.9e-14
    calc_effectRad (re_qc, re_qi, re_qs, on the input and on the stepped state)                 0  (bit-equal)
    calc_refl10cm  (tests/refl_oracle.py, absolute, dB)                                         2.2e-14
    tables (512 sampled elements of each of the 30, and their sums)                             1.2e-15 (sums 1.9e-16)
    constants (the 16 the reference module leaves PUBLIC)                                       0  (bit-equal)
    adapter tendencies (nx = 3, warm and mixed; metric of test_gpu_kid_adapter)                 4.0e-13 (nr)

Nothing measured above 1e-12, so the oracle's expression order is the Fortran's wherever these columns reach.

At the 113 levels (of 4 299) on the two residue-decided tests (M:3587, M:3596) the RECORD must equal one of the oracle's
two forced outcomes, all variables of the level at once (parity.branch_aware_compare with the record as `got`): measured
7.1e-13, within the state figure; at one level the Fortran took the outcome the unforced oracle did not.  The U1 entries (output qc and nc at kts, NaN in the fixtures) have no reference value:
there the oracle must return its no-sedimentation value.

P32n (oracle/_ref/native: -O2 -ffp-contract=off, the 4-byte REAL KiD is built with): the figures stand with the native
tests below.

The GPU entries meet the same records in tests/test_gpu_reference.py.
"""
import os

import numpy as np
import pytest

import cases
import refl_oracle as ro
import reference_record as rr
from parity import FLOORS, MAX_SENSITIVE_FRAC, OUT, against_record, branch_aware_compare, level_err, rel_err
from rates_parity import MAX_BEYOND_FRAC, rates_compare, rates_metric

ULP4 = 4 * 2.0 ** -52
DT = 10.0
BATCHES = ("warm120", "mixed120", "seeded120", "mixed33", "mixed200", "aero120")
# four times the figures of the docstring
BOUND = dict(state=4 * 7.4e-13, ppt=4 * 4.7e-16, rates=4 * 4.9e-14, radii=ULP4, dbz=4 * 2.2e-14, tables=4 * 1.2e-15, consts=ULP4,
             adapter=4 * 4.0e-13)


def _records(tree):
    rec = {}
    for suffix in ("", "_seeded", "_more"):
        rec.update(rr.load("reference_%s%s.npz" % (tree, suffix)))
    return rec


@pytest.fixture(scope="module")
def p64():
    return _records("p64")


@pytest.fixture(scope="module")
def native():
    return _records("native")


def _oracle_for(rec, b, oracle_warm, oracle_mixed, oracle_mixed_aero):
    return oracle_warm if rec[b + ".iiwarm"] else (oracle_mixed_aero if rec[b + ".aero"] else oracle_mixed)


def _inputs(rec, b, dtype=np.float64):
    return {k: np.ascontiguousarray(rec["%s.in.%s" % (b, k)].astype(dtype)) for k in cases.KEYS}


def _outputs(rec, b):
    return {k: rec["%s.out.%s" % (b, k)].astype(np.float64) for k in OUT}


def test_fixtures_hold_what_the_issue_lists(p64, native):
    for rec, real in ((p64, np.float64), (native, np.float32)):
        assert [rec[b + ".in.qv"].shape for b in BATCHES] == [(3, 120), (9, 120), (12, 120), (3, 33), (3, 200), (6, 120)]
        for b in BATCHES:
            out = _outputs(rec, b)
            assert rec[b + ".out.t"].dtype == real and rec[b + ".in.t"].dtype == real
            for k in OUT:                                    # NaN at the U1 entries and nowhere else
                nan = np.isnan(out[k])
                assert nan[:, 0].all() and not nan[:, 1:].any() if k in ("qc", "nc") else not nan.any(), (b, k)
            assert (rec[b + ".in.t"][:, 0] >= 235.16).all()  # block Q cannot carry the undefined qc(kts) into qi, ni, t
            assert np.isfinite(rec[b + ".ppt"]).all() and np.isfinite(rec[b + ".dbz"]).all()
            assert np.isnan(rec[b + ".re_qc"][:, 0]).all() and np.isfinite(rec[b + ".re_qc"][:, 1:]).all()
        assert (p64["aero120.in.w"] == 2.0).all() and bool(p64["aero120.aero"])
        assert rec["warm120.rates"].shape == (2, 36, 120) and rec["mixed120.rates"].shape == (2, 36, 120)
        assert rec["seeded120.rates"].shape == (2, 36, 120)
    for f in os.listdir(rr.GOLDEN):
        if f.startswith("reference_"):
            assert os.path.getsize(os.path.join(rr.GOLDEN, f)) < 256 * 1024, f


@pytest.mark.slow
@pytest.mark.parametrize("b", BATCHES)
def test_oracle_p64_state_and_ppt_match_the_reference(b, p64, oracle_warm, oracle_mixed, oracle_mixed_aero):
    """The RECORD is what is compared (its U1 entries filled with the oracle's values): against the oracle's step at
    every level, and at a level on a residue-decided test against the better of the oracle's two forced outcomes, all
    variables of the level at once -- the Fortran may have taken either."""
    o = _oracle_for(p64, b, oracle_warm, oracle_mixed, oracle_mixed_aero)
    st = _inputs(p64, b)
    step = {k: v.copy() for k, v in st.items()}
    o.batch_step(step, DT)
    rec = against_record(_outputs(p64, b), step)
    cmp = branch_aware_compare(o, st, DT, rec, p64[b + ".ppt"])
    flagged = cmp["flags"] != 0
    print("%-9s reference vs oracle P64: state %.2e; at the %d flagged levels %.2e (%d of them on the outcome the "
          "unforced oracle did not take); ppt %.2e"
          % (b, cmp["err"].max(), int(flagged.sum()), cmp["err"][flagged].max() if flagged.any() else 0.0,
             int((level_err(rec, step)[flagged] > BOUND["state"]).sum()), cmp["ppt_err"].max()))
    assert cmp["err"].max() <= BOUND["state"], float(cmp["err"].max())
    assert cmp["ppt_err"].max() <= BOUND["ppt"], float(cmp["ppt_err"].max())
    for k in OUT:                            # outside the flagged levels, variable by variable
        e = np.where(flagged, 0.0, rel_err(rec[k], step[k], FLOORS[k]))
        assert e.max() <= BOUND["state"], (b, k, float(e.max()))


@pytest.mark.slow
@pytest.mark.parametrize("b", BATCHES)
def test_oracle_u1_entries_are_the_no_sedimentation_value(b, p64, oracle_warm, oracle_mixed, oracle_mixed_aero):
    """qc and nc at kts, which the reference leaves undefined (NaN in the fixture): the oracle's "cloud water does not
    sediment" makes them what a run without any sedimentation gives there, bit for bit."""
    from oracle.oracle import Oracle
    o = _oracle_for(p64, b, oracle_warm, oracle_mixed, oracle_mixed_aero)
    nosed = Oracle(iiwarm=bool(p64[b + ".iiwarm"]), l_sediment=False, aerosol_aware=bool(p64[b + ".aero"]))
    try:
        a, c = _inputs(p64, b), _inputs(p64, b)
        o.batch_step(a, DT)
        nosed.batch_step(c, DT)
        for k in ("qc", "nc"):
            assert np.isnan(p64["%s.out.%s" % (b, k)][:, 0]).all()
            assert np.array_equal(a[k][:, 0], c[k][:, 0]), (b, k)
    finally:
        nosed.close()


@pytest.mark.slow
@pytest.mark.parametrize("b", ["warm120", "mixed120", "seeded120"])
def test_oracle_p64_rates_match_the_reference(b, p64, oracle_warm, oracle_mixed, oracle_mixed_aero):
    o = _oracle_for(p64, b, oracle_warm, oracle_mixed, oracle_mixed_aero)
    cols = p64[b + ".rate_cols"]
    st = {k: np.ascontiguousarray(v[cols]) for k, v in _inputs(p64, b).items()}
    worst = 0.0
    for j in range(len(cols)):
        col = {k: np.ascontiguousarray(v[j].copy()) for k, v in st.items()}
        _, r, _, _ = o.column_step(col, DT, want_rates=True)
        ref = p64[b + ".rates"][j]
        assert np.array_equal(np.any(r != 0, axis=1), np.any(ref != 0, axis=1)), (b, j)      # the same rows are reached
        worst = max(worst, float(rates_metric(r, ref).max()))
    print("%-9s oracle P64 rates vs reference: %.2e" % (b, worst))
    assert worst <= BOUND["rates"], worst
    if b == "warm120":
        assert not p64[b + ".rates"][:, :30].any() and p64[b + ".rates"][:, 30:].any()


@pytest.mark.slow
@pytest.mark.parametrize("b", BATCHES)
def test_oracle_diagnostics_match_the_reference(b, p64, oracle_warm, oracle_mixed, oracle_mixed_aero):
    """calc_effectRad (the C oracle) and calc_refl10cm (tests/refl_oracle.py) on the input state and on the state the
    reference stepped to (its U1 entries filled with the oracle's values; re_qc is not compared at kts there)."""
    o = _oracle_for(p64, b, oracle_warm, oracle_mixed, oracle_mixed_aero)
    c = ro.constants(o)
    st = _inputs(p64, b)
    stepped = {k: v.copy() for k, v in st.items()}
    o.batch_step(stepped, DT)
    stepped.update(against_record(_outputs(p64, b), stepped))
    worst_r, worst_d = 0.0, 0.0
    for state, sfx in ((st, "_in"), (stepped, "")):
        for g, n in zip(o.calc_effectRad(state), ("re_qc", "re_qi", "re_qs")):
            r = p64["%s.%s%s" % (b, n, sfx)]
            e = np.abs(g - r) / r
            worst_r = max(worst_r, float(np.nanmax(e)))
            assert np.isnan(e).sum() == (r.shape[0] if (n, sfx) == ("re_qc", "") else 0)
        worst_d = max(worst_d, float(np.abs(ro.of_state(c, state) - p64["%s.dbz%s" % (b, sfx)]).max()))
    print("%-9s oracle diagnostics vs reference: radii %.2e, dBZ %.2e dB" % (b, worst_r, worst_d))
    assert worst_r <= BOUND["radii"], worst_r
    assert worst_d <= BOUND["dbz"], worst_d


@pytest.mark.slow
def test_oracle_tables_and_constants_match_the_reference(oracle_mixed):
    """Every table of kidmp_tables.hip::table_dir (planar names) at the 512 sampled elements, with the element metric of
    test_gpu_parity.test_table_matches_oracle, its shape, its sum and its sum of absolute values (relative to the latter);
    the constants the reference module leaves PUBLIC (the others are PRIVATE there: they are held through the tables
    and the rates they feed)."""
    T = rr.load("reference_tables.npz")
    worst, worst_sum = 0.0, 0.0
    for n in rr.TABLES:
        t = oracle_mixed.table(n)
        assert t.shape == tuple(T[n + ".shape"]), n
        flat, v = t.ravel(order="F"), T[n + ".val"]
        assert len(v) == min(512, flat.size) and np.isfinite(v).all()
        e = np.abs(flat[T[n + ".idx"]] - v) / np.maximum(np.abs(v), 1e-30 + 1e-13 * np.max(np.abs(flat)))
        worst = max(worst, float(e.max()))
        for got, ref in ((flat.sum(), T[n + ".sum"]), (np.abs(flat).sum(), T[n + ".sumabs"])):
            worst_sum = max(worst_sum, abs(got - float(ref)) / max(float(T[n + ".sumabs"]), 1e-300))
    wc = max(abs(oracle_mixed.const(n)[0] / float(T["const." + n]) - 1.0) for n in rr.CONSTS)
    print("oracle tables vs reference: elements %.2e, sums %.2e; constants %.2e" % (worst, worst_sum, wc))
    assert worst <= BOUND["tables"] and worst_sum <= BOUND["tables"], (worst, worst_sum)
    assert wc <= BOUND["consts"], wc


HYD = (("qc", 0, 0), ("qr", 1, 0), ("nr", 1, 1), ("qi", 2, 0), ("ni", 2, 1), ("qs", 3, 0), ("qg", 4, 0))   # KiD species, moment


def adapter_case(A, tag):
    """(nz, nx, dt, p0, r_on_cp, inputs, recorded tendencies by field [nx, nz]) of reference_adapter.npz."""
    nz, nx = int(A[tag + ".nz"]), int(A[tag + ".nx"])
    hy = A[tag + ".in.hydro"].reshape(2, 5, nx, nz)
    F = {"theta": A[tag + ".in.theta"].reshape(nx, nz), "qv": A[tag + ".in.qv"].reshape(nx, nz)}
    F.update({k: np.ascontiguousarray(hy[im, ih]) for k, ih, im in HYD})
    dhy = A[tag + ".dhy"].reshape(2, 5, nx, nz)
    want = {"theta": A[tag + ".dth"].reshape(nx, nz), "qv": A[tag + ".dqv"].reshape(nx, nz)}
    want.update({k: dhy[im, ih] for k, ih, im in HYD})
    return nz, nx, float(A[tag + ".dt"]), float(A[tag + ".p0"]), float(A[tag + ".r_on_cp"]), F, want


def adapter_error(F, got, want, keys):
    """The metric of test_gpu_kid_adapter.test_warm_tendencies_match_the_oracle_adapter per field; the U1 entries (the
    tendency of qc at kts, NaN in the record) are left out and counted."""
    worst, nan = {}, 0
    for k in keys:
        scale = max(np.abs(F[k]).max() / 10.0, 1e-300)
        err = np.abs(got[k] - want[k]) / np.maximum(np.abs(want[k]), 1e-5 * scale)
        nan += int(np.isnan(want[k]).sum())
        worst[k] = float(np.nanmax(err))
    return worst, nan


def adapter_logged_rates(A, tag, nz, nx):
    """[nx, 36, nz]: the rates the adapter call logged through save_dg (form 'ki'); a row the call did not log stays 0."""
    from oracle.oracle import RATE_NAMES
    names = A[tag + ".log_names"][A[tag + ".log_name"]]
    out = np.zeros((nx, len(RATE_NAMES), nz))
    for j, n in enumerate(RATE_NAMES):
        sel = names == n
        out[A[tag + ".log_i"][sel] - 1, j, A[tag + ".log_k"][sel] - 1] = A[tag + ".log_v"][sel]
    return out


def expected_log(iiwarm, nz, nx):
    """The save_dg calls of one adapter call with nx > 1, in order: (form, name, k, i)."""
    from oracle.oracle import RATE_NAMES
    names = RATE_NAMES[30:] if iiwarm else RATE_NAMES
    log = [("ki", n, k, i) for i in range(1, nx + 1) for k in range(1, nz + 1) for n in names]            # M:3043-3118
    ppt = ["surface_ppt_for_" + h for h in ("rain", "ice", "snow", "graupel")] + ["total_surface_ppt"]
    return log + 2 * [("array", n, 0, i) for n in ppt for i in range(1, nx + 1)]                          # W:248-303


@pytest.mark.slow
@pytest.mark.parametrize("tag", ["warm", "mixed"])
def test_oracle_adapter_matches_the_reference(tag, oracle_warm, oracle_mixed):
    A = rr.load("reference_adapter.npz")
    o = oracle_warm if tag == "warm" else oracle_mixed
    nz, nx, dt, p0, r_on_cp, F, want = adapter_case(A, tag)
    z, zh = np.zeros(nz * nx), np.zeros(nz * nx * 10)
    dth, dqv, dhy, ppt = o.kid_interface(nz, nx, dt, p0, r_on_cp, A[tag + ".in.theta"], z, z, A[tag + ".in.exner"],
                                         A[tag + ".in.dz"], A[tag + ".in.qv"], z, z, A[tag + ".in.hydro"], zh, zh)
    got = {"theta": dth.reshape(nx, nz), "qv": dqv.reshape(nx, nz)}
    got.update({k: dhy.reshape(2, 5, nx, nz)[im, ih] for k, ih, im in HYD})
    keys = ("theta", "qv", "qc", "qr", "nr") + (() if tag == "warm" else ("qi", "ni", "qs", "qg"))
    worst, nan = adapter_error(F, got, want, keys)
    print(tag, "oracle adapter vs reference:", worst)
    assert nan == nx and np.isnan(want["qc"][:, 0]).all()
    assert max(worst.values()) <= BOUND["adapter"], worst
    assert all(np.abs(want[k]).max() > 0 for k in keys if k != "qc") and np.nanmax(np.abs(want["qc"])) > 0
    # the save_dg log: names, forms, indices and order; the precipitation entries against the oracle's
    names, forms = A[tag + ".log_names"], A[tag + ".log_forms"]
    log = list(zip(forms[A[tag + ".log_form"]], names[A[tag + ".log_name"]], A[tag + ".log_k"], A[tag + ".log_i"]))
    assert [(str(f), str(n), int(k), int(i)) for f, n, k, i in log] == expected_log(tag == "warm", nz, nx)
    v = A[tag + ".log_v"][-10 * nx:].reshape(2, 5, nx)
    rain, snow, graupel, ice = ppt
    for j, p in enumerate((rain, ice, snow, graupel, rain + ice + snow + graupel)):
        assert np.abs(v[0, j] * nx - p).max() <= BOUND["ppt"] * max(np.abs(p).max(), 1e-12)          # the means, W:255-275
        assert np.abs(v[1, j] - p).max() <= BOUND["ppt"] * max(np.abs(p).max(), 1e-12)


# ---- P32n: the oracle in the reference's native arithmetic against the native tree's record ----
# Measured when the fixtures were recorded (metric of test_gpu_precision._err: floors 1e-8 kg/kg, 1e-2 /kg):
#   warm120 (KAT-A warm, KAT-B step 1, config 2): most levels bit-equal, the worst 3.0e-7 (two ulps of binary32)
#   every batch: median 0, 99th percentile at most 1.2e-5 (mixed200), ppt at most 1.2e-6
#   KAT-B step 1, sums of qv, qc, qr, nr: 0, 1.3e-9, 2.9e-9, 4.0e-9;  KAT-A mixed, sum of qi: 8.6e-7
# All below today's bounds against the survey's digits (5e-7 on KAT-B, 4e-5 on KAT-A mixed), so 4 x the measurement is
# asserted; the median, measured 0, is held to one rounding of binary32 (2^-24).
P32N = dict(warm_max=4 * 3.0e-7, median=2.0 ** -24, q99=4 * 1.2e-5, ppt=4 * 1.2e-6, kat_b_sums=4 * 4.0e-9, kat_a_qi=4 * 8.6e-7)


def p32n_errors(got, rec, b):
    """The level errors of test_gpu_precision._stats over the 12 profiles, the U1 entries (NaN) left out."""
    es = []
    for k in OUT:
        r = rec["%s.out.%s" % (b, k)].astype(np.float64)
        e = np.abs(got[k].astype(np.float64) - r) / np.maximum(np.abs(r), 1e4 * FLOORS[k])
        es.append(e[~np.isnan(r)])
    return np.concatenate(es)


@pytest.mark.slow
@pytest.mark.parametrize("b", BATCHES)
def test_oracle_p32n_matches_the_native_reference(b, native, oracle_warm, oracle_mixed, oracle_mixed_aero):
    o = _oracle_for(native, b, oracle_warm, oracle_mixed, oracle_mixed_aero)
    st = _inputs(native, b, np.float32)
    ppt = o.batch_step_p32n(st, DT)
    e = p32n_errors(st, native, b)
    rp = native[b + ".ppt"].astype(np.float64)
    pe = float((np.abs(ppt.astype(np.float64) - rp) / np.maximum(np.abs(rp), 1e-8)).max())
    print("%-9s oracle P32n vs native reference: median %.1e q99 %.1e max %.1e ppt %.1e"
          % (b, np.median(e), np.quantile(e, 0.99), e.max(), pe))
    assert np.median(e) <= P32N["median"] and np.quantile(e, 0.99) <= P32N["q99"], (np.median(e), np.quantile(e, 0.99))
    assert pe <= P32N["ppt"], pe
    sums = lambda c, k: (float(st[k][c, 1:].astype(np.float64).sum()),                                    # noqa: E731
                         float(native["%s.out.%s" % (b, k)][c, 1:].astype(np.float64).sum()))
    if b == "warm120":
        assert e.max() <= P32N["warm_max"], float(e.max())
        for k in ("qv", "qc", "qr", "nr"):                   # KAT-B step 1 (column 1), the sums the survey quotes
            g, r = sums(1, k)
            assert abs(g / r - 1.0) <= P32N["kat_b_sums"], (k, g, r)
    if b == "mixed120":
        g, r = sums(0, "qi")                                 # KAT-A mixed (column 0)
        assert abs(g / r - 1.0) <= P32N["kat_a_qi"], (g, r)


# ---- the fixtures themselves ----
@pytest.mark.slow
@pytest.mark.parametrize("b", BATCHES)
def test_fixture_inputs_are_well_conditioned(b, p64, oracle_warm, oracle_mixed, oracle_mixed_aero):
    """The oracle alone (the pattern of test_gpu_table_fill.test_inputs_are_well_conditioned): the columns leave no more
    than parity.MAX_SENSITIVE_FRAC of a batch's levels, and rates_parity.MAX_BEYOND_FRAC of its rate elements, to the
    sensitivity allowance, so a pass of tests/test_gpu_reference.py is a pass on the levels themselves."""
    o = _oracle_for(p64, b, oracle_warm, oracle_mixed, oracle_mixed_aero)
    st = _inputs(p64, b)
    ref = {k: v.copy() for k, v in st.items()}
    o.batch_step(ref, DT)
    cmp = branch_aware_compare(o, st, DT, ref)
    n_sens = int((cmp["sens"] > 1e-11).sum())
    print(b, "sensitive levels", n_sens, "of", cmp["sens"].size, "branch levels", int((cmp["flags"] != 0).sum()))
    assert n_sens <= int(np.ceil(MAX_SENSITIVE_FRAC * cmp["sens"].size)), (b, n_sens)
    if b + ".rates" in p64:
        cols = p64[b + ".rate_cols"]
        sub = {k: np.ascontiguousarray(v[cols]) for k, v in st.items()}
        sens = rates_compare(o.column_step, sub, DT, p64[b + ".rates"])["sens"]
        print(b, "sensitive rate elements", int((sens > 1e-11).sum()), "of", sens.size)
        assert (sens > 1e-11).sum() <= int(np.ceil(MAX_BEYOND_FRAC * sens.size)), (b, int((sens > 1e-11).sum()))


@pytest.mark.slow
@pytest.mark.skipif(not all(rr.have_driver(t) for t in rr.TREES), reason="oracle/_ref/*/ref_driver is not built")
def test_fixtures_are_what_the_reference_computes_today():
    """Re-runs the reference on the committed inputs: the committed outputs, bit for bit, outside the U1 entries -- the
    step records of both trees, and the P64 tree's tables, constants and adapter calls.  The first mixed-phase run
    of a tree builds the reference's own collection tables, a minute and a half, alone in its tree (reference_record._run);
    every other process runs side by side with it or after it and reuses them."""
    from concurrent.futures import ThreadPoolExecutor
    recs = {tree: _records(tree) for tree in rr.TREES}

    def job(tree, iiwarm):
        rec = recs[tree]
        names = [b for b in BATCHES if bool(rec[b + ".iiwarm"]) == iiwarm]
        blocks = [({k: rec["%s.in.%s" % (b, k)] for k in cases.KEYS}, bool(rec[b + ".aero"])) for b in names]
        return tree, names, rr.run_step(tree, iiwarm, blocks, float(rec["dt"]))

    A, T = rr.load("reference_adapter.npz"), rr.load("reference_tables.npz")

    def adapter_job(tag):
        c = {k: A["%s.in.%s" % (tag, k)] for k in ("theta", "exner", "dz", "qv", "hydro")}
        c.update({k: float(A["%s.%s" % (tag, k)]) for k in ("dt", "p0", "r_on_cp")})
        c.update(nz=int(A[tag + ".nz"]), nx=int(A[tag + ".nx"]))
        return rr.run_adapter("p64", tag == "warm", c)

    with ThreadPoolExecutor(7) as pool:
        steps = pool.map(lambda a: job(*a), [(t, w) for t in rr.TREES for w in (True, False)])
        adapters = pool.map(adapter_job, ("warm", "mixed"))
        tabs, consts = pool.submit(rr.run_tables, "p64").result()
        done, adapters = list(steps), dict(zip(("warm", "mixed"), adapters))
    for name in rr.TABLES:
        flat = tabs[name].ravel(order="F")
        assert tabs[name].shape == tuple(T[name + ".shape"]), name
        assert np.array_equal(flat[T[name + ".idx"]].view(np.uint64), T[name + ".val"].view(np.uint64)), name
        assert flat.sum() == T[name + ".sum"] and np.abs(flat).sum() == T[name + ".sumabs"], name
    assert all(consts[n] == float(T["const." + n]) for n in rr.CONSTS)
    for tag, (dth, dqv, dhy, log) in adapters.items():
        for got, key in ((dth, ".dth"), (dqv, ".dqv"), (dhy, ".dhy")):
            keep = ~np.isnan(A[tag + key])                   # the U1 tendency: qc at kts
            assert np.array_equal(got[keep].view(np.uint64), A[tag + key][keep].view(np.uint64)), (tag, key)
        log = [e for e in log if e[1] != "total_ppt_level"]  # written from an array nothing assigns (W:32, W:307)
        names, forms = A[tag + ".log_names"], A[tag + ".log_forms"]
        assert [e[1] for e in log] == names[A[tag + ".log_name"]].tolist(), tag
        assert [e[0] for e in log] == forms[A[tag + ".log_form"]].tolist(), tag
        assert [e[2] for e in log] == A[tag + ".log_k"].tolist() and [e[3] for e in log] == A[tag + ".log_i"].tolist(), tag
        assert np.array_equal(np.array([e[4] for e in log]).view(np.uint64), A[tag + ".log_v"].view(np.uint64)), tag
    for tree, names, results in done:
        rec = recs[tree]
        for b, res in zip(names, results):
            for k in OUT + ("ppt",) + tuple(d + s for d in rr.DIAG for s in ("", "_in")):
                want = rec["%s.out.%s" % (b, k)] if k in OUT else rec["%s.%s" % (b, k)]
                keep = ~np.isnan(want)
                got = res[k].astype(want.dtype)
                assert np.array_equal(got[keep].view(np.uint8), want[keep].view(np.uint8)), (tree, b, k)
            if b + ".rates" in rec:
                got = res["rates"][rec[b + ".rate_cols"]]
                assert np.array_equal(got.view(np.uint64), rec[b + ".rates"].view(np.uint64)), (tree, b)
