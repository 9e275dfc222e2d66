"""tests/parity32.py and the probe build of the P32n oracle, with the oracle alone (no GPU).

  the probe build   shift 0, narrowing off: the bits of the P32n entry on config2(256); elsewhere the two differ only
                    where glibc's binary32 function is not the correctly rounded one -- the measured level difference
                    is asserted as measured (both sides are deterministic CPU code)
  the inputs        every input set of test_gpu_precision32_levels.py has at most parity32.MAX_UNDECIDABLE_FRAC
                    undecidable levels (slow: the mixed-phase oracle's tables), and every set it leaves out has more
  the check bites   a 1 % error of qr at one steady level fails and is named; at an undecidable level it passes and
                    the level is counted as undecidable
"""
import numpy as np
import pytest

import cases
import parity32 as p32
import test_gpu_precision32_levels as L
from oracle.oracle import PROBE_ALTERNATING, PROBE_DOWN, PROBE_UP

# measured: the largest level difference (parity32.level_err32) between the shift-0 probe build and the P32n entry
SHIFT0_SETS = ("fuzz1", "fuzz3", "fuzz11-warm", "edge_cases", "config3", "config5", "config2")
SHIFT0_MAX = 1.1368683772161603e-05           # fuzz3; the issue's sets (400 fuzz columns) gave 5.1e-5


def _bits_equal(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def _step(o, st, dt=L.DT, **kw):
    out = {k: v.copy() for k, v in st.items()}
    return out, o.batch_step_p32n(out, dt, **kw)


def test_probe_build_at_shift_0_has_the_p32n_bits_on_config2(oracle_warm):
    st = L._to32(cases.config2(256))
    a, pa = _step(oracle_warm, st)
    b, pb = _step(oracle_warm, st, probe=(0, PROBE_UP, False))
    assert _bits_equal(a, b) and np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    c, pc = _step(oracle_warm, st, probe=(0, PROBE_ALTERNATING, False))                    # a pattern without a shift is nothing
    assert _bits_equal(a, c)


def test_probe_patterns(oracle_warm):
    """Up and down move the result in different directions, alternating is neither, every pattern is reproducible
    whatever thread steps a column, and the setting does not reach the unmodified entry."""
    st = L.SETS["fuzz11-warm"][1]()
    base, _ = _step(oracle_warm, st)
    n = p32.probe_ulps()
    runs = {pat: _step(oracle_warm, st, probe=(n, pat, False))[0] for pat in p32.PATTERNS}
    for pat, r in runs.items():
        assert not _bits_equal(r, base), pat
        again = _step(oracle_warm, st, probe=(n, pat, False), nthreads=1)[0]
        assert _bits_equal(r, again), pat
    assert not _bits_equal(runs[PROBE_UP], runs[PROBE_DOWN]) and not _bits_equal(runs[PROBE_UP], runs[PROBE_ALTERNATING])
    assert _bits_equal(_step(oracle_warm, st, probe=(-n, PROBE_UP, False))[0], runs[PROBE_DOWN])   # the shift is signed
    assert _bits_equal(_step(oracle_warm, st)[0], base)                                           # the P32n entry is untouched
    narrowed = _step(oracle_warm, st, probe=(0, PROBE_UP, True))[0]
    assert not _bits_equal(narrowed, _step(oracle_warm, st, probe=(0, PROBE_UP, False))[0])
    col = {k: np.ascontiguousarray(v[3].copy()) for k, v in st.items()}                           # the one-column entry
    oracle_warm.column_step_p32n(col, L.DT, probe=(n, PROBE_ALTERNATING, False))
    assert all(np.array_equal(col[k].view(np.uint32), runs[PROBE_ALTERNATING][k][3].view(np.uint32)) for k in p32.OUT)


@pytest.mark.slow
def test_probe_build_at_shift_0_elsewhere(request):
    worst = {}
    for name in SHIFT0_SETS:
        kind, make = {**L.SETS, **L.LEFT_OUT}[name]
        o = request.getfixturevalue("oracle_" + kind)
        st = make()
        a, _ = _step(o, st)
        b, _ = _step(o, st, probe=(0, PROBE_UP, False))
        e = p32.level_err32(b, a)
        worst[name] = float(e.max())
        print("%-12s shift-0 probe against the P32n entry: %.2f %% of the levels differ, max %.3e" % (name, 100 * (e > 0).mean(), e.max()))
    assert max(worst.values()) <= SHIFT0_MAX, worst


# columns held of each set (parity32.held_columns), measured with the oracle alone; all columns where nothing is said
HELD = {"columns64-mixed": 61, "columns65-mixed": 57, "columns120-mixed": 60, "columns129-mixed": 58, "columns200-mixed": 58,
        "edge_cases": 4, "config3": 59, "fuzz11-warm": 25, "aero120": 2,
        "mixed33": 1, "mixed120": 5, "seeded120": 7, "mixed200": 1}


def _conditioning(o, st, dt, what):
    for narrow in (False, True):
        spread = p32.oracle_spread(o, st, dt, narrow=narrow)["spread"]
        assert np.isfinite(spread).all()
        cols = p32.held_columns(spread)
        steady, allowed, und = p32.shares(spread[cols])
        print("%-16s N = %d%s: %d of %d columns held (as drawn: %.2f %% undecidable); of their %d levels steady %.2f %% allowed "
              "%.2f %% undecidable %.2f %%" % (what, p32.probe_ulps(), " narrowed" if narrow else "", len(cols), spread.shape[0],
                                               100 * p32.shares(spread)[2], spread[cols].size, 100 * steady, 100 * allowed, 100 * und))
        p32.assert_well_conditioned(spread[cols], what)
        if not narrow:
            assert len(cols) == HELD.get(what, spread.shape[0]), (what, len(cols))
        assert len(cols) > 0


@pytest.mark.slow
@pytest.mark.parametrize("name", list(L.SETS))
def test_inputs_are_well_conditioned(request, name):
    """The kernel is not an input to this: the P32n oracle alone, its special functions and reciprocals moved by N ulp."""
    kind, make = L.SETS[name]
    _conditioning(request.getfixturevalue("oracle_" + kind), make(), L.DT, name)


@pytest.mark.slow
@pytest.mark.parametrize("b", L.RECORDS)
def test_record_inputs_are_well_conditioned(request, b):
    kind, st, out, _ = L.record_set(b)
    _conditioning(request.getfixturevalue("oracle_" + kind), st, L.RECORD_DT, b)
    assert st["qv"].shape == out["qv"].shape


@pytest.mark.slow
@pytest.mark.parametrize("name", list(L.LEFT_OUT) + ["record " + b for b in L.RECORDS_LEFT_OUT])
def test_left_out_sets_have_no_column_to_hold(request, name):
    """Why test_gpu_precision32_levels.py does not hold these (temporary, while they are out): not one column of them is
    within the cap.  When this fails, move the set to SETS / RECORDS."""
    kind, st = L.record_set(name[7:])[:2] if name.startswith("record ") else (L.LEFT_OUT[name][0], L.LEFT_OUT[name][1]())
    dt = L.RECORD_DT if name.startswith("record ") else L.DT
    spread = p32.oracle_spread(request.getfixturevalue("oracle_" + kind), st, dt)["spread"]
    print("%-18s undecidable %.2f %%" % (name, 100 * p32.shares(spread)[2]))
    assert len(p32.held_columns(spread)) == 0


@pytest.mark.slow
def test_rate_inputs_are_well_conditioned(request):
    """The element rule of test_gpu_rates_shapes.test_p32n_rates_against_the_p32n_oracle."""
    import rates_cases as rc
    for kind, nz in L.RATES_HELD + (("mixed", 120),):
        _, spread = p32.rates_spread32(request.getfixturevalue("oracle_" + kind), rc.to32(rc.batch(kind, nz)), rc.DT)
        und = float((p32.SENS_FACTOR * spread > p32.UNDECIDABLE).mean())
        print("%s rates nz %d: undecidable elements %.3f %%" % (kind, nz, 100 * und))
        assert und <= p32.MAX_UNDECIDABLE_FRAC


# ---- the check bites ----
@pytest.fixture(scope="module")
def warm_fuzz(oracle_warm):
    st = L.SETS["columns120-warm"][1]()
    return st, p32.oracle_spread(oracle_warm, st, L.DT)


def _with_qr_scaled(base, at, factor=1.01):
    got = {k: v.copy() for k, v in base["ref"].items()}
    got["qr"][at] = np.float32(got["qr"][at] * np.float32(factor))
    return got


def test_the_oracle_itself_passes(oracle_warm, warm_fuzz):
    st, base = warm_fuzz
    v = p32.assert_parity32(oracle_warm, st, L.DT, base["ref"], base["ppt_ref"], what="oracle against itself", base=base)
    assert v["worst_ratio"] == 0.0 and v["undecidable"] > 0.0 and v["steady"] > 0.9


def test_one_per_cent_at_a_steady_level_fails_and_is_named(oracle_warm, warm_fuzz):
    st, base = warm_fuzz
    ok = (p32.SENS_FACTOR * base["spread"] <= p32.TOL32) & (base["ref"]["qr"] > 1e-6)
    at = tuple(int(i) for i in np.argwhere(ok)[len(np.argwhere(ok)) // 2])
    got = _with_qr_scaled(base, at)
    with pytest.raises(AssertionError) as exc:
        p32.assert_parity32(oracle_warm, st, L.DT, got, base["ppt_ref"], what="qr x 1.01", base=base)
    assert "(column, level) %s" % (at,) in str(exc.value)
    v = p32.verdict32(p32.compare32(oracle_warm, st, L.DT, got, base=base), got)
    assert v["n_unmatched"] == 1 and v["worst_at"] == at and 0.009 < v["worst_err"] < 0.011


def test_one_per_cent_at_an_undecidable_level_passes_and_is_counted(oracle_warm, warm_fuzz):
    st, base = warm_fuzz
    und = (p32.SENS_FACTOR * base["spread"] > p32.UNDECIDABLE) & (base["ref"]["qr"] > 1e-6)
    assert und.any()
    at = tuple(int(i) for i in np.argwhere(und)[0])
    got = _with_qr_scaled(base, at)
    v = p32.assert_parity32(oracle_warm, st, L.DT, got, base["ppt_ref"], what="qr x 1.01, undecidable", base=base)
    assert v["n_unmatched"] == 0 and 0.009 < v["cmp"]["err"][at] < 0.011
    assert v["undecidable"] * v["n_levels"] == pytest.approx(float((p32.SENS_FACTOR * base["spread"] > p32.UNDECIDABLE).sum()))


def test_a_wrong_latent_heat_is_seen_in_the_temperature(oracle_warm, warm_fuzz):
    """0.05 K at a steady level: invisible to the metric of test_gpu_precision (T over a floor of 1e4), beyond TOL32 here."""
    st, base = warm_fuzz
    at = tuple(int(i) for i in np.argwhere(p32.SENS_FACTOR * base["spread"] <= p32.TOL32)[0])
    got = {k: v.copy() for k, v in base["ref"].items()}
    got["t"][at] += np.float32(0.05)
    v = p32.verdict32(p32.compare32(oracle_warm, st, L.DT, got, base=base), got)
    assert v["n_unmatched"] == 1 and v["worst_at"] == at


def test_f32_rule_holds_the_steady_levels(oracle_warm):
    st = L.SETS["columns64-warm"][1]()
    base = p32.oracle_spread(oracle_warm, st, L.DT, narrow=True)
    p32.assert_f32_near_p32n_oracle(oracle_warm, st, L.DT, base["ref"], base["ppt_ref"], what="oracle", base=base)
    ok = (p32.SENS_FACTOR * base["spread"] < p32.F32_TOL) & (base["ref"]["qr"] > 1e-6)
    at = tuple(int(i) for i in np.argwhere(ok)[0])
    with pytest.raises(AssertionError):
        p32.assert_f32_near_p32n_oracle(oracle_warm, st, L.DT, _with_qr_scaled(base, at), base["ppt_ref"], what="qr x 1.01", base=base)


def test_probe_ulps_comes_from_the_device_bounds():
    from test_gpu_fastmath_edges import DEVICE_ULP32, DIV_ULP32
    assert p32.probe_ulps() == 3 and max(DEVICE_ULP32.values()) > 2.5 and max(DIV_ULP32.values()) == 2.5
