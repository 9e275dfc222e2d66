"""The size-limit tests that the binary64 column kernel decides without the cube root (kid_amd/csrc/limit_bracket.h):
block B's ice test and block J's cloud-droplet, ice and rain tests.

(a) the probe   kidmp_math_probe_ex(KIDMP_MATH_LIMIT_BRACKET) evaluates, for pairs (num, den), the bracket and the kernel's
                original expression c / root3(num / den) on the device.  Wherever the bracket is certain the two agree --
                on pairs 0, +-1, +-2, +-8, +-64, +-4096 ulp around both exact thresholds of every site (limit_bracket_cases.py)
                and on log-uniform pairs; the device's bracket answers are those of the host build of the header, and
                ambiguity occurs only among the threshold-adjacent pairs.
(b) end to end  columns whose ice, cloud water and rain are set, level by level in turn, to land inside, beyond the lower and
                beyond the upper limit of each test, so that one wave holds every outcome in neighbouring lanes.  What
                block J's tests see AFTER the step's tendencies is derived from the oracle's own process rates
                (_post_tendency_regimes) and asserted on the CPU: each of the three tests meets all three outcomes within
                four neighbouring levels, in both contexts and at every nz >= 64 (at nz = 2: over the columns).  The contexts
                run at Nt_c = 0.3 cm-3: at conftest's 100 cm-3 the droplet test's upper limit takes 35 g/kg of cloud water,
                which autoconversion removes within the step, so that outcome would never be met.  The fifth column is
                set inside every limit at every level (and stays there after the tendencies at over 90 % of its levels):
                alone in its workgroup, its waves skip the sites; the waves of the other
                four nearly always hold a lane beyond a limit and run the original code -- the skip path is otherwise
                exercised by the whole existing suite, whose states are inside the limits.
                Every level-group count (NJ = 1, 2, 3), the one-column-per-workgroup layout above 120 levels, a single
                column and a workgroup with a remainder; mixed-phase and warm-rain kernels.  HIP path against the oracle
                through parity.assert_parity at its own bounds.  The inputs are chosen with the oracle alone
                (test_inputs_*, test_block_j_*: no GPU)."""
import functools

import numpy as np
import pytest

import cases
import kat_cases as kc
import limit_bracket_cases as lc
from parity import MAX_SENSITIVE_FRAC, assert_parity, branch_aware_compare

NZS = [2, 64, 65, 120, 129]
NCOLS = [1, 5]
SENS_CUT = 1e-11                              # parity.verdict: beyond it a level leans on the sensitivity allowance
R1 = 1e-12
# (q, n) per regime: inside, beyond the lower limit (many small particles), beyond the upper limit (few large ones)
ICE = ((1e-5, 1e5), (1e-8, 1e9), (1e-4, 1e2))
RAIN = ((1e-4, 1e4), (1e-9, 1e5), (1e-3, 1e1))
SET_NC = 0.3                                  # cm-3: nc is Nt_c in these contexts (M:1410), nu = 15
CLOUD = (1e-6, 2e-11, 2e-4)                   # qc inside, rc = qc rho beyond the lower limit (a trace), qc beyond the upper


# ---------------- (a) the probe ----------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("lbeval_gpu")
    exe = lc.build_driver(d)
    return exe, d, lc.constants(exe)


@pytest.mark.gpu
@pytest.mark.parametrize("site", lc.SITES)
def test_bracket_agrees_with_the_original_path_on_the_device(gpu_mixed, driver, site):
    exe, d, c = driver
    rng = np.random.default_rng(2000 + site)
    an, ad = lc.adjacent_pairs(c, site, 200, rng)
    fn, fd = lc.floor_pairs(c, site, 100, rng)                             # num at the number floors R2 / 2., den at R1 among them
    an, ad = np.concatenate([an, fn]), np.concatenate([ad, fd])
    un, ud = lc.log_uniform_pairs(c, site, 20000, rng)
    num, den = np.concatenate([an, un]), np.concatenate([ad, ud])
    sites = np.full(num.size, float(site))
    out = gpu_mixed.math_probe_ex("limit_bracket", num, den, sites).astype(np.int64)
    bracket, original, inside = out % 4, out // 4 % 4, out // 16
    certain = bracket != lc.AMBIGUOUS
    print("site %d: %d pairs, %d ambiguous, all among the %d threshold-adjacent ones" % (site, num.size, int((~certain).sum()), an.size))
    assert set(np.unique(original)) <= {lc.BELOW, lc.INSIDE, lc.ABOVE}
    assert (bracket[certain] == original[certain]).all()
    assert np.array_equal(inside == 1, bracket == lc.INSIDE)               # what the kernel votes on: decide() == INSIDE
    assert np.array_equal(bracket, lc.host_answers(exe, d, num, den, sites))
    assert certain[an.size:].all() and (~certain[:an.size]).any()
    assert all((bracket == a).any() for a in (lc.BELOW, lc.INSIDE, lc.ABOVE))


@pytest.mark.gpu
def test_probe_refuses_binary32_and_bad_sites(gpu_mixed):
    from kid_amd.thompson import KidmpError
    one = np.ones(4)
    for kw in (dict(z=one * 16.0), dict(z=one * 1.5), dict(z=-one), dict(z=one, binary32=True)):
        with pytest.raises(KidmpError):
            gpu_mixed.math_probe_ex("limit_bracket", one, one, **kw)


# ---------------- (b) end to end ----------------
def _resample(col, nz):
    x0 = np.linspace(0.0, 1.0, col["qv"].shape[0])
    x1 = np.linspace(0.0, 1.0, nz)
    out = {k: np.interp(x1, x0, v) for k, v in col.items()}
    out["dz"] = np.full(nz, 15000.0 / nz)
    return out


@functools.lru_cache(maxsize=None)
def _columns(nz, mixed):
    """Five columns; in columns c = 0 .. 3 the ice and cloud regime of level k is (k + c) % 3, the rain regime
    (k + c + 1) % 3 (so a trace of rain never shares a level with autoconverting cloud water); column 4 is inside
    everywhere.  Ice where it stays frozen (T < 263 K), rain below 233 K's level, and the trace of cloud water only where
    no snow rimes it away (there the oracle itself moves by 1e-9 under ulp-sized perturbations: a cancellation residue,
    nothing the limit tests decide)."""
    cols = []
    for c in range(5):
        col = _resample(kc.kat_a(mixed), nz)
        reg = (np.arange(nz) + c) % 3 if c < 4 else np.zeros(nz, dtype=int)
        rain_reg = (reg + 1) % 3 if c < 4 else reg
        for r in range(3):
            w = (rain_reg == r) & (col["t"] > 233.0)
            col["qr"][w], col["nr"][w] = RAIN[r]
            w = (reg == r) & (col["t"] > 240.0)
            if r == 1:                         # a fixed rc = qc rho, and only where no snow rimes the trace away
                rho = 0.622 * col["p"] / (287.04 * col["t"] * (col["qv"] + 0.622))
                w &= col["qs"] == 0.0
                col["qc"][w] = CLOUD[1] / rho[w]
            else:
                col["qc"][w] = CLOUD[r]
            if mixed:
                w = (reg == r) & (col["t"] < 263.0)
                col["qi"][w], col["ni"][w] = ICE[r]
        cols.append(col)
    return cols


def _batch(nz, ncol, mixed):
    cols = _columns(nz, mixed)[:ncol]
    return {k: np.ascontiguousarray(np.stack([c[k] for c in cols])) for k in cases.KEYS}


def _input_ice_regimes(st):
    """0 / 1 / 2 (inside / below / above), -1 where there is no ice: what block B's ice test (M:1420-1445) sees, which is the
    INPUT state (ni > R2 everywhere ice is set), in plain binary64 (the inputs are far from every limit)"""
    am_i = 3.1415926536 * 890.0 / 6.0
    with np.errstate(divide="ignore", invalid="ignore"):
        xd = 4.0 / np.cbrt(am_i * 6.0 * st["ni"] / st["qi"])
    return np.where(st["qi"] > R1, np.where(xd < 5e-6, 1, np.where(xd > 300e-6, 2, 0)), -1)


def _all_three_nearby(reg, ncol=4, span=4):
    return any(set(reg[c, k:k + span]) >= {0, 1, 2} for c in range(ncol) for k in range(max(1, reg.shape[1] - span + 1)))


def test_block_b_sees_every_outcome_in_neighbouring_levels():
    for nz in NZS[1:]:
        st = _batch(nz, 5, True)
        ice = _input_ice_regimes(st)
        assert _all_three_nearby(ice, span=3), nz
        assert (ice[4] <= 0).all() and (ice[4] == 0).any()                      # the fifth column: inside wherever it has ice
    assert {0, 1, 2} <= set(_input_ice_regimes(_batch(2, 5, True))[:4, 1])


MARGIN = 1.5                                  # a level counts for an outcome only if num / den is this factor clear of both limits


def _post_tendency_regimes(o, st, mixed, dt=10.0, Nt_c=100.e6):
    """What block J's three tests see, derived from the ORACLE's own process rates (column_step(want_rates=True): the
    limited rates of M:2967-3119, per m3): the tendencies of M:2393-2530 rebuilt from them in binary64,
        xrc, xri, xrr = MAX(R1, (q + qten DT) rho)     xnc, xni, xnr = MAX(2. | R2, (n + nten DT) rho)
    and num / den of each test set against (c/D)**3.  Returns (ice, rain, cloud) as [ncol, nz] arrays of 0 / 1 / 2 (inside /
    beyond the lower / beyond the upper limit) and -1 where the test is not entered (x <= R1) or where this derivation cannot
    vouch for the outcome:
      * num / den within a factor MARGIN of a limit (the sums here are not the oracle's to the last bit);
      * a species the rates leave all but consumed (the conservation rescaling of M:2300-2390 then changed mass rates whose
        number rates are not recorded);
      * rain in the mixed-phase context where ice, snow or graupel are present or T < T_0: prr_rcs, prr_rcg, prg_rfz and
        prr_rci are not among the recorded rates (they vanish elsewhere);
      * the droplet number sinks pnc_* are not recorded either: they are rebuilt from their mass rates (pnc = pr nc / rc,
        M:1722, M:1961, M:1983) and, for autoconversion, from M:1708."""
    from oracle.oracle import RATE_NAMES
    ncol, nz = st["qv"].shape
    am_i, am_r, T_0, R2 = 3.1415926536 * 890.0 / 6.0, 3.1415926536 * 1000.0 / 6.0, 273.15, 1e-6
    out = np.full((3, ncol, nz), -1)

    def cls(entered, ratio, c, d_lo, d_hi):
        t_lo, t_hi = (c / d_lo) ** 3, (c / d_hi) ** 3
        r = np.where(ratio > MARGIN * t_lo, 1, np.where(ratio < t_hi / MARGIN, 2,
                     np.where((ratio > MARGIN * t_hi) & (ratio < t_lo / MARGIN), 0, -1)))
        return np.where(entered, r, -1)

    for c in range(ncol):
        col = {k: np.ascontiguousarray(st[k][c].copy()) for k in st}
        _, rates, _, no_micro = o.column_step(col, dt, want_rates=True)
        if no_micro:
            continue
        r = dict(zip(RATE_NAMES, rates))
        rho = 0.622 * st["p"][c] / (287.04 * st["t"][c] * (np.maximum(st["qv"][c], 1e-10) + 0.622))
        q = {k: np.where(st[k][c] > R1, st[k][c], 0.0) for k in ("qc", "qi", "qr", "qs", "qg")}
        ni1, nr1 = np.where(q["qi"] > 0, st["ni"][c], 0.0), np.where(q["qr"] > 0, st["nr"][c], 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            # ice, M:2457-2480
            qi2 = q["qi"] + (r["pri_inu"] + r["pri_ihm"] + r["pri_wfz"] + r["pri_rfz"] + r["pri_ide"] - r["prs_iau"] - r["prs_sci"] - r["pri_rci"]) / rho * dt
            ni2 = ni1 + (r["pni_rfz"] + r["pni_wfz"] + r["pni_inu"] + r["pni_ihm"] + r["pni_ide"] - r["pni_iau"] - r["pni_sci"] - r["pni_rci"]) / rho * dt
            xri, xni = np.maximum(R1, qi2 * rho), np.maximum(R2, ni2 * rho)
            out[0, c] = cls((xri > 10 * R1) & (qi2 > 1e-3 * q["qi"]), am_i * 6.0 * xni / xri, 4.0, 5e-6, 300e-6)
            # rain, M:2508-2530
            qr2 = q["qr"] + (r["prr_wau"] + r["prr_rcw"] + r["prr_sml"] + r["prr_gml"]) / rho * dt
            nr2 = nr1 + (r["pnr_wau"] + r["pnr_sml"] + r["pnr_gml"] - r["pnr_rcr"] - r["pnr_rcs"] - r["pnr_rcg"] - r["pnr_rfz"] - r["pnr_rci"]) / rho * dt
            xrr, xnr = np.maximum(R1, qr2 * rho), np.maximum(R2, nr2 * rho)
            known = (q["qi"] == 0) & (q["qs"] == 0) & (q["qg"] == 0) & (st["t"][c] > T_0) if mixed else True
            out[1, c] = cls((xrr > 10 * R1) & known, am_r * 6.0 * xnr / xrr, 3.0 + 0.672, 0.75 * 50e-6, 2.5e-3)
            # cloud droplets, M:2422-2445: nc is Nt_c on input (M:1410); the denominator is the INPUT rc
            rc = q["qc"] * rho
            qc2 = q["qc"] - (r["prr_wau"] + r["pri_wfz"] + r["prr_rcw"] + r["prs_scw"] + r["prg_scw"] + r["prg_gcw"]) / rho * dt
            nu0 = min(15, int(round(1000.e6 / Nt_c)) + 2)
            lamc = np.cbrt(Nt_c * am_r * (nu0 + 3) * (nu0 + 2) * (nu0 + 1) / rc)
            mvd_c = (3.0 + nu0 + 0.672) / lamc
            nc_m = (np.minimum(Nt_c / dt, r["prr_wau"] / (am_r * mvd_c ** 3)) + r["pni_wfz"]
                    + Nt_c / rc * (r["prr_rcw"] + r["prs_scw"] + r["prg_gcw"]))
            regs = []
            for f in (0.5, 1.0, 2.0):          # the rebuilt sink halved and doubled: the outcome must not hang on it
                xnc = np.maximum(2.0, Nt_c - f * np.nan_to_num(nc_m) * dt)
                nu = np.minimum(15, np.rint(1000.e6 / xnc).astype(int) + 2)
                ratio = xnc * am_r * (nu + 3) * (nu + 2) * (nu + 1) / rc
                t_lo, t_hi = ((nu + 4.0) / 1e-6) ** 3, ((nu + 4.0) / 100e-6) ** 3
                regs.append(np.where(ratio > MARGIN * t_lo, 1, np.where(ratio < t_hi / MARGIN, 2,
                                     np.where((ratio > MARGIN * t_hi) & (ratio < t_lo / MARGIN), 0, -1))))
            reg = np.where((regs[0] == regs[1]) & (regs[1] == regs[2]), regs[1], -1)
            out[2, c] = np.where((qc2 * rho > 10 * R1) & (qc2 > 1e-3 * q["qc"]), reg, -1)
    return out[0], out[1], out[2]


@pytest.fixture(scope="module")
def oracle_warm_lo():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True, set_Nc=SET_NC)
    yield o
    o.close()


@pytest.fixture(scope="module")
def oracle_mixed_lo():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=False, set_Nc=SET_NC)       # its tables: built once per value, then cached
    yield o
    o.close()


@pytest.fixture(scope="module")
def gpu_lo():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible; the HIP path has no CPU fallback")
    from kid_amd import ThompsonMP
    made = {}

    def get(mixed):
        if mixed not in made:
            made[mixed] = ThompsonMP(iiwarm=not mixed, set_Nc=SET_NC)
        return made[mixed]

    yield get
    for m in made.values():
        m.close()


def _block_j_outcomes(o, mixed):
    for nz in NZS:
        st = _batch(nz, 5, mixed)
        regs = dict(zip(("ice", "rain", "cloud"), _post_tendency_regimes(o, st, mixed, Nt_c=SET_NC * 1e6)))
        for name, reg in regs.items():
            counts = {v: int((reg[:4] == v).sum()) for v in (-1, 0, 1, 2)}
            print("mixed" if mixed else "warm", nz, name, counts)
            if name == "ice" and not mixed:
                assert (reg == -1).all()
            elif nz >= 64:
                assert _all_three_nearby(reg), (mixed, nz, name, counts)
                assert (reg[4] == 0).sum() >= 0.9 * (reg[4] >= 0).sum() > 0, (mixed, nz, name)   # the fifth column stays inside
            elif name == "ice":                  # two levels: nucleation at 210 K moves the few large crystals inside
                assert {0, 1} <= set(reg[:4].ravel()), (mixed, nz, name, counts)
            else:
                assert {0, 1, 2} <= set(reg[:4].ravel()), (mixed, nz, name, counts)


def test_block_j_sees_every_outcome_after_the_tendencies_warm(oracle_warm_lo):
    _block_j_outcomes(oracle_warm_lo, False)


@pytest.mark.slow
def test_block_j_sees_every_outcome_after_the_tendencies_mixed(oracle_mixed_lo):
    _block_j_outcomes(oracle_mixed_lo, True)


def _sensitive(o, nz, ncol, mixed):
    st = _batch(nz, ncol, mixed)
    ref = {k: v.copy() for k, v in st.items()}
    o.batch_step(ref, 10.0)
    cmp = branch_aware_compare(o, st, 10.0, ref)
    n_sens = int((cmp["sens"] > SENS_CUT).sum())
    print(nz, ncol, "mixed" if mixed else "warm", "sensitive levels", n_sens, "of", cmp["sens"].size, "max sens %.2e" % cmp["sens"].max())
    assert n_sens <= int(np.ceil(MAX_SENSITIVE_FRAC * cmp["sens"].size)), (nz, ncol, mixed, n_sens)


def test_inputs_are_well_conditioned_warm(oracle_warm_lo):
    for nz in NZS:
        for ncol in NCOLS:
            _sensitive(oracle_warm_lo, nz, ncol, False)


@pytest.mark.slow
def test_inputs_are_well_conditioned_mixed(oracle_mixed_lo):
    for nz in NZS:
        for ncol in NCOLS:
            _sensitive(oracle_mixed_lo, nz, ncol, True)


def _run(m, o, st):
    got = {k: v.copy() for k, v in st.items()}
    gppt, _ = m.batch_step_host(got, 10.0)
    v = assert_parity(o, st, 10.0, got, gppt)
    print(st["qv"].shape, v)


@pytest.mark.gpu
@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nz", NZS)
def test_mixed_phase_step_matches_oracle(gpu_lo, oracle_mixed_lo, nz, ncol):
    _run(gpu_lo(True), oracle_mixed_lo, _batch(nz, ncol, True))


@pytest.mark.gpu
@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nz", NZS)
def test_warm_rain_step_matches_oracle(gpu_lo, oracle_warm_lo, nz, ncol):
    _run(gpu_lo(False), oracle_warm_lo, _batch(nz, ncol, False))
