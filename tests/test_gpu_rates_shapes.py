"""The 36 rate profiles of the column kernel at every level count and variant (-m gpu).

The RATES instantiation is what a stock KiD run gets (l_rate_diagnostics = .true.).  It stores its rates from inside
the banded sweep -- 34 rows in pass 1, rows 32 and 34 after block N, zeros for a no_micro column in pass 0 -- at
rates + column * 36 * nz + row * nz + k, and the band arithmetic differs between four columns per workgroup
(nz <= 120) and one, and between one, two, three and four level groups.  Until now the rate VALUES were compared
with the oracle at nz = 120 only, in binary64, without aerosols, at one batch size.  Here: every bucket from both
sides of its edges, mixed / aerosol-aware / warm / warm + aerosol-aware, a bound per-column droplet number, every
workgroup remainder with a dry column at every position, the buffer's edges and its reuse, chained steps, the
chunked host entry, the column sum, and the two binary32 builds.

Bounds: rates_parity.assert_rates (1e-10 or 10 x the oracle's own response, parity.ABS_CEILING, at most 1e-3 of the
elements beyond 1e-10: tests/test_rates_inputs.py holds the inputs to that share), parity.assert_parity for the
state as test_gpu_pass5_handover.py calls it, and bit equality where the project already claims it.  The binary32
figures are measured ones, see P32N_BOUNDS.
"""
import numpy as np
import pytest

import rates_cases as rc
from parity import OUT, assert_parity
from parity32 import assert_rates32
from rates_parity import NRATES, assert_rates, oracle_rates, rates_metric
from test_gpu_column_nc import CYCLE, _own_defaults
from test_gpu_precision32_levels import RATES_HELD          # (kind, nz) where every p32n rate element is held

pytestmark = pytest.mark.gpu
DT = rc.DT
PAYLOAD = 0x7FF8DEADBEEF0001            # a quiet NaN no arithmetic produces


# ---- contexts and oracles that conftest.py does not offer ----
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible; the HIP path has no CPU fallback")


@pytest.fixture(scope="module")
def gpu_warm_aero():
    _need_gpu()
    from kid_amd import ThompsonMP
    m = ThompsonMP(iiwarm=True, aerosol_aware=True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def oracle_warm_aero():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True, aerosol_aware=True)               # warm rain: no tables to build
    yield o
    o.close()


@pytest.fixture(scope="module")
def own_ctx():
    """A context of its own per droplet number: the per-value reference of the bound batches, never bound itself."""
    _need_gpu()
    from kid_amd import ThompsonMP
    made = {}

    def get(iiwarm, set_Nc):
        key = (bool(iiwarm), float(set_Nc))
        if key not in made:
            made[key] = ThompsonMP(iiwarm=iiwarm, set_Nc=set_Nc)
        return made[key]

    yield get
    for m in made.values():
        m.close()


_FIXTURES = {"mixed": ("gpu_mixed", "oracle_mixed"), "aero": ("gpu_mixed_aero", "oracle_mixed_aero"),
             "warm": ("gpu_warm", "oracle_warm"), "warm_aero": ("gpu_warm_aero", "oracle_warm_aero")}


def _pair(request, kind):
    g, o = _FIXTURES[kind]
    return request.getfixturevalue(g), request.getfixturevalue(o)


# ---- stepping ----
def _copy(st):
    return {k: np.ascontiguousarray(v.copy()) for k, v in st.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _host(m, st):
    """One step through the host entry with rates: (state after, ppt, rates [ncol, 36, nz])."""
    got = _copy(st)
    ppt, rates = m.batch_step_host(got, DT, want_rates=True)
    return got, ppt, rates


def _dev(st):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in st.items()}


def _device(m, st, rates=None):
    """One step through the device entry into `rates` (a fresh zeroed tensor when None): (state after, ppt, rates)."""
    import torch
    ncol, nz = st["qv"].shape
    dev = _dev(st)
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda")
    if rates is None:
        rates = torch.zeros(ncol, NRATES, nz, dtype=torch.float64, device="cuda")
    m.batch_step(dev, DT, ppt, rates=rates)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dev.items()}, ppt.cpu().numpy(), rates.cpu().numpy()


_shared = {}


def _stepped(kind, nz, m):
    """(inputs, state after, ppt, rates) of one kind and level count through the host entry: computed once, shared by
    the tests below, written by nobody."""
    if (kind, nz) not in _shared:
        st = rc.batch(kind, nz)
        _shared[(kind, nz)] = (st,) + _host(m, st)
    return _shared[(kind, nz)]


def _brief(v):
    return {k: x for k, x in v.items() if k != "cmp"}


def _check_values(m, o, kind, nz, st=None, got=None):
    st, got, gppt, rates = (st,) + got if st is not None else _stepped(kind, nz, m)
    v = assert_rates(o.column_step, st, DT, rates)
    print(kind, nz, "rates", _brief(v))
    # the state: the call of test_handover_matches_oracle; the warm batch at the cap test_other_level_counts_warm has
    sv = assert_parity(o, st, DT, got, gppt, max_branch_frac=0.08 if kind.startswith("warm") else 0.2)
    print(kind, nz, "state", sv)
    if kind.startswith("warm"):
        assert not _bits(rates[:, :30]).any()                 # +0.0, bit for bit: the 30 rates of the ice phase
        assert rates[:, 30:].any()
    else:
        assert v["cmp"]["dry"][rc.DRY] and not _bits(rates[rc.DRY]).any()
    return v


# ---- 1. values, every bucket, binary64 ----
@pytest.mark.parametrize("kind,nz", [(k, nz) for k in rc.KINDS for nz in rc.levels(k)])
def test_rate_values_at_every_level_count(request, kind, nz):
    m, o = _pair(request, kind)
    _check_values(m, o, kind, nz)


# ---- 2. warm + aerosol-aware ----
@pytest.mark.parametrize("nz", [64, 120, 200])
def test_rate_values_warm_aerosol_aware(gpu_warm_aero, oracle_warm_aero, nz):
    st = rc.batch("warm_aero", nz)
    _check_values(gpu_warm_aero, oracle_warm_aero, "warm_aero", nz, st, _host(gpu_warm_aero, st))
    # the switch does something to the rates: the plain warm oracle gives other autoconversion numbers
    ref_aero, _ = oracle_rates(oracle_warm_aero.column_step, st, DT)
    from oracle.oracle import Oracle
    plain = Oracle(iiwarm=True)
    try:
        ref_plain, _ = oracle_rates(plain.column_step, st, DT)
    finally:
        plain.close()
    assert not np.array_equal(ref_aero[:, 30:], ref_plain[:, 30:])


# ---- 3. a bound per-column droplet number, with rates ----
def _nc_batch(iiwarm, nz, ncol=10):
    values = np.array([CYCLE[c % 4] for c in range(ncol)])
    st = rc.batch("warm" if iiwarm else "mixed", nz, pick=[c % rc.NCOL for c in range(ncol)])
    return _own_defaults(st, values), values


@pytest.mark.parametrize("nz", [40, 120, 128, 200])          # NJ = 1, banded (CPW = 4), CPW = 1, tall
@pytest.mark.parametrize("iiwarm", [False, True], ids=["mixed", "warm"])
def test_bound_droplet_number_rates_are_those_of_a_context_of_each_value(request, own_ctx, iiwarm, nz):
    m = request.getfixturevalue("gpu_warm" if iiwarm else "gpu_mixed")
    st, values = _nc_batch(iiwarm, nz)
    try:
        m.set_column_nc(values)
        got, gppt, grates = _device(m, st)
        differ = 0
        for v in CYCLE:
            idx = np.flatnonzero(values == v)
            sub = {k: np.ascontiguousarray(a[idx]) for k, a in st.items()}
            ref, rppt, rrates = _device(own_ctx(iiwarm, v), sub)
            assert _same_bits(rrates, grates[idx]), v
            assert _same_bits(rppt, gppt[idx]), v
            for k in OUT:
                assert _same_bits(ref[k], got[k][idx]), (v, k)
            differ += v != 100.0 and not np.array_equal(rrates, _device(own_ctx(iiwarm, 100.0), sub)[2])
        assert differ                                         # the droplet number reaches the rates (autoconversion)
        # a uniform binding at the context's own value: the scalar context's bits
        m.set_column_nc(None)
        plain = _device(m, st)
        m.set_column_nc(np.full(values.size, 100.0))
        bound = _device(m, st)
        assert _same_bits(plain[2], bound[2]) and _same_bits(plain[1], bound[1])
        for k in OUT:
            assert _same_bits(plain[0][k], bound[0][k]), k
        assert plain[2].any()
    finally:
        m.set_column_nc(None)
    assert m.column_nc_count == 0


# ---- 4. workgroup remainders ----
LIVE = (0, 2, 3, 4)


def _alone(nz, m):
    """Every column of the mixed batch stepped on its own (ncol = 1)."""
    if ("alone", nz) not in _shared:
        _shared[("alone", nz)] = [_host(m, rc.batch("mixed", nz, pick=(c,))) for c in range(rc.NCOL)]
    return _shared[("alone", nz)]


@pytest.mark.parametrize("ncol", [1, 2, 3, 5, 6, 7])
@pytest.mark.parametrize("nz", [64, 120])                     # the buckets with four columns per workgroup
def test_workgroup_remainders_keep_every_columns_rates(gpu_mixed, oracle_mixed, nz, ncol):
    alone = _alone(nz, gpu_mixed)
    for pos in range(min(ncol, 4)):
        pick = [LIVE[(i + pos) % 4] for i in range(ncol)]
        pick[pos] = rc.DRY
        st = rc.batch("mixed", nz, pick=pick)
        got, gppt, rates = _host(gpu_mixed, st)
        for i, c in enumerate(pick):
            agot, appt, arates = alone[c]
            assert _same_bits(rates[i], arates[0]), (pos, i, c)
            assert _same_bits(gppt[i], appt[0]), (pos, i, c)
            for k in OUT:
                assert _same_bits(got[k][i], agot[k][0]), (pos, i, c, k)
            if c == rc.DRY:
                assert not _bits(rates[i]).any(), (pos, i)
            else:
                assert rates[i].any(), (pos, i)
        if pos == 0:
            print(nz, ncol, _brief(assert_rates(oracle_mixed.column_step, st, DT, rates)))


# ---- 5. buffer discipline, device entry ----
def _guarded(ncol, nz):
    """A float64 tensor filled with PAYLOAD; the rates view is its middle, 36 nz elements of guard on either side."""
    import torch
    g, n = NRATES * nz, ncol * NRATES * nz
    big = torch.empty(n + 2 * g, dtype=torch.float64, device="cuda")
    big.view(torch.int64).fill_(PAYLOAD)
    return big, big[g:g + n].view(ncol, NRATES, nz), g


def _check_guarded(m, kind, nz, and_dry):
    import torch
    ncol = rc.NCOL
    big, view, g = _guarded(ncol, nz)
    assert view.is_contiguous() and view.data_ptr() == big.data_ptr() + 8 * g
    _, _, rates = _device(m, rc.batch(kind, nz), rates=view)
    bits = big.view(torch.int64).cpu().numpy()
    assert (bits[:g] == PAYLOAD).all() and (bits[-g:] == PAYLOAD).all(), "a store outside the rate buffer"
    assert not (bits[g:-g] == PAYLOAD).any(), "an element of the rate buffer left unwritten"
    assert np.isfinite(rates).all() and rates.any()
    if and_dry:                                               # the same buffer, every column through the no_micro exit
        _, _, rates = _device(m, rc.all_dry(kind, nz), rates=view)
        bits = big.view(torch.int64).cpu().numpy()
        assert (bits[:g] == PAYLOAD).all() and (bits[-g:] == PAYLOAD).all()
        assert not bits[g:-g].any(), "a rate of the previous step left in a no_micro column"


@pytest.mark.parametrize("nz", [2, 63, 65, 121, 129, 193, 255])
def test_rate_buffer_is_written_whole_and_nowhere_else(gpu_mixed, nz):
    _check_guarded(gpu_mixed, "mixed", nz, and_dry=True)


@pytest.mark.parametrize("nz", [65, 193])
@pytest.mark.parametrize("kind", ["aero", "warm"])
def test_rate_buffer_is_written_whole_other_contexts(request, kind, nz):
    _check_guarded(_pair(request, kind)[0], kind, nz, and_dry=False)


# ---- 6. three chained steps, one rates tensor ----
@pytest.mark.parametrize("nz", [65, 193])
def test_chained_steps_leave_no_stale_rates(gpu_mixed, oracle_mixed, nz):
    """Device-resident, the rates tensor reused and never cleared: each step's rates against the oracle stepped ONCE
    from the state the GPU actually had before that step (three one-step comparisons, no drift in the bound)."""
    import torch
    st = rc.batch("mixed", nz)
    dev = _dev(st)
    ppt = torch.zeros(rc.NCOL, 4, dtype=torch.float64, device="cuda")
    rates = torch.zeros(rc.NCOL, NRATES, nz, dtype=torch.float64, device="cuda")
    previous = None
    for n in range(3):
        pre = {k: v.cpu().numpy() for k, v in dev.items()}
        gpu_mixed.batch_step(dev, DT, ppt, rates=rates)
        torch.cuda.synchronize()
        now = rates.cpu().numpy()
        v = assert_rates(oracle_mixed.column_step, pre, DT, now)
        print(nz, "step", n, _brief(v))
        assert not _bits(now[rc.DRY]).any()
        assert previous is None or not np.array_equal(previous, now)      # the state moved, so did the rates
        previous = now


# ---- 7. host entry in chunks ----
@pytest.mark.parametrize("nz", [65, 193])
def test_chunked_host_entry_gives_the_device_entrys_rates(gpu_mixed, nz):
    st = rc.batch("mixed", nz)
    dgot, dppt, drates = _device(gpu_mixed, st)
    gpu_mixed.set_host_chunk(2)                               # 5 columns: chunks of 2, 2 and 1
    try:
        hgot, hppt, hrates = _host(gpu_mixed, st)
    finally:
        gpu_mixed.set_host_chunk(0)
    assert _same_bits(hrates, drates) and _same_bits(hppt, dppt)
    for k in OUT:
        assert _same_bits(hgot[k], dgot[k]), k
    assert drates.any()


# ---- 8. reduce_rates at other shapes ----
def _reduce_ref(rates):
    """The documented order: per = ceil(ncol / 128) columns per chunk, summed in sequence inside each of the 128
    chunks, then the chunks summed in sequence."""
    ncol = rates.shape[0]
    per = -(-ncol // 128)
    out = np.zeros(rates.shape[1:])
    for j in range(128):
        acc = np.zeros(rates.shape[1:])
        for c in range(j * per, min(j * per + per, ncol)):
            acc = acc + rates[c]
        out = out + acc
    return out


@pytest.mark.parametrize("ncol", [1, 5, 130])
@pytest.mark.parametrize("nz", [2, 65, 256])
def test_reduce_rates_at_other_shapes(gpu_mixed, nz, ncol):
    import torch
    src = _stepped("mixed", nz, gpu_mixed)[3]
    idx = np.arange(ncol) % rc.NCOL
    rates = np.ascontiguousarray(src[idx] * (1.0 + 0.01 * np.arange(ncol))[:, None, None])     # no two columns alike
    got = gpu_mixed.reduce_rates(torch.from_numpy(rates).cuda()).cpu().numpy()
    assert got.shape == (NRATES, nz) and _same_bits(got, _reduce_ref(rates))
    assert got.any()


# ---- 9. the binary32 builds ----
# Nobody had a number for these.  Measured on the MI355X over the inputs of rates_cases.py rounded to binary32, element
# metric of rates_parity, worst of the five level counts:
#                                            all 36 nz elements of every column    where the reference is non-zero
#                                            median      q99        max            median     (share of the elements)
#   p32n kernel against the p32n ORACLE mixed  0           5.78e-6    1.8e7          7.34e-8    (~20 %)
#                                       warm   0           5.78e-6    5.0e-1         2.05e-7    (~4 %)
#   f32 kernel against the p32n KERNEL  mixed  0           7.26e-7    1.4e8          2.96e-8
#                                       warm   0           1.43e-7    1.2e-6         6.01e-8
# More than half of the elements are zero on both sides, so the median over all elements is zero and stays an
# assertion of exactly that; the median where the reference is non-zero is the informative one and is asserted too.
# The bounds are 3 x the measured figure rounded up to one digit: the CPU oracle's powf / expf differ between hosts
# (ADVICE.md).  The maximum is printed, not asserted (as in test_p32n_kernel_against_the_p32n_oracle): it belongs to
# the handful of elements where binary32 rounding decides a branch -- a rate that is zero on one side and not on the
# other in a row that is otherwise alive (at most 4 of 34 740 elements), measured against 1e-9 of the row's largest.
#            (median, q99) over all elements, median where the reference is non-zero
P32N_BOUNDS = {"mixed": (0.0, 2e-5, 3e-7), "warm": (0.0, 2e-5, 7e-7)}
F32_BOUNDS = {"mixed": (0.0, 3e-6, 9e-8), "warm": (0.0, 5e-7, 2e-7)}
NZ32 = (17, 65, 120, 129, 193)
ZERO_DISAGREE_FRAC = 1e-3


def _stats(err):
    e = np.where(np.isfinite(err), err, np.inf).ravel()
    return float(np.median(e)), float(np.quantile(e, 0.99)), float(e.max())


def _stepped32(kind, nz, m, arith):
    if (kind, nz, arith) not in _shared:
        st = rc.to32(rc.batch(kind, nz))
        got = _copy(st)
        ppt, rates, _ = m.batch_step32_host(got, DT, arith=arith, want_rates=True)
        _shared[(kind, nz, arith)] = (st, got, ppt, rates)
    return _shared[(kind, nz, arith)]


def _zero_checks(rates, ref, what):
    zero_rows = ~np.any(ref != 0, axis=2)                     # [ncol, 36]: rows the reference leaves at zero
    assert not rates[zero_rows].any(), (what, "a row the reference leaves at zero", np.argwhere(rates.any(axis=2) & zero_rows)[:8])
    disagree = (rates != 0) != (ref != 0)
    print(what, "elements that disagree on zero / non-zero: %d of %d" % (disagree.sum(), disagree.size))
    assert disagree.sum() <= int(np.ceil(ZERO_DISAGREE_FRAC * disagree.size)), (what, int(disagree.sum()), np.argwhere(disagree)[:8])


def _hold32(what, kind, nz, rates, ref, bounds):
    """Print the figures, then hold `rates` to `ref`: zeros where the reference has zero rows, the measured bounds."""
    assert rates.dtype == np.float64 and np.isfinite(rates).all()
    err = rates_metric(rates, ref)
    med, q99, mx = _stats(err)
    nzr = ref != 0
    med_nz, q99_nz, _ = _stats(err[nzr])
    w = np.unravel_index(int(np.argmax(np.where(np.isfinite(err), err, np.inf))), err.shape)
    print("%s nz %3d %s: median %.2e q99 %.2e max %.2e at (column, row, level) %s got %.6e reference %.6e; where the "
          "reference is non-zero (%d of %d): median %.2e q99 %.2e"
          % (kind, nz, what, med, q99, mx, tuple(int(i) for i in w), rates[w], ref[w], nzr.sum(), nzr.size, med_nz, q99_nz))
    _zero_checks(rates, ref, (kind, nz, what))
    assert med <= bounds[kind][0] and q99 <= bounds[kind][1] and med_nz <= bounds[kind][2], (med, q99, med_nz, mx)


@pytest.mark.parametrize("nz", NZ32)
@pytest.mark.parametrize("kind", ["mixed", "warm"])
def test_p32n_rates_against_the_p32n_oracle(request, kind, nz):
    m, o = _pair(request, kind)
    st, _, _, rates = _stepped32(kind, nz, m, "p32n")
    if (kind, nz) in RATES_HELD:
        # EVERY element (the maximum is only printed below): within max(the q99 bound, 10 x the spread of that rate under
        # 3-ulp moves of the P32n oracle's binary32 special functions, reciprocals and rate limiters), parity32.assert_rates32
        assert_rates32(o, st, DT, rates, P32N_BOUNDS[kind][1], what="%s nz %d" % (kind, nz))
    _hold32("p32n kernel against the p32n oracle", kind, nz, rates, oracle_rates(o.column_step_p32n, st, DT)[0], P32N_BOUNDS)


@pytest.mark.parametrize("nz", NZ32)
@pytest.mark.parametrize("kind", ["mixed", "warm"])
def test_f32_rates_stay_near_the_p32n_kernels(request, kind, nz):
    m, _ = _pair(request, kind)
    _hold32("f32 kernel against the p32n kernel", kind, nz, _stepped32(kind, nz, m, "f32")[3],
            _stepped32(kind, nz, m, "p32n")[3], F32_BOUNDS)
