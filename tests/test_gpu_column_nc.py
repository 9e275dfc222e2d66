"""A droplet number per column (kidmp_set_column_nc, ThompsonMP.set_column_nc): Nd ensembles in one launch.  -m gpu.

The decisive checks are exact and rest on no tolerance: a bound uniform array must give the bits of the context's own
scalar, a bound value X the bits of a context initialised with set_Nc = X, and every member of a mixed ensemble the bits
its own per-value context gives for that column.  Against the CPU oracle the project's existing bounds are used as they
are: parity.assert_parity (P64), the statistics of test_gpu_precision.py (P32n), 1e-12 for the radii
(test_gpu_column_outputs.py)."""
import ctypes as C

import numpy as np
import pytest

import cases
import kat_cases as kc
from parity import FLOORS, OUT, assert_parity

pytestmark = pytest.mark.gpu
f32 = np.float32
CYCLE = (25.0, 100.0, 300.0, 1000.0)            # nu_c = 15, 12, 5, 3


# ---- contexts and oracles at other droplet numbers than the default (conftest.py only has set_Nc = 100) ----
@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible; the HIP path has no CPU fallback")
    from kid_amd import ThompsonMP
    made = {}

    def get(iiwarm, set_Nc=100.0, own=False):
        """own: the per-value reference context, never bound -- not the one the tests bind arrays to, also at 100"""
        key = (bool(iiwarm), float(set_Nc), bool(own))
        if key not in made:
            made[key] = ThompsonMP(iiwarm=iiwarm, set_Nc=set_Nc)
        return made[key]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle.oracle import Oracle
    made = {}

    def get(iiwarm, set_Nc=100.0):
        key = (bool(iiwarm), float(set_Nc))
        if key not in made:
            made[key] = Oracle(iiwarm=iiwarm, set_Nc=set_Nc)      # mixed phase: ~55 s of tables per new value, cached
        return made[key]

    yield get
    for o in made.values():
        o.close()


@pytest.fixture(autouse=True)
def _leave_unbound(ctx):
    yield
    for iiwarm in (False, True):
        ctx(iiwarm).set_column_nc(None)


# ---- batches ----
def _copy(st):
    return {k: np.ascontiguousarray(v.copy()) for k, v in st.items()}


def _subset(st, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}


def _own_defaults(st, values):
    """Every member starts from the droplet number of its own set_Nc (M:960), as a context of that value would."""
    rho = 0.622 * st["p"] / (287.04 * st["t"] * (st["qv"] + 0.622))
    st["nc"] = np.ascontiguousarray(np.asarray(values, dtype=np.float64)[:, None] * 1e6 / rho)
    return st


def _resample(col, nz):
    x0 = np.linspace(0.0, 1.0, col["qv"].shape[0])
    x1 = np.linspace(0.0, 1.0, nz)
    out = {k: np.interp(x1, x0, v) for k, v in col.items()}
    out["dz"] = np.full(nz, 15000.0 / nz)
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def _warm_batch(ncol, seed=7):
    """config-2 columns (cloud and rain present), each with its own cloud and rain content."""
    rng = np.random.Generator(np.random.PCG64(cases.SEED + seed))
    st = cases.config2(ncol)
    for k in ("qc", "qr", "nr"):
        st[k] *= rng.lognormal(0.0, 0.3, size=(ncol, 1))
    return st


def _batch(iiwarm, ncol, nz=cases.NZ, seed=7):
    """ncol columns of nz levels for the warm-rain / the mixed-phase context."""
    if nz == cases.NZ:
        return _warm_batch(ncol, seed) if iiwarm else cases.config3(ncol, seed=cases.SEED + seed)
    base = [kc.kat_a(False), kc.kat_c()] if iiwarm else [kc.kat_a(True), kc.kat_a(False), kc.kat_c()]
    cols = []
    for i in range(ncol):
        c = _resample(base[i % len(base)], nz)
        for k in ("qc", "qr", "qi", "qs", "qg"):
            c[k] = c[k] * (1.0 + 0.07 * i)
        if iiwarm:
            for k in ("qi", "qs", "qg", "ni"):
                c[k][:] = 0.0
        cols.append(c)
    return {k: np.ascontiguousarray(np.stack([c[k] for c in cols])) for k in cases.KEYS}


# ---- one step through every entry; everything that comes back, as numpy ----
def _step(m, st, entry, arith="p64", rates=False):
    import torch
    ncol, nz = st["qv"].shape
    if arith != "p64":
        st = {k: np.ascontiguousarray(v.astype(f32)) for k, v in st.items()}
    if entry == "device":
        dev = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
        ppt = torch.zeros(ncol, 4, dtype=dev["qv"].dtype, device="cuda")
        r = torch.zeros(ncol, 36, nz, dtype=torch.float64, device="cuda") if rates else None
        ns = torch.zeros(ncol, 4, dtype=torch.int32, device="cuda")
        if arith == "p64":
            m.batch_step(dev, 10.0, ppt, rates=r, nstep=ns)
        else:
            m.batch_step32(dev, 10.0, ppt, arith=arith, rates=r, nstep=ns)
        torch.cuda.synchronize()
        out = {k: dev[k].cpu().numpy() for k in OUT}
        out["ppt"], out["nstep"] = ppt.cpu().numpy(), ns.cpu().numpy()
        if rates:
            out["rates"] = r.cpu().numpy()
        return out
    got = _copy(st)
    if arith == "p64":
        from kid_amd.thompson import load_library
        L = load_library()                                    # (the Python host entry does not return nstep)
        dp = C.POINTER(C.c_double)
        ppt, ns = np.zeros((ncol, 4)), np.zeros((ncol, 4), dtype=np.int32)
        r = np.zeros((ncol, 36, nz)) if rates else None
        m._check(L.kidmp_batch_step_host_diag(m._h, ncol, nz, 10.0, *[got[k].ctypes.data_as(dp) for k in cases.KEYS],
                                              ppt.ctypes.data_as(dp), r.ctypes.data_as(dp) if rates else None,
                                              ns.ctypes.data_as(C.POINTER(C.c_int32))))
    else:
        ppt, r, ns = m.batch_step32_host(got, 10.0, arith=arith, want_rates=rates, want_nstep=True)
    out = {k: got[k] for k in OUT}
    out["ppt"], out["nstep"] = ppt, ns
    if rates:
        out["rates"] = r
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _assert_same_bits(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _take(res, idx):
    return {k: v[idx] for k, v in res.items()}


# ---- 1. identity with the scalar ----
@pytest.mark.parametrize("nz", [40, 120, 128, 200])          # NJ = 1, banded (CPW = 4), CPW = 1, tall
@pytest.mark.parametrize("iiwarm", [False, True], ids=["mixed", "warm"])
def test_uniform_binding_gives_the_bits_of_the_scalar(ctx, iiwarm, nz):
    m = ctx(iiwarm)
    ncol = 10                                                  # two full workgroups of 4 and a remainder
    st = _batch(iiwarm, ncol, nz)
    runs = [(e, a, r) for e in ("device", "host") for a in ("p64", "p32n", "f32") for r in (False, True)]
    for entry, arith, rates in runs:
        m.set_column_nc(None)
        assert m.column_nc_count == 0
        plain = _step(m, st, entry, arith, rates)
        m.set_column_nc(np.full(ncol, 100.0))
        assert m.column_nc_count == ncol
        bound = _step(m, st, entry, arith, rates)
        _assert_same_bits(plain, bound, (entry, arith, rates))
        assert np.abs(plain["qr"]).sum() > 0 and (not rates or np.abs(plain["rates"]).sum() > 0)


# ---- 2. identity with a context of that value ----
@pytest.mark.parametrize("X", [25.0, 50.0, 300.0, 1000.0])   # nu_c = 15, 15, 5, 3
@pytest.mark.parametrize("iiwarm", [False, True], ids=["mixed", "warm"])
def test_uniform_binding_gives_the_bits_of_a_context_of_that_value(ctx, iiwarm, X):
    import torch
    m, own = ctx(iiwarm), ctx(iiwarm, X, own=True)
    for st in (_batch(iiwarm, 37), _batch(iiwarm, 6, nz=200), cases.edge_cases()):
        ncol = st["qv"].shape[0]
        _own_defaults(st, np.full(ncol, X))
        m.set_column_nc(torch.full((ncol,), X, dtype=torch.float64, device="cuda"))      # a device array
        for entry, arith, rates in (("device", "p64", True), ("host", "p64", False), ("device", "p32n", False),
                                    ("host", "f32", False)):
            _assert_same_bits(_step(own, st, entry, arith, rates), _step(m, st, entry, arith, rates), (X, entry, arith))
    # and it is not the default's answer
    st = _own_defaults(_batch(iiwarm, 16), np.full(16, X))
    m.set_column_nc(None)
    assert not np.array_equal(_step(m, st, "device")["qr"], _step(own, st, "device")["qr"])


# ---- 3. the ensemble ----
def _ensemble(iiwarm, ncol=4096):
    return _batch(iiwarm, ncol, seed=11)


@pytest.mark.parametrize("iiwarm", [False, True], ids=["config3", "config2"])
def test_ensemble_cyclic_every_workgroup_holds_four_values(ctx, iiwarm):
    m = ctx(iiwarm)
    ncol = 4096
    values = np.array([CYCLE[c % 4] for c in range(ncol)])
    st = _own_defaults(_ensemble(iiwarm, ncol), values)
    m.set_column_nc(values)
    got = _step(m, st, "device", rates=True)
    for v in CYCLE:
        idx = np.flatnonzero(values == v)
        ref = _step(ctx(iiwarm, v, own=True), _subset(st, idx), "device", rates=True)
        _assert_same_bits(ref, _take(got, idx), v)
    # the members' droplet numbers matter: against the unbound step only the members at the context's own 100 keep their bits
    m.set_column_nc(None)
    plain = _step(m, st, "device", rates=True)
    for v in CYCLE:
        idx = np.flatnonzero(values == v)
        assert np.array_equal(_bits(plain["qr"][idx]), _bits(got["qr"][idx])) == (v == 100.0), v


@pytest.mark.parametrize("iiwarm", [False, True], ids=["config3", "config2"])
def test_ensemble_log_uniform_all_values_distinct(ctx, iiwarm):
    from kid_amd import ThompsonMP
    m = ctx(iiwarm)
    ncol = 4096
    rng = np.random.Generator(np.random.PCG64(cases.SEED + 31))
    values = np.exp(rng.uniform(np.log(25.0), np.log(1600.0), ncol))
    assert np.unique(values).size == ncol
    st = _own_defaults(_ensemble(iiwarm, ncol), values)
    m.set_column_nc(values)
    got = _step(m, st, "device")
    for c in rng.choice(ncol, 16, replace=False):
        own = ThompsonMP(iiwarm=iiwarm, set_Nc=float(values[c]))
        try:
            _assert_same_bits(_step(own, _subset(st, [c]), "device"), _take(got, [c]), (int(c), float(values[c])))
        finally:
            own.close()
    # the host pipeline cuts 4 096 columns into chunks and offsets into the bound buffer: the same bits
    m.set_host_chunk(1000)                                    # chunks that do not end on a workgroup of the whole batch
    try:
        _assert_same_bits(got, _step(m, st, "host"), "host pipeline")
    finally:
        m.set_host_chunk(0)


# ---- 4. against the oracle ----
def _p32n_stats(got, ref):
    def err(a, b, k):
        a, b = a.astype(np.float64), b.astype(np.float64)
        return np.abs(a - b) / np.maximum(np.abs(b), 1e4 * FLOORS[k])
    e = np.concatenate([err(got[k], ref[k], k).ravel() for k in OUT])
    return float(np.median(e)), float(np.quantile(e, 0.99))


def _against_oracles(ctx, oracle, iiwarm, values_cycle, ncol, **caps):
    m = ctx(iiwarm)
    values = np.array([values_cycle[c % len(values_cycle)] for c in range(ncol)])
    st = _own_defaults(_batch(iiwarm, ncol, seed=17), values)
    m.set_column_nc(values)
    got = _step(m, st, "device")
    got32 = _step(m, st, "host", arith="p32n")
    for v in values_cycle:
        idx = np.flatnonzero(values == v)
        o = oracle(iiwarm, v)
        sub = _subset(st, idx)
        assert_parity(o, sub, 10.0, {k: got[k][idx] for k in OUT}, got["ppt"][idx], **caps)
        # P32n against batch_step_p32n, at the bounds of test_gpu_precision.py
        ref = {k: np.ascontiguousarray(a.astype(f32)) for k, a in sub.items()}
        rppt = o.batch_step_p32n(ref, 10.0)
        med, q99 = _p32n_stats({k: got32[k][idx] for k in OUT}, ref)
        print("set_Nc %g p32n vs the p32n oracle: median %.1e q99 %.1e" % (v, med, q99))
        assert med < 3e-7 and q99 < 1e-4, (v, med, q99)
        pe = np.abs(got32["ppt"][idx].astype(np.float64) - rppt) / np.maximum(np.abs(rppt), 1e-8)
        assert float(pe.max()) < 1e-4, (v, float(pe.max()))
    return st, values


def test_warm_ensemble_against_the_oracle_of_each_value(ctx, oracle):
    st, values = _against_oracles(ctx, oracle, True, CYCLE, 64)
    # the oracle's own answers differ between the extremes, so the comparison above could fail
    one = _subset(st, np.flatnonzero(values == 100.0))
    lo, hi = _copy(one), _copy(one)
    oracle(True, 25.0).batch_step(lo, 10.0)
    oracle(True, 1000.0).batch_step(hi, 10.0)
    d = np.abs(lo["qr"] - hi["qr"]) / np.maximum(np.abs(hi["qr"]), 1e-8)
    print("oracle rain mass, set_Nc 25 against 1000: largest difference %.0f %%" % (100 * d.max()))
    assert d.max() > 0.10


@pytest.mark.slow
def test_mixed_ensemble_against_the_oracle_of_each_value(ctx, oracle):
    # (the config-3 profile keeps ~4 % of its levels on the M:3596 residue branch: the cap of test_config3_sample_one_step)
    _against_oracles(ctx, oracle, False, (100.0, 300.0), 128, max_branch_frac=6e-2)


# ---- 5. diagnostics ----
def _dev(st):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in st.items()}


def _np(t):
    return tuple(_np(x) for x in t) if isinstance(t, (tuple, list)) else (None if t is None else t.cpu().numpy())


def test_diagnostics_follow_the_binding(ctx, oracle):
    m = ctx(False)
    ncol = 64
    values = np.array([CYCLE[c % 4] for c in range(ncol)])
    st = _own_defaults(np_cat(cases.config3(48, seed=cases.SEED + 5), cases.config5(16, seed=cases.SEED + 6)), values)
    m.set_column_nc(values)
    dev = _dev(st)
    radii = _np(m.effective_radii(dev))
    dbz, fused = _np(m.column_outputs(dev))
    aer = _np(m.default_aerosols(dev["qv"], dev["t"], dev["p"]))
    refl = _np(m.reflectivity(dev))
    radii_host = m.effective_radii_host({k: st[k] for k in m.RADII_NAMES})
    radii_host32 = m.effective_radii_host({k: st[k].astype(f32) for k in m.RADII_NAMES})
    dev32 = {k: v.float() for k, v in dev.items()}
    dbz32, fused32 = _np(m.column_outputs(dev32))                          # the binary32 entry: binary64 arithmetic inside
    stepped = _copy(st)
    ppt, _, step_radii = m.batch_step_host(stepped, 10.0, want_radii=True)
    for v in CYCLE:
        idx = np.flatnonzero(values == v)
        own, sub = ctx(False, v, own=True), _subset(st, idx)
        sdev = _dev(sub)
        for a, b, what in zip(radii, _np(own.effective_radii(sdev)), ("re_qc", "re_qi", "re_qs")):
            assert np.array_equal(_bits(a[idx]), _bits(b)), (v, what)
        odbz, ofused = _np(own.column_outputs(sdev))
        assert np.array_equal(_bits(dbz[idx]), _bits(odbz)), v
        for a, b in zip(fused, ofused):
            assert np.array_equal(_bits(a[idx]), _bits(b)), v
        for a, b, what in zip(aer, _np(own.default_aerosols(sdev["qv"], sdev["t"], sdev["p"])), ("nc", "nwfa", "nifa")):
            assert np.array_equal(_bits(a[idx]), _bits(b)), (v, what)
        for a, b in zip(radii_host, own.effective_radii_host({k: sub[k] for k in m.RADII_NAMES})):
            assert np.array_equal(_bits(a[idx]), _bits(b)), v
        for a, b in zip(radii_host32, own.effective_radii_host({k: sub[k].astype(f32) for k in m.RADII_NAMES})):
            assert a.dtype == f32 and np.array_equal(_bits(a[idx]), _bits(b)), v
        ostepped = _copy(sub)
        oppt, _, ostep_radii = own.batch_step_host(ostepped, 10.0, want_radii=True)
        assert np.array_equal(_bits(ppt[idx]), _bits(oppt))
        for k in OUT:
            assert np.array_equal(_bits(stepped[k][idx]), _bits(ostepped[k])), (v, k)
        for a, b in zip(step_radii, ostep_radii):
            assert np.array_equal(_bits(a[idx]), _bits(b)), v
        odbz32, ofused32 = _np(own.column_outputs({k: t.float() for k, t in sdev.items()}))
        assert dbz32.dtype == f32 and np.array_equal(_bits(dbz32[idx]), _bits(odbz32)), v
        for a, b in zip(fused32, ofused32):
            assert a.dtype == f32 and np.array_equal(_bits(a[idx]), _bits(b)), v
        # calc_effectRad of the oracle at that value, at the bound of test_gpu_column_outputs.py (no table enters it)
        for a, r, what in zip(radii, oracle(True, v).calc_effectRad(sub), ("re_qc", "re_qi", "re_qs")):
            assert np.max(np.abs(a[idx] - r) / r) < 1e-12, (v, what)
        for a, r in zip(fused, oracle(True, v).calc_effectRad(sub)):
            assert np.max(np.abs(a[idx] - r) / r) < 1e-12, v
        for a, r in zip(step_radii, oracle(True, v).calc_effectRad(_subset(stepped, idx))):   # of the post-step state
            assert np.max(np.abs(a[idx] - r) / r) < 1e-12, v
    # calc_refl10cm does not read Nt_c; re_qc and nc = Nt_c/rho do
    m.set_column_nc(None)
    lo = np.flatnonzero(values == 25.0)
    assert not np.array_equal(radii[0][lo], _np(m.effective_radii(dev))[0][lo])
    assert not np.array_equal(aer[0][lo], _np(m.default_aerosols(dev["qv"], dev["t"], dev["p"]))[0][lo])
    assert np.array_equal(_bits(refl), _bits(_np(m.reflectivity(dev))))
    assert np.array_equal(_bits(dbz), _bits(_np(m.column_outputs(dev))[0]))


def np_cat(a, b):
    return {k: np.ascontiguousarray(np.concatenate([a[k], b[k]])) for k in cases.KEYS}


# ---- 6. refusals ----
def _refused(m, fn, *args, **kw):
    from kid_amd import KidmpError
    with pytest.raises(KidmpError, match=r"kidmp error -1:") as e:
        fn(*args, **kw)
    return str(e.value)


def test_refusals_leave_everything_untouched(ctx, gpu_mixed_aero):
    import torch
    from kid_amd import ThompsonMulti
    m = ctx(False)
    st = _batch(False, 12)
    plain = _step(m, st, "device")
    m.set_column_nc(np.full(7, 300.0))
    # count mismatch: device, host (all forms), binary32, one column, the column outputs
    dev = _dev(st)
    before = {k: v.clone() for k, v in dev.items()}
    ppt = torch.zeros(12, 4, dtype=torch.float64, device="cuda")
    assert "bound 7 columns" in _refused(m, m.batch_step, dev, 10.0, ppt)
    dev32 = {k: v.float() for k, v in dev.items()}
    assert "bound 7" in _refused(m, m.batch_step32, dev32, 10.0, ppt.float())
    assert "bound 7" in _refused(m, m.column_outputs, dev)
    torch.cuda.synchronize()
    for k in dev:
        assert torch.equal(dev[k], before[k]), k
    assert not ppt.any()
    host = _copy(st)
    for kw in ({}, {"want_dbz": True}, {"want_radii": True}, {"want_rates": True}):
        assert "bound 7" in _refused(m, m.batch_step_host, host, 10.0, **kw)
    host32 = {k: v.astype(f32) for k, v in st.items()}
    assert "bound 7" in _refused(m, m.batch_step32_host, host32, 10.0)
    col = {k: np.ascontiguousarray(v[0]) for k, v in st.items()}
    assert "bound 7" in _refused(m, m.mp_thompson, *[col[k] for k in cases.KEYS])
    for k in st:
        assert np.array_equal(host[k], st[k]) and np.array_equal(col[k], st[k][0]), k
    # n not a multiple of the count
    dev5 = {k: v[:5].contiguous() for k, v in dev.items()}                # 5 * 120 = 600 elements, 7 columns bound
    assert "multiple" in _refused(m, m.effective_radii, dev5)
    assert "multiple" in _refused(m, m.default_aerosols, dev5["qv"], dev5["t"], dev5["p"])
    assert "multiple" in _refused(m, m.effective_radii_host, {k: st[k][:5] for k in m.RADII_NAMES})
    assert "multiple" in _refused(m, m.effective_radii_host, {k: st[k][:5].astype(f32) for k in m.RADII_NAMES})
    # bad values: the first offending column is named and the previous binding stays
    for bad, where in ((0.0, 3), (-5.0, 0), (float("nan"), 7), (float("inf"), 5)):
        v = np.full(12, 100.0)
        v[where] = bad
        v[9] = bad
        assert "column %d " % where in _refused(m, m.set_column_nc, v)
        assert m.column_nc_count == 7
    # an aerosol-aware context
    assert "aerosol-aware" in _refused(gpu_mixed_aero, gpu_mixed_aero.set_column_nc, np.full(4, 100.0))
    assert gpu_mixed_aero.column_nc_count == 0
    # a multi handle one of whose contexts holds a binding
    mm = ThompsonMulti([0, 0], iiwarm=False)
    try:
        from kid_amd.thompson import load_library
        L = load_library()
        h = L.kidmp_multi_context(mm._h, 1)
        v = np.full(12, 100.0)
        assert L.kidmp_set_column_nc(h, 12, v.ctypes.data) == 0
        host = _copy(st)
        from kid_amd import KidmpError
        with pytest.raises(KidmpError, match=r"failed \(-1\).*kidmp_set_column_nc binding"):
            mm.batch_step_host(host, 10.0)
        for k in st:
            assert np.array_equal(host[k], st[k]), k
        assert L.kidmp_set_column_nc(h, 0, None) == 0
        mm.batch_step_host(host, 10.0)                                     # unbound again: it steps
    finally:
        mm.close()
    # unbinding restores the unbound bits
    m.set_column_nc(None)
    assert m.column_nc_count == 0
    _assert_same_bits(plain, _step(m, st, "device"))


# ---- 7. graph capture ----
def test_hip_graph_capture_of_bound_steps(ctx):
    """The bound step allocates nothing either: captured into a HIP graph and replayed it gives the bits of eager
    launches (as test_hip_graph_capture_of_steps for the plain step)."""
    import torch
    m = ctx(False)
    ncol = 76                                                 # no other test steps 76 columns
    values = np.array([CYCLE[c % 4] for c in range(ncol)])
    st = _own_defaults(cases.config3(ncol, seed=cases.SEED + 3), values)
    m.set_column_nc(values)
    graphed = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
    ppt_g = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(3):
            m.batch_step(graphed, 10.0, ppt_g)
    for k in graphed:                                          # capture does not execute: state still initial
        assert torch.equal(graphed[k].cpu(), torch.from_numpy(st[k]))
    g.replay()
    torch.cuda.synchronize()
    eager = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
    ppt_e = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda")
    for _ in range(3):
        m.batch_step(eager, 10.0, ppt_e)
    torch.cuda.synchronize()
    for k in cases.KEYS:
        assert torch.equal(graphed[k], eager[k]), k
    assert torch.equal(ppt_g, ppt_e)
    m.set_column_nc(None)
    plain = {k: torch.from_numpy(v).cuda() for k, v in st.items()}
    ppt_p = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda")
    for _ in range(3):
        m.batch_step(plain, 10.0, ppt_p)
    torch.cuda.synchronize()
    assert not torch.equal(plain["qr"], eager["qr"])           # and the binding mattered
