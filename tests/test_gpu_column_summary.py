"""The per-column summary on the MI355X (include/kidmp_summary.h, kidmp::k_column_summary): water paths, liquid cloud optical
depth, composite reflectivity, echo-top, cloud and freezing heights of a column from one read of its profiles.

Bounds (tests/column_summary_ref.py; none is a measured number): a summed slot and a height lie within
(nz + 4) * 2**-53 * sum|term| of math.fsum of the same terms, which numpy forms bit for bit; a dBZ slot against
tests/refl_oracle.py within BOUND_DB = 3e-13 dB; TAU_C against oracle radii adds BOUND_RE = 1e-12 relative to sum|term|;
everything else is equality of bits.  The tests print their measured maxima."""
import ctypes as C

import numpy as np
import pytest

import cases
import column_summary_ref as ref
import effrad_cases as ec
import refl_oracle as ro

pytestmark = pytest.mark.gpu

NZ_SWEEP = (2, 63, 64, 65, 120, 128, 129, 256)
NCOL_SWEEP = (1, 3, 4, 5, 9)
KEYS = ref.INPUTS + ("ni",)                        # ni: only the library's own radii entry reads it
EINVAL, ESTATE = -1, -5


def _uneven_dz(ncol, nz, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.ascontiguousarray(np.exp(rng.uniform(np.log(3.0), np.log(700.0), (ncol, nz))))


def _with_dz(st, seed):
    st = {k: np.ascontiguousarray(st[k]) for k in KEYS}
    st["dz"] = _uneven_dz(*st["t"].shape, seed)
    return st


def _own_dz(st):
    return {k: np.ascontiguousarray(st[k]) for k in KEYS + ("dz",)}


def _all_dry(ncol=8, nz=120):
    st = ec.random_state(nz, ncol, 31)
    for k in ("qc", "qi", "ni", "qr", "nr", "qs", "qg"):
        st[k][:] = 0.0
    return st


@pytest.fixture(scope="module")
def sets():
    """name -> state with its dz, built once and left unchanged."""
    return {
        "config3": _own_dz(cases.config3(96)),
        "config5": _own_dz(cases.config5(96)),                    # dz from 3 to 709 m
        "config2": _own_dz(cases.config2(64)),                    # no level below freezing: slot 14 is NaN
        "hand_built": _with_dz(ec.stack(ec.hand_built()), 41),
        "batch": _with_dz(ec.batch(), 42),
        "random65": _with_dz(ec.random_state(65, 96, 265), 43),
        "all_dry": _with_dz(_all_dry(), 44),
    }


@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = ro.constants(o)
    o.close()
    return c


@pytest.fixture(autouse=True)
def _leave_contexts_as_found(gpu_mixed, gpu_warm):
    yield
    for m in (gpu_mixed, gpu_warm):
        m.set_column_nc(None)
        m.set_host_chunk(0)


def _dev(st, dtype=None, keys=ref.INPUTS):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(st[k] if dtype is None else st[k].astype(dtype))).to("cuda:0")
            for k in keys if st.get(k) is not None}


def _summary(m, st, dz=None, dtype=None, **kw):
    import torch
    dz = st["dz"] if dz is None else dz
    dz = torch.from_numpy(np.ascontiguousarray(dz if dtype is None else dz.astype(dtype))).to("cuda:0")
    out = m.column_summary(_dev(st, dtype), dz, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _own_profiles(m, st):
    """dBZ, re_qc and its formed mask as the library's own entries give them."""
    import torch
    dev = _dev(st, keys=KEYS)
    dbz = m.reflectivity(dev).cpu().numpy()
    re = m.effective_radii(dev)[0].cpu().numpy()
    torch.cuda.synchronize()
    return dbz, re, re != ref.RE_QC_PRESET


def _take(st, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}


# ---- 1. against the library's own profiles: exact in every decision ----
@pytest.mark.parametrize("ctx", ["mixed", "aero"])
@pytest.mark.parametrize("name", ["config3", "config5", "config2", "hand_built", "batch", "random65", "all_dry"])
def test_against_the_librarys_own_profiles(request, sets, name, ctx):
    m = request.getfixturevalue("gpu_mixed" if ctx == "mixed" else "gpu_mixed_aero")
    st = sets[name]
    nz = st["t"].shape[1]
    dbz, re, formed = _own_profiles(m, st)
    want, mag, k = ref.summary(st, st["dz"], dbz, re, formed)
    got = _summary(m, st)
    worst = ref.check(got, want, mag, nz)                     # slots 7 and 10: bits; levels: through their heights and NaNs
    print("summary %s (%s): worst error %.3f of its bound; levels chosen %s" % (name, ctx, worst, [sorted({int(x) for x in k[:, i]})[:3] for i in range(5)]))
    if name == "config2":
        assert np.isnan(got[:, ref.Z_FREEZE]).all()
    if name == "all_dry":
        assert np.isnan(got[:, [ref.Z_ECHO_TOP, ref.Z_CLOUD_BASE, ref.Z_CLOUD_TOP]]).all() and not got[:, ref.N_CLOUD].any()
        assert not got[:, [ref.CWP, ref.RWP, ref.IWP, ref.SWP, ref.GWP, ref.TAU_C]].any() and (got[:, ref.WVP] > 0).all()
        assert (got[:, ref.Z_DBZ_MAX] == 0.5 * st["dz"][:, 0]).all()


# ---- 2. against the independent oracles ----
@pytest.mark.parametrize("ctx", ["mixed", "aero"])
def test_against_the_oracles(request, sets, consts, ctx):
    m = request.getfixturevalue("gpu_mixed" if ctx == "mixed" else "gpu_mixed_aero")
    o = request.getfixturevalue("oracle_mixed" if ctx == "mixed" else "oracle_mixed_aero")
    for name, st in sets.items():
        nz = st["t"].shape[1]
        dbz = ref.oracle_dbz(consts, st)
        re, formed = ref.oracle_re_qc(o, st)
        want, mag, _ = ref.summary(st, st["dz"], dbz, re, formed)
        skip = ref.undecidable(dbz)
        assert skip.mean() <= 0.01, (name, skip.mean())
        got = _summary(m, st)
        worst = ref.check(got, want, mag, nz, extra_tau=ref.BOUND_RE, db_bound=ref.BOUND_DB, skip_levels=skip)
        print("summary vs oracles %s (%s): %d undecidable, worst error %.3g of its bound, max |ddBZ| %.3g"
              % (name, ctx, skip.sum(), worst, np.max(np.abs(got[:, [7, 10]] - want[:, [7, 10]]))))


# ---- 3. nz and ncol sweeps ----
@pytest.mark.parametrize("nz", NZ_SWEEP)
def test_nz_sweep(gpu_mixed, nz):
    st = _with_dz(ec.random_state(nz, 24, 300 + nz), 500 + nz)
    dbz, re, formed = _own_profiles(gpu_mixed, st)
    want, mag, _ = ref.summary(st, st["dz"], dbz, re, formed)
    print("summary nz=%d: worst error %.3f of its bound" % (nz, ref.check(_summary(gpu_mixed, st), want, mag, nz)))
    st32 = {k: v[:5].astype(np.float32) for k, v in st.items()}                    # binary32 storage at every level-group count
    assert _same(_summary(gpu_mixed, st32), _summary(gpu_mixed, {k: v.astype(np.float64) for k, v in st32.items()}))


@pytest.mark.parametrize("ncol", NCOL_SWEEP)
def test_ncol_sweep(gpu_mixed, sets, ncol):
    st = _take(sets["config3"], slice(0, ncol))
    dbz, re, formed = _own_profiles(gpu_mixed, st)
    want, mag, _ = ref.summary(st, st["dz"], dbz, re, formed)
    got = _summary(gpu_mixed, st)
    ref.check(got, want, mag, 120)
    assert _same(got, _summary(gpu_mixed, sets["config3"])[:ncol])


# ---- 4. equalities of bits ----
def test_bit_equalities(gpu_mixed, sets):
    m = gpu_mixed
    for name in ("config5", "random65", "hand_built"):
        st = sets[name]
        ncol = st["t"].shape[0]
        whole = _summary(m, st)
        assert _same(whole, _summary(m, st)), "a repeated call"
        for c in (0, 1, 5, ncol - 1):                          # alone, and at another position in another batch
            assert _same(_summary(m, _take(st, [c])), whole[c:c + 1]), (name, c)
        idx = np.arange(ncol)[::-1].copy()
        assert _same(_summary(m, _take(st, idx)), whole[idx])
        one = np.ascontiguousarray(st["dz"][3])
        assert _same(_summary(m, st, dz=one), _summary(m, st, dz=np.ascontiguousarray(np.broadcast_to(one, st["dz"].shape)))), "dz_col_stride 0"
        assert _same(whole, _summary(m, st, cfg=(18.0, 1.0e-5, 273.15))), "cfg NULL"
        assert _same(whole, _summary(m, st, cfg={"dbz_echo": 18.0, "q_cloud": 1.0e-5, "t_freeze": 273.15}))
        st32 = {k: v.astype(np.float32) for k, v in st.items()}
        wide = {k: v.astype(np.float64) for k, v in st32.items()}
        assert _same(_summary(m, st32), _summary(m, wide)), "kidmp32 on float32 = kidmp on the widened arrays"
        assert _same(_summary(m, st32, dz=st32["dz"][3].copy()), _summary(m, wide, dz=wide["dz"][3].copy()))


def test_out_argument_and_stream(gpu_mixed, sets):
    import torch
    st = sets["config3"]
    out = torch.full((96, 16), -7.0, dtype=torch.float64, device="cuda:0")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        r = gpu_mixed.column_summary(_dev(st), torch.from_numpy(st["dz"]).cuda(), out=out)
    s.synchronize()
    assert r is out and _same(out.cpu().numpy(), _summary(gpu_mixed, st))


# ---- 5. warm context ----
def test_warm_context_left_out_species_are_zeros(gpu_warm, sets):
    st = sets["config2"]
    zeros = dict(st, qi=np.zeros_like(st["t"]), qs=np.zeros_like(st["t"]), qg=np.zeros_like(st["t"]))
    left_out = {k: v for k, v in st.items() if k not in ("qi", "qs", "qg", "nc")}
    a, b = _summary(gpu_warm, zeros), _summary(gpu_warm, left_out)
    assert _same(a, b)
    assert np.array_equal(a[:, 3:6].view(np.uint64), np.zeros((64, 3), dtype=np.uint64))          # +0.0
    assert (a[:, ref.CWP] > 0).all() and (a[:, ref.TAU_C] > 0).all()
    dbz, re, formed = _own_profiles(gpu_warm, zeros)
    want, mag, _ = ref.summary(zeros, st["dz"], dbz, re, formed)
    ref.check(a, want, mag, 120)


# ---- 6. per-column droplet number ----
def test_per_column_droplet_number(gpu_warm, sets):
    from kid_amd import KidmpError, ThompsonMP
    m = gpu_warm
    st = _take(sets["config2"], slice(0, 10))
    lo, hi = 50.0, 300.0
    own = {v: ThompsonMP(iiwarm=True, set_Nc=v) for v in (lo, hi)}
    try:
        want = {v: _summary(own[v], st) for v in (lo, hi)}
        for v in (lo, hi):
            m.set_column_nc(np.full(10, v))
            assert _same(_summary(m, st), want[v]), "a uniform binding = a context of that value"
        values = np.array([lo, hi] * 5)
        m.set_column_nc(values)
        got = _summary(m, st)
        assert _same(got, np.where((values == lo)[:, None], want[lo], want[hi]))
        assert (want[lo][:, ref.TAU_C] != want[hi][:, ref.TAU_C]).all() and _same(want[lo][:, ref.CWP].copy(), want[hi][:, ref.CWP].copy())
        sentinel = None
        with pytest.raises(KidmpError, match="bound 10 columns"):
            sentinel = _summary(m, _take(st, slice(0, 9)))
        assert sentinel is None
        with pytest.raises(KidmpError, match="bound 10 columns"):
            m.column_summary_host(_take(st, slice(0, 9)), st["dz"][:9].copy())
        m.set_host_chunk(4)                                   # chunks take their share of the binding
        assert _same(m.column_summary_host({k: st[k] for k in ref.INPUTS}, st["dz"]), got)
    finally:
        for o in own.values():
            o.close()


# ---- 7. thresholds ----
def test_thresholds(gpu_mixed, sets):
    st = sets["config3"]
    base = _summary(gpu_mixed, st)
    assert np.isfinite(base[:, ref.Z_ECHO_TOP]).any()
    high = _summary(gpu_mixed, st, cfg=(base[:, ref.DBZ_MAX].max() + 1.0, 1.0e-5, 273.15))
    assert np.isnan(high[:, ref.Z_ECHO_TOP]).all()
    keep = [s for s in range(16) if s != ref.Z_ECHO_TOP]
    assert _same(high[:, keep].copy(), base[:, keep].copy())
    at_max = _summary(gpu_mixed, st, cfg=(float(base[0, ref.DBZ_MAX]), 1.0e-5, 273.15))             # >= : the level of the maximum counts
    assert np.isfinite(at_max[0, ref.Z_ECHO_TOP])
    for name in ("config3", "hand_built"):                    # hand_built: sweeps of qc and qi from 1e-12 up
        any_q = _summary(gpu_mixed, sets[name], cfg=(18.0, 0.0, 273.15))
        assert np.array_equal(any_q[:, ref.N_CLOUD], ((sets[name]["qc"] + sets[name]["qi"]) > 0.0).sum(axis=1).astype(np.float64))
    assert (any_q[:, ref.N_CLOUD] > _summary(gpu_mixed, sets["hand_built"])[:, ref.N_CLOUD]).any()
    dbz, re, formed = _own_profiles(gpu_mixed, st)
    cfg = (5.0, 3.0e-4, 260.0)
    want, mag, _ = ref.summary(st, st["dz"], dbz, re, formed, cfg)
    ref.check(_summary(gpu_mixed, st, cfg=cfg), want, mag, 120)


# ---- 8. refusals ----
HOST = "a pageable host array"


def test_refusals_write_nothing(gpu_mixed, gpu_mixed_aero, gpu_warm, sets):
    import torch
    from kid_amd.summary import _SummaryCfg, library
    L = library()
    st = _take(sets["config3"], slice(0, 6))
    ncol, nz = 6, 120
    dev = {False: dict(_dev(st), dz=torch.from_numpy(st["dz"]).cuda())}
    dev[True] = {k: v.float() for k, v in dev[False].items()}
    host = {False: torch.zeros(ncol, nz, dtype=torch.float64), True: torch.zeros(ncol, nz, dtype=torch.float32)}
    out = torch.full((ncol, 16), -7.0, dtype=torch.float64, device="cuda:0")
    good = torch.empty_like(out)

    def call(m, f32=False, ncol=ncol, nz=nz, stride=nz, cfg=None, out=out, **over):
        p = {k: v.data_ptr() for k, v in dev[f32].items()}
        p.update({k: host[f32].data_ptr() if v is HOST else v for k, v in over.items()})
        c = _SummaryCfg(*cfg) if cfg is not None else None
        fn = L.kidmp32_column_summary_device if f32 else L.kidmp_column_summary_device
        return fn(m._h if m is not None else None, ncol, nz, *[p[k] for k in ref.INPUTS], p["dz"], stride,
                  C.byref(c) if c is not None else None, out.data_ptr() if out is not None else None, None)

    nan, inf = float("nan"), float("inf")
    refused = [
        dict(t=None), dict(p=None), dict(qv=None), dict(qc=None), dict(qr=None), dict(nr=None), dict(dz=None), dict(out=None),
        dict(qi=None), dict(qs=None), dict(qg=None), dict(qs=None, qg=None),                       # required in a mixed-phase context
        dict(nz=1), dict(nz=257), dict(ncol=-1), dict(stride=nz - 1), dict(stride=-nz), dict(stride=1),
        dict(cfg=(nan, 1e-5, 273.15)), dict(cfg=(18.0, inf, 273.15)), dict(cfg=(18.0, 1e-5, -inf)),
        dict(t=HOST), dict(qg=HOST), dict(dz=HOST),
    ]
    for f32 in (False, True):
        for kw in refused:
            assert call(gpu_mixed, f32, **kw) == EINVAL, (f32, kw)
        assert call(gpu_mixed_aero, f32, nc=None) == EINVAL                                    # nc: required where the context is aerosol-aware
        assert call(gpu_warm, f32, qs=None) == EINVAL                                          # qs and qg: together or not at all
        assert call(None, f32) == ESTATE
    assert L.kidmp_column_summary_device(gpu_mixed._h, ncol, nz, *[dev[False][k].data_ptr() for k in ref.INPUTS], dev[False]["dz"].data_ptr(),
                                         nz, None, host[False].data_ptr(), None) == EINVAL      # summary in host memory
    gpu_mixed.set_column_nc(np.full(ncol + 1, 100.0))
    assert call(gpu_mixed) == EINVAL                                                           # ncol is not the bound count
    gpu_mixed.set_column_nc(None)
    assert call(gpu_mixed, ncol=0) == 0 and call(gpu_mixed, ncol=0, t=None, dz=None, out=None) == 0
    # the host entries refuse alike
    hst = {k: st[k] for k in ref.INPUTS}
    hout = np.full((ncol, 16), -7.0)

    def hcall(m, ncol=ncol, nz=nz, stride=nz, cfg=None, **over):
        p = {k: hst[k].ctypes.data for k in ref.INPUTS}
        p.update(dz=st["dz"].ctypes.data, out=hout.ctypes.data)
        p.update(over)
        c = _SummaryCfg(*cfg) if cfg is not None else None
        return L.kidmp_column_summary_host(m._h if m is not None else None, ncol, nz, *[p[k] for k in ref.INPUTS], p["dz"], stride,
                                           C.byref(c) if c is not None else None, p["out"])

    for kw in (dict(t=None), dict(qi=None), dict(dz=None), dict(out=None), dict(nz=1), dict(nz=257), dict(ncol=-1), dict(stride=nz - 1),
               dict(cfg=(nan, 1e-5, 273.15))):
        assert hcall(gpu_mixed, **kw) == EINVAL, kw
    assert hcall(None) == ESTATE and hcall(gpu_mixed, ncol=0) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (hout == -7.0).all()                          # nothing was written
    # good calls afterwards still work
    want = _summary(gpu_mixed, st)
    assert call(gpu_mixed, out=good) == 0 and hcall(gpu_mixed) == 0
    torch.cuda.synchronize()
    assert _same(good.cpu().numpy(), want) and _same(hout, want)
    assert call(gpu_mixed, nc=None, out=good) == 0 and call(gpu_warm, qi=None, qs=None, qg=None, nc=None, out=good) == 0
    torch.cuda.synchronize()


# ---- 9. host entries ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_entries_equal_the_device_entry(gpu_mixed, dtype):
    m = gpu_mixed
    st = _own_dz(cases.config3(100, seed=cases.SEED + 5))
    st = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in st.items()}
    st["dz"] = np.ascontiguousarray((st["dz"] * np.linspace(0.5, 2.0, 100)[:, None]).astype(dtype))   # a dz of its own per column
    want = _summary(m, st)
    hst = {k: st[k] for k in ref.INPUTS}
    for chunk in (0, 16):
        m.set_host_chunk(chunk)
        assert _same(m.column_summary_host(hst, st["dz"]), want), chunk
        assert _same(m.column_summary_host(hst, st["dz"][7].copy()), _summary(m, st, dz=st["dz"][7].copy())), chunk
        wide = np.ascontiguousarray(np.concatenate([st["dz"], st["dz"][:, :5]], axis=1))        # dz_col_stride = nz + 5
        from kid_amd.summary import library
        out = np.empty((100, 16))
        fn = library().kidmp_column_summary_host if dtype == np.float64 else library().kidmp32_column_summary_host
        assert fn(m._h, 100, 120, *[hst[k].ctypes.data for k in ref.INPUTS], wide.ctypes.data, 125, None, out.ctypes.data) == 0
        assert _same(out, want), ("stride", chunk)
    m.set_host_chunk(1)                                       # seven columns, one per chunk
    st7 = {k: np.ascontiguousarray(v[:7]) for k, v in st.items()}
    assert _same(m.column_summary_host({k: st7[k] for k in ref.INPUTS}, st7["dz"]), _summary(m, st7))


# ---- 10. KiD workspace ----
def test_summary_of_the_kid_workspace(gpu_mixed):
    import torch
    P0, R_ON_CP, DT = 1.0e5, 287.058 / 1005.0, 10.0
    m, ncol, nz = gpu_mixed, 24, 120
    st = cases.config3(ncol, seed=cases.SEED + 7)
    exner = (st["p"] / P0) ** R_ON_CP
    F = {k: st[k] for k in ("qv", "qc", "qr", "nr", "qi", "ni", "qs", "qg")}
    F["theta"] = st["t"] / exner
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    r = m.kid_interface({k: cu(v) for k, v in F.items()}, DT, P0, R_ON_CP, cu(exner), cu(st["dz"][0]))
    torch.cuda.synchronize()
    v = m.kid_workspace_views(r["work"], ncol, nz, torch.float64)
    assert v["dz"].stride(0) == nz
    got = m.column_summary({k: v[k] for k in ref.INPUTS}, v["dz"])
    post = {k: v[k].clone() for k in ref.INPUTS}
    direct = m.column_summary(post, cu(st["dz"][0]))
    torch.cuda.synchronize()
    assert _same(got.cpu().numpy(), direct.cpu().numpy())
    assert not _same(direct.cpu().numpy(), _summary(m, st))   # the step changed the state


# ---- 11. into level_stats ----
def test_summary_as_a_field_of_level_stats(gpu_mixed, sets):
    import torch
    st = sets["batch"]                                        # a few columns without an echo, a few without cloud: NaN slots
    s = gpu_mixed.column_summary(_dev(st), torch.from_numpy(st["dz"]).cuda())
    r = gpu_mixed.level_stats({"summary": s})                 # nz = 16, col_stride = 16
    torch.cuda.synchronize()
    a = s.cpu().numpy()
    assert np.isnan(a).any() and np.isfinite(a[:, ref.Z_ECHO_TOP]).any()
    assert np.array_equal(r.count[0, 0].cpu().numpy(), (~np.isnan(a)).sum(axis=0).astype(np.float64))
    some = (~np.isnan(a)).any(axis=0)
    assert np.array_equal(r.min[0, 0].cpu().numpy()[some], np.nanmin(a[:, some], axis=0))
    assert np.array_equal(r.max[0, 0].cpu().numpy()[some], np.nanmax(a[:, some], axis=0))
