"""The Doppler moments on the MI355X (include/kidmp_doppler.h, kidmp::k_doppler_moments) against tests/doppler_ref.py.

Bounds (none is a measured number): dbz and dbz_x within BOUND_DB = 3e-13 dB (the bound of test_gpu_reflectivity.py);
vz_x within BOUND = 1e-12 relative, the project's bound for this class of arithmetic: a few fastmath calls of 1-3.5 ulp,
raised to powers up to about 7; vd within BOUND * (V + |w|), the size of what is subtracted; sw through its square,
|sw**2 - ref**2| <= 4 BOUND m2: m2 - V**2 cancels up to ~100x for rain near 2.5 mm, so the bound is on the variance at
the scale of what is subtracted.  Everything else is an equality of bits.  The tests print their measured maxima."""
import ctypes as C

import numpy as np
import pytest

import cases
import doppler_ref as ref
import effrad_cases as ec
import fall_cases as fc

pytestmark = pytest.mark.gpu

BOUND = 1e-12
BOUND_DB = 3e-13
NZ_SWEEP = (2, 63, 64, 65, 120, 128, 129, 256)
NCOL_SWEEP = (1, 3, 4, 5, 9)
EINVAL, ESTATE = -1, -5
SET_NAMES = ["config3", "config5", "config2", "hand_built", "random65_365", "random65_366"]


def only(st):
    return {k: np.ascontiguousarray(st[k]) for k in ref.INPUTS}


@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = ref.constants(o)
    o.close()
    return c


@pytest.fixture(scope="module")
def sets():
    """name -> (state, w, warm), built once and left unchanged."""
    s = {
        "config3": (only(cases.config3(96)), False),
        "config5": (only(cases.config5(96)), False),
        "config2": (only(cases.config2(64)), True),
        "hand_built": (only(ec.stack(ec.hand_built())), False),
    }
    for seed in (365, 366):
        s["random65_%d" % seed] = (only(ec.random_state(65, 96, seed)), False)
    rng = np.random.Generator(np.random.PCG64(2025))
    return {k: (st, np.ascontiguousarray(rng.uniform(-6.0, 6.0, st["t"].shape)), warm) for k, (st, warm) in s.items()}


@pytest.fixture(scope="module")
def refs(sets, consts):
    return {k: ref.doppler_moments(consts, st, w) for k, (st, w, _) in sets.items()}


@pytest.fixture(autouse=True)
def _leave_contexts_as_found(gpu_mixed, gpu_warm):
    yield
    for m in (gpu_mixed, gpu_warm):
        m.set_host_chunk(0)


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _dev(st, dtype=None):
    return {k: _cu(v if dtype is None else v.astype(dtype)) for k, v in st.items() if v is not None}


def _doppler(m, st, w=None, dtype=None, **kw):
    import torch
    out = m.doppler_moments(_dev(st, dtype), None if w is None else _cu(w if dtype is None else w.astype(dtype)), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_all(a, b):
    return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)


def _take(st, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}


def check_parity(got, want):
    """Asserts the bounds of the module docstring; returns the measured maxima, each relative to its bound's scale (dB for
    the reflectivities)."""
    worst = {}
    for n in ref.NAMES:
        assert np.isfinite(got[n]).all(), n
    for n in ("dbz", "dbz_r", "dbz_s", "dbz_g"):
        err = np.abs(got[n] - want[n])
        worst[n] = float(err.max())
        assert (err <= BOUND_DB).all(), (n, worst[n])
    scales = {"vz_r": np.abs(want["vz_r"]), "vz_s": np.abs(want["vz_s"]), "vz_g": np.abs(want["vz_g"]),
              "vd": want["V"] + np.abs(want["w"])}
    for n, scale in scales.items():
        err = np.abs(got[n] - want[n])
        worst[n] = float(np.max(np.where(scale > 0, err / np.maximum(scale, 1e-300), 0.0)))
        assert (err <= BOUND * scale).all(), (n, worst[n])
    err = np.abs(got["sw"] ** 2 - want["sw"] ** 2)
    worst["sw"] = float(np.max(np.where(want["m2"] > 0, err / np.maximum(want["m2"], 1e-300), 0.0)))
    assert (err <= 4 * BOUND * want["m2"]).all(), ("sw", worst["sw"])
    return worst


def check_zeros(got, want):
    """Absent species and empty levels are +0.0 (no inheritance, w not applied)."""
    for x in "rsg":
        assert not _bits(got["vz_" + x])[~want["present_" + x]].any(), x
        assert (got["vz_" + x][want["present_" + x]] > 0).all(), x
        assert (got["dbz_" + x][~want["present_" + x]] == -40.0).all(), x
    empty = ~(want["present_r"] | want["present_s"] | want["present_g"])
    assert not _bits(got["vd"])[empty].any() and not _bits(got["sw"])[empty].any()


# ---- 1. parity and the equalities of bits on the sets ----
@pytest.mark.parametrize("name", SET_NAMES)
def test_parity_and_bits(request, sets, refs, consts, name):
    import torch
    st, w, warm = sets[name]
    m = request.getfixturevalue("gpu_warm" if warm else "gpu_mixed")
    got = _doppler(m, st, w)
    worst = check_parity(got, refs[name])
    print("doppler %s: max error (dB; relative to scale) %s" % (name, {k: "%.2e" % v for k, v in worst.items()}))
    check_zeros(got, refs[name])
    still = _doppler(m, st)                                   # w = None
    check_parity(still, ref.doppler_moments(consts, st))
    assert _same_all(still, _doppler(m, st, np.zeros_like(w))), "w = None is w = 0"
    for n in ref.NAMES:
        if n != "vd":
            assert _same(got[n], still[n]), (n, "w does not enter")
    dev = _dev(st)
    dbz = m.reflectivity(dev)
    torch.cuda.synchronize()
    assert _same(got["dbz"], dbz.cpu().numpy()), "dbz is kidmp_reflectivity_device's"
    if name != "hand_built":
        assert all(refs[name]["present_" + x].any() for x in ("r" if warm else "rsg")), name
        assert (got["sw"] > 0).any() and (got["vd"] != still["vd"]).any()


# ---- 2. shapes where the scan can go wrong ----
def _scan_state(nz):
    st = only(fc.scan_state(nz, 12, 900 + nz))
    for k in ("qr", "qs", "qg"):
        st[k][6:8] = 0.0
    st["qg"][7, nz - 1] = 5.0e-4                              # 7: graupel only at the top level, rain only at level 0
    st["qr"][7, 0] = 1.0e-3
    st["qg"][6, 0] = 5.0e-4                                   # 6: graupel only at level 0: the minimum of all the levels above
    st["qr"][6, 1:] = 1.0e-3                                  #    with (partly supercooled) rain over it
    return st


@pytest.mark.parametrize("nz", NZ_SWEEP)
def test_scan_shapes(gpu_mixed, consts, nz):
    m = gpu_mixed
    whole_st = _scan_state(nz)
    w = np.ascontiguousarray(np.linspace(-3.0, 3.0, 12 * nz).reshape(12, nz))
    whole = _doppler(m, whole_st, w)
    want = ref.doppler_moments(consts, whole_st, w)
    check_parity(whole, want)
    check_zeros(whole, want)
    assert whole["vz_g"][7, nz - 1] > 0 and not whole["vz_g"][7, :nz - 1].any()
    assert whole["vz_r"][7, 0] > 0 and not whole["vz_r"][7, 1:].any()
    assert whole["vz_g"][6, 0] > 0 and not whole["vz_g"][6, 1:].any()
    assert not any(whole[n][-1].any() for n in ("vd", "sw", "vz_r", "vz_s", "vz_g"))          # the column with none
    assert _same_all(whole, _doppler(m, whole_st, w)), "a repeated call"
    for ncol in NCOL_SWEEP:
        idx = (np.arange(ncol) * 5 + nz) % 12                                    # other positions in another batch
        part = _doppler(m, _take(whole_st, idx), np.ascontiguousarray(w[idx]))
        assert _same_all(part, {k: v[idx] for k, v in whole.items()}), (nz, ncol)
    for c in (0, 6, 7, 11):
        assert _same_all(_doppler(m, _take(whole_st, [c]), w[c:c + 1].copy()), {k: v[c:c + 1] for k, v in whole.items()}), c


# ---- 3. subsets, sentinels, qs / qg left out ----
def test_subsets_and_sentinels(gpu_mixed, sets):
    import torch
    m = gpu_mixed
    st, w, _ = sets["random65_365"]
    full = _doppler(m, st, w)
    for want_names in (("vd",), ("dbz", "vd", "sw"), ("vz_r", "vz_s", "vz_g"), ("sw", "dbz_g"), "dbz", ref.NAMES[::-1]):
        part = _doppler(m, st, w, want=want_names)
        names = (want_names,) if isinstance(want_names, str) else want_names
        assert sorted(part) == sorted(names)
        assert all(_same(part[n], full[n]) for n in names), want_names
    # a profile that was not requested is untouched: the raw entry on sentinel-filled arrays
    from kid_amd.doppler import _DopplerOut, library
    dev = _dev(st)
    dw = _cu(w)
    outs = {n: torch.full_like(dev["t"], -7.0) for n in ref.NAMES}
    asked = ("vd", "dbz_s")
    o = _DopplerOut(**{n: outs[n].data_ptr() for n in asked})
    rc = library().kidmp_doppler_moments_device(m._h, 96, 65, *[dev[k].data_ptr() for k in ref.INPUTS], dw.data_ptr(), C.byref(o), None)
    torch.cuda.synchronize()
    assert rc == 0
    for n in ref.NAMES:
        a = outs[n].cpu().numpy()
        assert _same(a, full[n]) if n in asked else (a == -7.0).all(), n
    # qs and qg left out mean zero, in a mixed-phase context too
    zero = dict(st, qs=np.zeros_like(st["qs"]), qg=np.zeros_like(st["qg"]))
    left_out = {k: v for k, v in st.items() if k not in ("qs", "qg")}
    assert _same_all(_doppler(m, zero, w), _doppler(m, left_out, w))
    no_g = _doppler(m, dict(st, qg=None), w)
    assert _same_all(no_g, _doppler(m, dict(st, qg=np.zeros_like(st["qg"])), w)) and not no_g["vz_g"].any()


# ---- 4. binary32 entries ----
def test_binary32_entries_round_once(gpu_mixed, gpu_warm, sets):
    scans = {"scan%d" % nz: (_take(_scan_state(nz), np.arange(5)), np.linspace(-3.0, 3.0, 5 * nz).reshape(5, nz))
             for nz in (2, 129, 256)}                                                # one, three and four level groups
    for name, m in (("config3", gpu_mixed), ("random65_366", gpu_mixed), ("config2", gpu_warm)) + tuple((n, gpu_mixed) for n in scans):
        st0, w0 = scans[name] if name in scans else sets[name][:2]
        st = {k: v.astype(np.float32) for k, v in st0.items()}
        w = np.ascontiguousarray(w0.astype(np.float32))
        wide = {k: v.astype(np.float64) for k, v in st.items()}
        got = _doppler(m, st, w)
        ref64 = _doppler(m, wide, w.astype(np.float64))
        for n in ref.NAMES:
            assert got[n].dtype == np.float32 and _same(got[n], ref64[n].astype(np.float32)), (name, n)


# ---- 5. host entries ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_entries_equal_the_device_entry(gpu_mixed, sets, dtype):
    m = gpu_mixed
    st = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in sets["random65_365"][0].items()}
    w = np.ascontiguousarray(sets["random65_365"][1].astype(dtype))
    ncol = st["t"].shape[0]
    want_w, want_still = _doppler(m, st, w), _doppler(m, st, want=("vd", "sw", "dbz"))
    for chunk in (0, 1, 7, ncol):
        m.set_host_chunk(chunk)
        assert _same_all(m.doppler_moments_host(st, w), want_w), chunk
        assert _same_all(m.doppler_moments_host(st, want=("vd", "sw", "dbz")), want_still), chunk
    m.set_host_chunk(7)
    few = m.doppler_moments_host({k: v for k, v in st.items() if k != "qs"}, w, want=("vd",))
    assert sorted(few) == ["vd"] and _same(few["vd"], _doppler(m, dict(st, qs=None), w)["vd"])


# ---- 6. graph capture ----
def test_hip_graph_capture_step_doppler_level_stats(gpu_mixed):
    """Step, then doppler_moments, then level_stats on dbz and vd, captured once and replayed twice, gives the eager bits."""
    import torch
    m, ncol = gpu_mixed, 52
    st = cases.config3(ncol, seed=cases.SEED + 14)

    def run(dev, ppt):
        m.batch_step(dev, 10.0, ppt)
        d = m.doppler_moments({k: dev[k] for k in ref.INPUTS}, dev["w"])
        return d, m.level_stats({"dbz": d["dbz"], "vd": d["vd"]})

    graphed = {k: _cu(v) for k, v in st.items()}
    ppt_g = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d_g, s_g = run(graphed, ppt_g)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    eager = {k: _cu(v) for k, v in st.items()}
    ppt_e = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda")
    for _ in range(2):
        d_e, s_e = run(eager, ppt_e)
    torch.cuda.synchronize()
    for n in ref.NAMES:
        assert torch.equal(d_g[n], d_e[n]), n
    assert _same(s_g.mom.cpu().numpy(), s_e.mom.cpu().numpy())
    assert (d_e["sw"] > 0).any() and (d_e["vz_r"] > 0).any()


# ---- 7. refusals ----
HOST = "a pageable host array"


def test_refusals_write_nothing(gpu_mixed, gpu_warm, sets):
    import torch
    from kid_amd.doppler import _DopplerOut, library
    L = library()
    st = _take(sets["config3"][0], slice(0, 6))
    w_np = np.ascontiguousarray(sets["config3"][1][:6])
    ncol, nz = 6, 120
    dev = {False: dict(_dev(st), w=_cu(w_np))}
    dev[True] = {k: v.float() for k, v in dev[False].items()}
    host = {False: torch.zeros(ncol, nz, dtype=torch.float64), True: torch.zeros(ncol, nz, dtype=torch.float32)}
    outs = {f32: {n: torch.full((ncol, nz), -7.0, dtype=torch.float32 if f32 else torch.float64, device="cuda:0") for n in ref.NAMES}
            for f32 in (False, True)}
    ALL = object()
    KEYS = ref.INPUTS + ("w",)

    def call(m, f32=False, ncol=ncol, nz=nz, out=ALL, **over):
        p = {k: v.data_ptr() for k, v in dev[f32].items()}
        p.update({k: host[f32].data_ptr() if v is HOST else v for k, v in over.items()})
        if out is ALL:
            o = _DopplerOut(**{n: outs[f32][n].data_ptr() for n in ref.NAMES})
        else:
            o = _DopplerOut(**{n: (host[f32].data_ptr() if v is HOST else outs[f32][n].data_ptr()) for n, v in (out or {}).items()})
        fn = L.kidmp32_doppler_moments_device if f32 else L.kidmp_doppler_moments_device
        return fn(m._h if m is not None else None, ncol, nz, *[p[k] for k in KEYS], C.byref(o) if out is not None else None, None)

    refused = [
        dict(t=None), dict(p=None), dict(qv=None), dict(qr=None), dict(nr=None),
        dict(nz=1), dict(nz=257), dict(nz=0), dict(ncol=-1),
        dict(out=None), dict(out={}),                                                              # nothing requested
        dict(t=HOST), dict(nr=HOST), dict(qs=HOST), dict(qg=HOST), dict(w=HOST), dict(out={"vd": HOST}), dict(out={"dbz": None, "sw": HOST}),
    ]
    for f32 in (False, True):
        for m in (gpu_mixed, gpu_warm):
            for kw in refused:
                assert call(m, f32, **kw) == EINVAL, (f32, kw)
                assert L.kidmp_last_error(m._h), kw
        assert call(None, f32) == ESTATE
        assert call(gpu_mixed, f32, ncol=0) == 0 and call(gpu_mixed, f32, ncol=0, t=None, out=None) == 0
    # the host entries refuse alike
    hst = {False: dict(st, w=w_np)}
    hst[True] = {k: v.astype(np.float32) for k, v in hst[False].items()}
    hout = {f32: {n: np.full((ncol, nz), -7.0, dtype=np.float32 if f32 else np.float64) for n in ref.NAMES} for f32 in (False, True)}

    def hcall(m, f32=False, ncol=ncol, nz=nz, out=ALL, **over):
        p = {k: v.ctypes.data for k, v in hst[f32].items()}
        p.update(over)
        o = _DopplerOut(**{n: hout[f32][n].ctypes.data for n in (ref.NAMES if out is ALL else ())})
        fn = L.kidmp32_doppler_moments_host if f32 else L.kidmp_doppler_moments_host
        return fn(m._h if m is not None else None, ncol, nz, *[p[k] for k in KEYS], C.byref(o) if out is not None else None)

    for f32 in (False, True):
        for kw in (dict(t=None), dict(p=None), dict(qv=None), dict(qr=None), dict(nr=None), dict(nz=1), dict(nz=257), dict(ncol=-1),
                   dict(out=None), dict(out={})):
            assert hcall(gpu_mixed, f32, **kw) == EINVAL, (f32, kw)
            assert L.kidmp_last_error(gpu_mixed._h), kw
        assert hcall(None, f32) == ESTATE and hcall(gpu_mixed, f32, ncol=0) == 0
    torch.cuda.synchronize()
    for f32 in (False, True):
        assert all((o.cpu().numpy() == -7.0).all() for o in outs[f32].values())                   # nothing was written
        assert all((o == -7.0).all() for o in hout[f32].values())
    # good calls afterwards still work, with any of the optional inputs left out
    for f32 in (False, True):
        dtype = np.float32 if f32 else None
        want = _doppler(gpu_mixed, st, w_np, dtype=dtype)
        assert call(gpu_mixed, f32) == 0 and hcall(gpu_mixed, f32) == 0
        torch.cuda.synchronize()
        assert all(_same(outs[f32][n].cpu().numpy(), want[n]) and _same(hout[f32][n], want[n]) for n in ref.NAMES)
        assert call(gpu_mixed, f32, qs=None, qg=None, w=None, out={"vd": None}) == 0 and hcall(gpu_warm, f32, qs=None, w=None) == 0
    torch.cuda.synchronize()
