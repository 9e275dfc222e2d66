"""calc_refl10cm (M:4946-5244) on the MI355X: the reflectivity kernel (kid_amd/csrc/thompson_reflectivity.hip) against the
numpy restatement of tests/refl_oracle.py, and its C ABI / Python entries (include/kidmp.h)."""
import ctypes as C

import numpy as np
import pytest

import cases
import refl_oracle as ro

pytestmark = pytest.mark.gpu

# |dBZ(kernel) - dBZ(restatement)| at every level: about 10x the measured maximum, 2.8e-14 dB
BOUND_DB = 3e-13
NZ_SWEEP = (2, 63, 64, 65, 120, 128, 129, 256)
KEYS = ("t", "p", "qv", "qr", "nr", "qs", "qg")


@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = ro.constants(o)
    o.close()
    return c


def _dev(st, dtype=None):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(st[k] if dtype is None else st[k].astype(dtype))).to("cuda:0")
            for k in KEYS if st.get(k) is not None}


def _gpu_dbz(m, st, dtype=None):
    import torch
    out = m.reflectivity(_dev(st, dtype))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _random_state(nz, ncol, seed):
    """Columns with rain, snow and graupel switched on and off at random, supercooled rain, levels without graupel
    between graupel levels (they enter the running minimum of the intercept)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    z = np.linspace(0.0, 14000.0, nz)[None, :]
    t = 302.0 - 6.5e-3 * z + rng.uniform(-3, 3, (ncol, 1))
    p = 1.0e5 * np.exp(-z / 8000.0) * np.ones((ncol, 1))
    qv = 0.016 * np.exp(-z / 2500.0) * rng.uniform(0.5, 1.2, (ncol, nz))
    def species(lo, hi, frac):
        q = np.exp(rng.uniform(np.log(lo), np.log(hi), (ncol, nz)))
        return np.where(rng.uniform(size=(ncol, nz)) < frac, q, 0.0)
    qr = species(1e-9, 8e-3, 0.6)
    nr = np.exp(rng.uniform(np.log(1.0), np.log(1e6), (ncol, nz)))
    qs = species(1e-7, 4e-3, 0.5)
    qg = species(1e-7, 1.2e-2, 0.5)
    return {k: np.ascontiguousarray(v) for k, v in dict(t=t, p=p, qv=qv, qr=qr, nr=nr, qs=qs, qg=qg).items()}


def _hand_built(nz=120):
    """The parity hazards of the issue, one column each (a base sounding with everything else switched off)."""
    base = _random_state(nz, 1, 7)
    for k in ("qr", "nr", "qs", "qg"):
        base[k][:] = 0.0
    cols = []
    def col(**kw):
        c = {k: v.copy() for k, v in base.items()}
        for k, v in kw.items():
            c[k][0, :] = v
        cols.append(c)
    r1, r2 = 1e-12, 1e-6
    col(qr=np.resize([np.nextafter(r1, 0), r1, np.nextafter(r1, 1)], nz), nr=1e3)          # qr at R1 -1 / 0 / +1 ulp
    col(qs=np.resize([np.nextafter(r2, 0), r2, np.nextafter(r2, 1)], nz))                   # qs at R2
    col(qg=np.resize([np.nextafter(r2, 0), r2, np.nextafter(r2, 1)], nz))                   # qg at R2
    t = np.resize([270.64, 270.65, 270.66], nz)                                              # T at 270.65 -/0/+ 0.01
    col(t=t, qr=2e-3, nr=50.0, qg=3e-3)                                                      # (mvd_r > 100 um there)
    # mvd_r swept through 100 um: mvd_r = 3.672/lamr, lamr**3 = am_r*6*nr/rr; supercooled, with graupel
    rho = 0.622 * base["p"][0] / (ro.R * 260.0 * (base["qv"][0] + 0.622))
    mvd = np.linspace(85e-6, 115e-6, nz)
    rr = 1e-3 * rho
    nr = rr * (3.672 / mvd) ** 3 / (ro.am_r * 6.0) / rho
    col(t=260.0, qr=1e-3, nr=nr, qg=2e-3)
    # N0_exp at gonv_min: heavy supercooled rain of large drops and heavy graupel (zans1 < 4).  (gonv_max cannot be reached:
    # zans1 <= 3.1 + 100/30.09 = 6.42 < log10(3e6), so the top of the column only meets the initial N0_min = gonv_max.)
    col(t=255.0, qr=5e-3, nr=5.0, qg=1.5e-2)
    # a running minimum set by a level without graupel: light graupel everywhere (rg < 5e-5: ygra1 as at a graupel-free
    # level) but at one level, which holds supercooled rain instead (xslw1 > 0.01 lowers its intercept) -- near the top
    # and in the middle of the column
    for ke in (nz - 3, nz // 2):
        qg = np.full(nz, 1e-5)
        qg[ke] = 0.0
        qr = np.zeros(nz)
        qr[ke] = 6e-3
        col(qg=qg, qr=qr, nr=2.0, t=262.0)
    # rain just above R1 with a huge number: the cube root's argument (unclamped, as in the reference) passes 1e37
    col(qr=2e-12, nr=1e30)
    return {k: np.ascontiguousarray(np.concatenate([c[k] for c in cols])) for k in KEYS}


def _max_err(m, c, st):
    want = ro.of_state(c, st)
    got = _gpu_dbz(m, st)
    assert np.all(np.isfinite(got))
    return float(np.max(np.abs(got - want)))


def test_parity_configs_and_edge_cases(gpu_mixed, consts):
    worst = 0.0
    for st in (cases.config3(48), cases.config5(48), cases.edge_cases(), _hand_built()):
        worst = max(worst, _max_err(gpu_mixed, consts, st))
    print("reflectivity parity (configs, edge cases, hand-built): max |ddBZ| = %.3e dB" % worst)
    assert worst <= BOUND_DB


@pytest.mark.parametrize("nz", NZ_SWEEP)
def test_parity_nz_sweep(gpu_mixed, consts, nz):
    worst = max(_max_err(gpu_mixed, consts, _random_state(nz, 96, 100 + nz)), _max_err(gpu_mixed, consts, _hand_built(nz)))
    print("reflectivity parity nz=%d: max |ddBZ| = %.3e dB" % (nz, worst))
    assert worst <= BOUND_DB


def test_hand_built_columns_exercise_the_branches(consts):
    """The hazards are reached: clamps, thresholds and the running minimum take effect in the restatement."""
    st = _hand_built()
    v = ro.load(consts, st["qv"], st["qr"], st["nr"], st["qs"], st["qg"], st["t"], st["p"])
    assert v["L_qr"][0].sum() == 40 and v["L_qs"][1].sum() == 40 and v["L_qg"][2].sum() == 40
    assert (v["mvd_r"][4] > 100e-6).any() and (v["mvd_r"][4] < 100e-6).any()
    _, N0_g = ro.graupel(consts, v["temp"], v["L_qr"], v["mvd_r"], v["rg"])
    assert np.isclose(N0_g[5].min(), ro.gonv_min, rtol=1e-12, atol=0)
    # T = 270.64 / 270.65 / 270.66 with supercooled-size rain everywhere: only T < 270.65 switches xslw1 (M:5089)
    assert v["L_qr"][3].all() and (v["mvd_r"][3] > 100e-6).all()
    slw = (v["temp"][3] < 270.65) & v["L_qr"][3] & (v["mvd_r"][3] > 100e-6)
    assert np.array_equal(slw, np.resize([True, False, False], 120))
    # the graupel-free level with supercooled rain sets the running minimum for every graupel level below it
    for c, ke in ((6, 117), (7, 60)):
        assert not v["L_qg"][c][ke] and v["L_qg"][c][:ke].all() and v["L_qg"][c][ke + 1:].all()
        below, above = N0_g[c][:ke], N0_g[c][ke + 1:]
        # (N0_g = N0_exp / lam_exp * lamg: the same intercept to rounding)
        assert np.allclose(below, below[0], rtol=1e-14, atol=0) and below.max() < 0.9 * above.min()
    # the cube root's argument of the rain slope passes the 1e37 the fp32-seeded root covers
    rr, nr = v["rr"][8], v["nr"][8]
    assert (ro.am_r * consts["crg"][2] * consts["org2"] * nr / rr > 1e37).all()


def test_repeatable_and_batch_independent(gpu_mixed):
    st = _random_state(120, 64, 5)
    a, b = _gpu_dbz(gpu_mixed, st), _gpu_dbz(gpu_mixed, st)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    for i in (0, 17, 63):
        one = _gpu_dbz(gpu_mixed, {k: v[i:i + 1] for k, v in st.items()})
        assert np.array_equal(one[0].view(np.uint64), a[i].view(np.uint64))


def test_float32_entry_is_fp64_kernel_on_widened_inputs(gpu_mixed):
    st32 = {k: v.astype(np.float32) for k, v in _random_state(129, 40, 9).items()}
    got = _gpu_dbz(gpu_mixed, st32)
    assert got.dtype == np.float32
    wide = _gpu_dbz(gpu_mixed, {k: v.astype(np.float64) for k, v in st32.items()})
    assert np.array_equal(got.view(np.uint32), wide.astype(np.float32).view(np.uint32))


def test_host_entry_equals_device_entry(gpu_mixed):
    try:
        for chunk, ncol in ((16, 50), (1, 7)):   # several chunks through the staging memory: 16 + 16 + 16 + 2 columns; seven of one
            gpu_mixed.set_host_chunk(chunk)
            for dtype, view in ((np.float64, np.uint64), (np.float32, np.uint32)):
                st = {k: np.ascontiguousarray(v[:ncol].astype(dtype)) for k, v in _random_state(65, 50, 11).items()}
                h = gpu_mixed.reflectivity_host(st)
                d = _gpu_dbz(gpu_mixed, st)
                assert h.dtype == dtype and h.shape == (ncol, 65) and np.array_equal(h.view(view), d.view(view))
    finally:
        gpu_mixed.set_host_chunk(0)


def _step_inputs(ncol):
    st = cases.config3(ncol)
    return {k: np.ascontiguousarray(v) for k, v in st.items()}


def _diag_step(m, st, dt):
    from kid_amd import STATE_NAMES, FORCING_NAMES, load_library
    L = load_library()
    ncol, nz = st["qv"].shape
    ppt = np.zeros((ncol, 4))
    rates = np.zeros((ncol, 36, nz))
    nstep = np.zeros((ncol, 4), dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    rc = L.kidmp_batch_step_host_diag(m._h, ncol, nz, dt, *[dp(st[k]) for k in STATE_NAMES + FORCING_NAMES], dp(ppt),
                                      dp(rates), nstep.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0
    return ppt, rates, nstep


def _refl_step(m, st, dt):
    from kid_amd import STATE_NAMES, FORCING_NAMES, load_library
    L = load_library()
    ncol, nz = st["qv"].shape
    ppt = np.zeros((ncol, 4))
    rates = np.zeros((ncol, 36, nz))
    nstep = np.zeros((ncol, 4), dtype=np.int32)
    dbz = np.full((ncol, nz), np.nan)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    rc = L.kidmp_batch_step_host_refl(m._h, ncol, nz, dt, *[dp(st[k]) for k in STATE_NAMES + FORCING_NAMES], dp(ppt),
                                      dp(rates), nstep.ctypes.data_as(C.POINTER(C.c_int32)), dp(dbz))
    assert rc == 0
    return ppt, rates, nstep, dbz


@pytest.mark.parametrize("chunk", [0, 1000])
def test_refl_host_step_matches_diag_and_reflectivity(gpu_mixed, chunk):
    from kid_amd import STATE_NAMES
    ncol = 2500
    gpu_mixed.set_host_chunk(chunk)              # 1000: three chunks through the three-stage pipeline
    try:
        a = _step_inputs(ncol)
        b = {k: v.copy() for k, v in a.items()}
        pa, ra, na = _diag_step(gpu_mixed, a, 10.0)
        pb, rb, nb, dbz = _refl_step(gpu_mixed, b, 10.0)
    finally:
        gpu_mixed.set_host_chunk(0)
    for k in STATE_NAMES:
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    assert np.array_equal(pa.view(np.uint64), pb.view(np.uint64))
    assert np.array_equal(ra.view(np.uint64), rb.view(np.uint64))
    assert np.array_equal(na, nb)
    want = _gpu_dbz(gpu_mixed, b)                # reflectivity() of the post-step state
    assert np.array_equal(dbz.view(np.uint64), want.view(np.uint64))


def test_refl_host_step_python_and_binary32(gpu_mixed):
    from kid_amd import STATE_NAMES
    st = _step_inputs(300)
    a = {k: v.copy() for k, v in st.items()}
    ppt, rates, dbz = gpu_mixed.batch_step_host(a, 10.0, want_rates=True, want_dbz=True)
    assert np.array_equal(dbz.view(np.uint64), _gpu_dbz(gpu_mixed, a).view(np.uint64))
    s32 = {k: v.astype(np.float32) for k, v in st.items()}
    x = {k: v.copy() for k, v in s32.items()}
    y = {k: v.copy() for k, v in s32.items()}
    px, rx, nx = gpu_mixed.batch_step32_host(x, 10.0, want_rates=True, want_nstep=True)
    py, ry, ny, dbz32 = gpu_mixed.batch_step32_host(y, 10.0, want_rates=True, want_nstep=True, want_dbz=True)
    for k in STATE_NAMES:
        assert np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)), k
    assert np.array_equal(px.view(np.uint32), py.view(np.uint32)) and np.array_equal(nx, ny)
    assert np.array_equal(rx.view(np.uint64), ry.view(np.uint64))
    assert dbz32.dtype == np.float32
    assert np.array_equal(dbz32.view(np.uint32), _gpu_dbz(gpu_mixed, y).view(np.uint32))


def test_bad_arguments_are_refused(gpu_mixed):
    import torch
    from kid_amd import load_library
    L = load_library()
    st = _dev(_random_state(64, 4, 3))
    out = torch.empty_like(st["t"])
    args = [st[k].data_ptr() for k in KEYS]
    s = torch.cuda.current_stream().cuda_stream
    assert L.kidmp_reflectivity_device(gpu_mixed._h, 4, 64, *args, out.data_ptr(), s) == 0
    for i in range(5):                           # t, p, qv, qr, nr
        bad = list(args)
        bad[i] = None
        assert L.kidmp_reflectivity_device(gpu_mixed._h, 4, 64, *bad, out.data_ptr(), s) == -1
    assert L.kidmp_reflectivity_device(gpu_mixed._h, 4, 64, *args, None, s) == -1
    assert L.kidmp_reflectivity_device(gpu_mixed._h, 4, 64, *args[:5], None, None, out.data_ptr(), s) == -1   # mixed
    assert L.kidmp_reflectivity_device(gpu_mixed._h, 4, 64, *args[:5], args[5], None, out.data_ptr(), s) == -1
    for nz in (1, 257):
        assert L.kidmp_reflectivity_device(gpu_mixed._h, 1, nz, *args, out.data_ptr(), s) == -1
    host = np.zeros(4 * 64)                      # a host array on a device entry
    assert L.kidmp_reflectivity_device(gpu_mixed._h, 4, 64, host.ctypes.data, *args[1:], out.data_ptr(), s) == -1
    assert L.kidmp_reflectivity_device(gpu_mixed._h, 4, 64, *args, host.ctypes.data, s) == -1
    torch.cuda.synchronize()


def test_warm_context_without_frozen_species(gpu_warm, consts):
    st = _random_state(120, 32, 21)
    st["qs"][:] = 0.0
    st["qg"][:] = 0.0
    want = ro.of_state(consts, st)
    got = _gpu_dbz(gpu_warm, {k: v for k, v in st.items() if k not in ("qs", "qg")})
    assert np.max(np.abs(got - want)) <= BOUND_DB
    h = gpu_warm.reflectivity_host({k: v for k, v in st.items() if k not in ("qs", "qg")})
    assert np.array_equal(h.view(np.uint64), got.view(np.uint64))
