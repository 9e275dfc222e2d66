"""The lidar operator on the MI355X (include/kidmp_lidar.h, kidmp::k_lidar_profiles) against tests/lidar_ref.py.

Bounds (none is a measured number).  BOUND = 1e-12 is the parameters' bound of tests/test_gpu_size_spectra.py, taken over,
u = 2**-53 and eps = 4 BOUND:
  ext_x, ext, bsc   eps relative: a slope enters cubed
  bsc_mol           8 u relative
  tau_*             eps tau_ref(k) + nz u tau_column absolute: the second term covers a tree order against a serial order
                    over positive terms
  att_*             ref (eps (1 + 2 tau_incl(k)) + 2 nz u tau_column + 16 u) + 1e-250: the floor covers a term on the 700
                    threshold, as in the size spectra
  sr_*              the sum of its operands' relative bounds; the molecular profile's own is 8 u + 2 nz u taum_column + 16 u
  TAU_PART, TAU_MOL (eps + nz u) and (10 u + nz u) relative: the terms' bounds and the order of the sum
  heights           the reference's level, and its face within nz u of the column's depth; counts are equal
The thresholds of the summary are taken from the reference itself, the geometric mean of two adjacent distinct sorted
values whose ratio exceeds 1 + 1e-6, so that no level lies within a bound of a threshold and no column is left out.
Absent species, sub-batches, subsets, the binary32 entries, the host entries and graph replay are equalities of bits.
The cross-check against size_spectra's bins is held to twice the difference the two numpy references show on the same
grid.  The tests print their measured maxima."""
import ctypes as C
import math

import numpy as np
import pytest

import cases
import effrad_cases as ec
import fall_cases as fc
import lidar_cases as lc
import lidar_ref as ref
import size_spectra_ref as ssr

pytestmark = pytest.mark.gpu

BOUND = 1e-12                                         # tests/test_gpu_size_spectra.py
U, EPS, FLOOR = 2.0 ** -53, 4 * BOUND, 1e-250
NZ_SWEEP = (2, 63, 64, 65, 120, 129, 256)
NCOL_SWEEP = (1, 5, 33)
EINVAL, ESTATE = -1, -5
CFG = ref.cfg(s_ratio=(17.0, 29.0, 21.0, 33.0, 27.0), eta=0.6, c_mol=5.0e-32, beta_detect=1.0e-6, trans_lost=1.0e-2)
X_OF = dict(ext_c="c", ext_i="i", ext_r="r", ext_s="s", ext_g="g")


@pytest.fixture(scope="module")
def consts():
    return ssr.constants()


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _dev(st, dtype=None):
    return {k: _cu(v if dtype is None else v.astype(dtype)) for k, v in st.items() if v is not None}


def _only(st):
    return {k: np.ascontiguousarray(st[k]) for k in ref.INPUTS}


def _after_one_step(m, st):
    import torch
    dev = {k: _cu(v) for k, v in st.items()}
    ppt = torch.zeros(st["t"].shape[0], 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)
    torch.cuda.synchronize()
    return {k: dev[k].cpu().numpy() for k in ref.INPUTS}


def _with_cloud(st, seed):
    """fall_cases.scan_state has no cloud water: add some, as tests/test_gpu_size_spectra.py adds it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    shape = st["t"].shape
    qc = np.where(rng.uniform(size=shape) < 0.5, np.exp(rng.uniform(np.log(1e-9), np.log(3e-3), shape)), 0.0)
    qc[-3:] = 0.0
    qc[-3, -1] = 5.0e-4
    return _only(dict(st, qc=qc, nc=np.exp(rng.uniform(np.log(1e1), np.log(1e11), shape))))


def _per_column_dz(ncol, nz, seed):
    return np.ascontiguousarray(np.stack([lc.uneven_dz(nz, seed + c, 10.0, 150.0) for c in range(ncol)]))


@pytest.fixture(scope="module")
def sets(gpu_mixed, gpu_warm):
    """name -> (state, warm, dz), built once and left unchanged."""
    return {
        "config3": (_after_one_step(gpu_mixed, cases.config3(64)), False, lc.uneven_dz(120, 3, 20.0, 200.0)),
        "config5": (_after_one_step(gpu_mixed, cases.config5(64)), False, _per_column_dz(64, 120, 40)),
        "config2": (_after_one_step(gpu_warm, cases.config2(64)), True, np.full(120, 25.0)),
        "hand_built": (_only(ec.stack(ec.hand_built())), False, lc.uneven_dz(120, 4, 1.0, 60.0)),
        "fall_hand_built": (_with_cloud(fc.scan_state(65, 12, 765), 31), False, lc.uneven_dz(65, 6, 5.0, 100.0)),
    }


@pytest.fixture(autouse=True)
def _leave_contexts_as_found(gpu_mixed, gpu_warm):
    yield
    for m in (gpu_mixed, gpu_warm):
        m.set_host_chunk(0)
        m.set_column_nc(None)


def _lidar(m, st, dz, cf=CFG, want=ref.NAMES, summary=True, dtype=None):
    import torch
    d = None if dz is None else _cu(dz if dtype is None else dz.astype(dtype))
    out = m.lidar_profiles(_dev(st, dtype), d, cf, want, summary)
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


def _reference(consts, st, dz, cf=CFG, **kw):
    """The reference's profiles, the configuration with thresholds chosen from them, and its summary."""
    o = ref.profiles(consts, st, dz, cf, **kw)
    cf2, clear = ref.with_thresholds(o, cf)
    assert clear, "no column may be left out: a threshold must be found"
    s, k = ref.summary(o, cf2)
    return o, cf2, s, k


def check_profiles(got, o, names=ref.NAMES):
    """Asserts the bounds of the module docstring and the exact zeros; returns the measured maxima relative to each bound."""
    nz = o["ext"].shape[-1]
    worst = {}
    any_x = np.zeros(o["ext"].shape, dtype=bool)
    for x in ref.SPECIES:
        any_x |= o["has_" + x]
    for n in names:
        g, w = got[n], o[n]
        if n in ("ext_c", "ext_i", "ext_r", "ext_s", "ext_g", "ext", "bsc"):
            has = o["has_" + X_OF[n]] if n in X_OF else any_x
            assert np.isfinite(g).all() and not _bits(g)[~has].any(), n            # +0.0 where absent
            assert (g[has] > 0).all(), n
            tol = EPS * np.abs(w)
        elif n == "bsc_mol":
            tol = 8 * U * w
        elif n.startswith("tau"):
            assert np.isfinite(g).all() and (g >= 0).all(), n
            tol = EPS * w + nz * U * o["tau_column"]
        elif n.startswith("att"):
            assert np.isfinite(g).all() and (g >= 0).all(), n
            tol = w * _att_rel(o, n[-2:], nz) + FLOOR
        else:
            d = n[-2:]
            a, m = o["att_" + d], o["attm_" + d]
            ok = (m > 1e-200) & (a > 1e-200)
            assert ok.any(), n
            rel = _att_rel(o, d, nz) + FLOOR / np.where(ok, a, 1.0) + (8 * U + 2 * nz * U * o["taum_column"] + 16 * U) \
                + FLOOR / np.where(ok, m, 1.0)
            g, w, tol = g[ok], w[ok], (w * rel)[ok]
        err = np.abs(g - w)
        assert (err <= tol).all(), (n, float((err / np.where(tol > 0, tol, 1.0)).max()))
        worst[n] = float((err / np.where(tol > 0, tol, 1.0)).max()) if err.size else 0.0
    return worst


def _att_rel(o, d, nz):
    return EPS * (1.0 + 2.0 * o["tau_incl_" + d]) + 2 * nz * U * o["tau_column"] + 16 * U


def check_summary(got, o, s, k):
    nz = o["ext"].shape[-1]
    depth = np.sum(o["dz"], axis=-1)
    assert (np.abs(got[:, ref.TAU_PART] - s[:, ref.TAU_PART]) <= (EPS + nz * U) * s[:, ref.TAU_PART]).all()
    assert (np.abs(got[:, ref.TAU_MOL] - s[:, ref.TAU_MOL]) <= (10 + nz) * U * s[:, ref.TAU_MOL]).all()
    for slot in (ref.Z_BASE_UP, ref.Z_LOST_UP, ref.Z_TOP_DN, ref.Z_LOST_DN):
        none = np.isnan(s[:, slot])
        assert np.array_equal(np.isnan(got[:, slot]), none), slot
        assert (np.abs(got[:, slot] - s[:, slot])[~none] <= (nz * U * depth)[~none]).all(), slot
    assert np.array_equal(got[:, ref.N_UP], s[:, ref.N_UP]) and np.array_equal(got[:, ref.N_DN], s[:, ref.N_DN])


# ---- 1. parity on the sets ----
@pytest.mark.parametrize("name", ["config3", "config5", "config2", "hand_built", "fall_hand_built"])
def test_parity(request, sets, consts, name):
    st, warm, dz = sets[name]
    m = request.getfixturevalue("gpu_warm" if warm else "gpu_mixed")
    o, cf, s, k = _reference(consts, st, dz, warm=warm)
    got = _lidar(m, st, dz, cf)
    worst = check_profiles(got, o)
    check_summary(got["summary"], o, s, k)
    print("lidar %s: max error / bound %s; levels found %d of %d" % (name, {n: "%.3f" % v for n, v in worst.items()}, (k >= 0).sum(), k.size))
    assert (k >= 0).any()
    if warm:
        assert not any(_bits(got[n]).any() for n in ("ext_i", "ext_s", "ext_g"))
        liquid = {n: v for n, v in st.items() if n not in ("qi", "ni", "qs", "qg", "nc")}
        assert _same_all(got, _lidar(m, liquid, dz, cf))                         # the frozen inputs may be left out
    if name == "config3":
        assert all((got["ext_" + x] > 0).any() for x in ref.SPECIES)


def test_g_over_three_hundred_decades(gpu_warm, consts):
    """Clear air with ext_mol = 1 m-1 and 2 dtau from 1e-300 to 1e3: the attenuated profile is g, and sr is 1 exactly."""
    st, dz, c_mol = lc.g_column()
    cf = ref.cfg(eta=1.0, c_mol=c_mol)
    o = ref.profiles(consts, st, dz, cf, warm=True)
    got = _lidar(gpu_warm, st, dz, cf, summary=False)
    x = 2.0 * o["dtau"][0]
    assert x.min() < 1.1e-300 and x.max() > 999.0 and (o["att_up"][0] > 0).all()
    worst = check_profiles(got, o, ("bsc_mol", "tau_up", "tau_dn", "att_up", "att_dn"))
    # the layer mean itself: att_up / (bsc_mol E(2 tau_up)) against expm1, E's error (2 u + that of its argument) taken out
    with np.errstate(under="ignore"):
        gl = got["att_up"][0] / (got["bsc_mol"][0] * np.exp(-2.0 * got["tau_up"][0]))
    want = np.where(x > 0, -np.expm1(-x) / x, 1.0)
    err = np.abs(gl / want - 1.0) / U
    print("g on the device: max %.1f u over 2 dtau in [%.0e, %.0e]; error / bound %s" % (err.max(), x.min(), x.max(), worst))
    assert (err <= 16).all()              # 16 u: g 3 ulp, E 1 ulp and two products on the device; exp, expm1 and four operations here
    assert (got["sr_up"][0] == 1.0).all() and (got["sr_dn"][0][o["attm_dn"][0] > 0] == 1.0).all()


def test_the_700_rule_on_an_opaque_column(gpu_warm, consts):
    st, dz = lc.opaque_column()
    o, cf, s, k = _reference(consts, st, dz, warm=True)
    got = _lidar(gpu_warm, st, dz, cf)
    check_profiles(got, o)
    check_summary(got["summary"], o, s, k)
    for d in ("up", "dn"):
        two_tau = 2.0 * o["tau_" + d][0]
        assert (two_tau > 700).sum() > 20 and (two_tau < 700).sum() > 20
        assert not _bits(got["att_" + d][0])[two_tau > 700 * (1 + 1e-9)].any()     # exact +0.0 past the threshold
        assert (got["att_" + d][0][two_tau < 700 * (1 - 1e-9)] > 0).all()
    assert got["summary"][0, ref.TAU_PART] > 700 and not np.isnan(got["summary"][0]).any()


# ---- 2. shapes ----
@pytest.mark.parametrize("nz", NZ_SWEEP)
def test_level_and_column_shapes(gpu_mixed, consts, nz):
    m = gpu_mixed
    st = _only(ec.random_state(nz, max(NCOL_SWEEP), 700 + nz))
    dz = _per_column_dz(33, nz, nz) if nz % 2 else lc.uneven_dz(nz, nz, 5.0, 80.0)
    o, cf, s, k = _reference(consts, st, dz)
    whole = _lidar(m, st, dz, cf)
    assert whole["att_up"].shape == (33, nz) and whole["summary"].shape == (33, 8)
    worst = check_profiles(whole, o)
    check_summary(whole["summary"], o, s, k)
    print("nz = %d: max error / bound %.3f" % (nz, max(worst.values())))
    assert _same_all(whole, _lidar(m, st, dz, cf)), "a repeated call"
    for ncol in NCOL_SWEEP[:-1]:
        idx = (np.arange(ncol) * 7 + nz) % 33                                    # other positions in another batch
        part = _lidar(m, _take(st, idx), dz[idx] if dz.ndim == 2 else dz, cf)
        assert _same_all(part, {n: v[idx] for n, v in whole.items()}), (nz, ncol)


# ---- 3. options ----
def test_each_output_alone_subsets_and_sentinels(gpu_mixed, sets):
    import torch
    from kid_amd.lidar import _LidarCfg, _LidarOut, library
    m, L = gpu_mixed, library()
    st, _, dz = sets["fall_hand_built"]
    ncol, nz = st["t"].shape
    full = _lidar(m, st, dz)
    dev, ddz = _dev(st), _cu(dz)
    outs = {n: torch.empty((ncol, nz), dtype=torch.float64, device="cuda:0") for n in ref.NAMES}
    summ = torch.empty((ncol, 8), dtype=torch.float64, device="cuda:0")
    c = _LidarCfg((C.c_double * 5)(*CFG["s_ratio"]), CFG["eta"], CFG["c_mol"], CFG["beta_detect"], CFG["trans_lost"])
    rng = np.random.Generator(np.random.PCG64(77))
    subsets = [((n,), False) for n in ref.NAMES] + [((), True)]
    subsets += [(tuple(n for n in ref.NAMES if rng.uniform() < 0.4), bool(rng.uniform() < 0.5)) for _ in range(20)]
    for asked, with_summary in subsets:
        if not asked and not with_summary:
            asked = ("ext",)
        for t in list(outs.values()) + [summ]:
            t.fill_(-7.0)
        o = _LidarOut(**{n: outs[n].data_ptr() for n in asked})
        rc = L.kidmp_lidar_profiles_device(m._h, ncol, nz, *[dev[k].data_ptr() for k in ref.INPUTS], ddz.data_ptr(), 0, C.byref(c), C.byref(o),
                                           summ.data_ptr() if with_summary else None, None)
        torch.cuda.synchronize()
        assert rc == 0, asked
        for n in ref.NAMES:
            a = outs[n].cpu().numpy()
            assert _same(a, full[n]) if n in asked else (a == -7.0).all(), (asked, n)
        a = summ.cpu().numpy()
        assert (_bits(a) == _bits(full["summary"])).all() if with_summary else (a == -7.0).all(), asked
    # the profiles that need no neighbour, without dz: the bits of the full request
    local = _lidar(m, st, None, want=ref.LOCAL, summary=False)
    assert sorted(local) == sorted(ref.LOCAL) and all(_same(local[n], full[n]) for n in ref.LOCAL)
    # a NULL cfg is the library's conventions
    assert _same_all(_lidar(m, st, dz, None), _lidar(m, st, dz, ref.cfg()))


def test_binary32_entries_round_once(gpu_mixed, gpu_warm, sets):
    randoms = {"random%d" % nz: (_only(ec.random_state(nz, 5, 700 + nz)), None, lc.uneven_dz(nz, nz, 5.0, 80.0))
               for nz in (2, 129, 256)}                                              # one, three and four level groups
    for name, m in (("config3", gpu_mixed), ("fall_hand_built", gpu_mixed), ("config2", gpu_warm)) + tuple((n, gpu_mixed) for n in randoms):
        st0, _, dz0 = randoms[name] if name in randoms else sets[name]
        st = {k: v.astype(np.float32) for k, v in st0.items()}
        dz = dz0.astype(np.float32)
        got = _lidar(m, st, dz)
        ref64 = _lidar(m, {k: v.astype(np.float64) for k, v in st.items()}, dz.astype(np.float64))
        for n in ref.NAMES:
            with np.errstate(over="ignore", under="ignore"):
                rounded = ref64[n].astype(np.float32)
            same = _bits(got[n]) == _bits(rounded)
            assert got[n].dtype == np.float32 and (same | (np.isnan(got[n]) & np.isnan(rounded))).all(), (name, n)
        assert got["summary"].dtype == np.float64 and (_bits(got["summary"]) == _bits(ref64["summary"])).all(), name


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_entries_equal_the_device_entry(gpu_mixed, sets, dtype, monkeypatch):
    from padded_rows import with_padded
    from kid_amd.lidar import library
    m = gpu_mixed
    st0, _, dz0 = sets["config5"]                                                # dz per column
    st = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in st0.items()}
    dz = np.ascontiguousarray(dz0.astype(dtype))
    ncol = st["t"].shape[0]
    want = _lidar(m, st, dz)
    shared = _lidar(m, st, dz[0])
    some = ("ext_s", "att_dn", "tau_up")
    for chunk in (0, 1, 7, ncol):
        m.set_host_chunk(chunk)
        got = m.lidar_profiles_host(st, dz, CFG, ref.NAMES, True)
        assert sorted(got) == sorted(want) and all((_bits(got[n]) == _bits(want[n])).all() for n in want), chunk
        part = m.lidar_profiles_host(st, dz, CFG, some)
        assert sorted(part) == sorted(some) and all(_same(part[n], want[n]) for n in some), chunk
        got = m.lidar_profiles_host(st, np.ascontiguousarray(dz[0]), CFG, ("att_up",), True)
        assert _same(got["att_up"], shared["att_up"]) and (_bits(got["summary"]) == _bits(shared["summary"])).all(), chunk
        only = m.lidar_profiles_host(st, None, CFG, ("ext", "bsc_mol"))
        assert _same(only["ext"], want["ext"]) and _same(only["bsc_mol"], want["bsc_mol"]), chunk
    # seven columns in chunks of 3, 3 and 1, the rows of dz nz + 5 apart (dz_col_stride)
    st7, dz7 = _take(st, np.arange(7)), np.ascontiguousarray(dz[:7])
    want7 = _lidar(m, st7, dz7)
    m.set_host_chunk(3)
    seen = with_padded(monkeypatch, library(), "kidmp_lidar_profiles_host" if dtype == np.float64 else "kidmp32_lidar_profiles_host", {14: dz7})
    got = m.lidar_profiles_host(st7, dz7, CFG, ref.NAMES, True)
    assert sorted(got) == sorted(want7) and all((_bits(got[n]) == _bits(want7[n])).all() for n in want7) and seen == [(14, 125)]


def test_hip_graph_replay_of_one_captured_launch(gpu_mixed, sets):
    import torch
    from kid_amd.lidar import _LidarCfg, _LidarOut, library
    m, L = gpu_mixed, library()
    st, _, dz = sets["config3"]
    ncol, nz = st["t"].shape
    dev, ddz = _dev(st), _cu(dz)
    names = ("ext", "att_up", "sr_dn", "tau_dn")
    out = {n: torch.full((ncol, nz), -7.0, dtype=torch.float64, device="cuda:0") for n in names}
    summ = torch.full((ncol, 8), -7.0, dtype=torch.float64, device="cuda:0")
    c = _LidarCfg((C.c_double * 5)(*CFG["s_ratio"]), CFG["eta"], CFG["c_mol"], CFG["beta_detect"], CFG["trans_lost"])
    o = _LidarOut(**{n: out[n].data_ptr() for n in names})
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = L.kidmp_lidar_profiles_device(m._h, ncol, nz, *[dev[k].data_ptr() for k in ref.INPUTS], ddz.data_ptr(), 0, C.byref(c), C.byref(o),
                                           summ.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    eager = _lidar(m, st, dz, want=names)
    for _ in range(2):
        for t in list(out.values()) + [summ]:
            t.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert all(_same(out[n].cpu().numpy(), eager[n]) for n in names)
        assert (_bits(summ.cpu().numpy()) == _bits(eager["summary"])).all()


def test_a_bound_droplet_number_changes_cloud_water_alone(gpu_mixed, sets, consts):
    st, _, dz = sets["fall_hand_built"]
    ncol = st["t"].shape[0]
    plain = _lidar(gpu_mixed, st, dz)
    nd = np.exp(np.linspace(np.log(5.0), np.log(3000.0), ncol))                  # cm-3
    gpu_mixed.set_column_nc(nd)
    o, cf, s, k = _reference(consts, st, dz, Nt_c=(nd * 1.e6)[:, None])
    bound = _lidar(gpu_mixed, st, dz, cf)
    gpu_mixed.set_column_nc(None)
    worst = check_profiles(bound, o)
    check_summary(bound["summary"], o, s, k)
    print("per-column droplet number: max error / bound %.3f" % max(worst.values()))
    for n in ("ext_i", "ext_r", "ext_s", "ext_g", "bsc_mol"):
        assert _same(bound[n], plain[n]), n
    assert not _same(bound["ext_c"], plain["ext_c"]) and not _same(bound["att_up"], plain["att_up"])
    assert _same_all(_lidar(gpu_mixed, st, dz), plain), "unbound again"


def test_aerosol_aware_context_takes_the_callers_droplet_number(gpu_mixed_aero, consts):
    st = _only(ec.stack([ec.hand_built(64)[k] for k in ("nc_sweep", "qc_sweep")]))
    dz = lc.uneven_dz(64, 9, 1.0, 30.0)
    o, cf, s, k = _reference(consts, st, dz, aero=True)
    got = _lidar(gpu_mixed_aero, st, dz, cf)
    worst = check_profiles(got, o)
    check_summary(got["summary"], o, s, k)
    print("aerosol-aware: max error / bound %.3f" % max(worst.values()))
    assert (got["ext_c"] > 0).sum() > 60


# ---- 4. cross-checks on the device ----
@pytest.mark.parametrize("x", ref.SPECIES)
def test_telescoping_identity_on_the_device(gpu_mixed, x):
    """sum_k att(k) dz_k = (1 - E(2 tau_total))/(2 eta S), as tests/test_lidar_abi.py holds the reference to it."""
    st = lc.one_species(x)
    nz = st["t"].shape[1]
    dz = lc.uneven_dz(nz)
    S = 31.0 + ref.SPECIES.index(x)
    cf = ref.cfg(s_ratio=[S] * 5, eta=0.45, c_mol=0.0)
    got = _lidar(gpu_mixed, st, dz, cf, want=("att_up", "att_dn", "tau_up", "tau_dn"), summary=True)
    tau = 0.45 * got["summary"][0, ref.TAU_PART]
    assert got["summary"][0, ref.TAU_MOL] == 0.0 and 0.05 < tau < 30.0
    rhs = (1.0 - math.exp(-2.0 * tau)) / (2.0 * 0.45 * S)
    for d in ("up", "dn"):
        lhs = math.fsum(got["att_" + d][0] * dz)
        print("identity %s %s: %.2f ulp" % (x, d, abs(lhs - rhs) / np.spacing(rhs)))
        assert abs(lhs - rhs) <= 16 * nz * np.spacing(rhs), (x, d)
    assert got["tau_up"][0, 0] == 0.0 and got["tau_dn"][0, -1] == 0.0 and not np.signbit(got["tau_dn"][0, -1])


def test_tau_part_of_liquid_columns_is_the_summarys_tau_c(gpu_warm, oracle_warm):
    """On the columns tests/test_lidar_abi.py selects (re_qc unclamped, qv >= 1e-10) the two entries state one number: within
    lc.PI_GAP (the scheme's ten-digit PI in am_r) plus the two sums' own bounds, 2 (BOUND + nz u)."""
    import torch
    st, dz, cols, _ = lc.select_liquid(oracle_warm)
    nz = dz.size
    mine = _lidar(gpu_warm, st, dz, want=("ext_c",))["summary"][:, ref.TAU_PART]
    dev = _dev({k: st[k] for k in ("t", "p", "qv", "qc", "nc", "qi", "qr", "nr", "qs", "qg")})
    tau_c = gpu_warm.column_summary(dev, _cu(dz))
    torch.cuda.synchronize()
    tau_c = tau_c.cpu().numpy()[:, 6]
    rel = np.abs(mine / tau_c - 1.0)
    print("TAU_PART against TAU_C: %s" % rel)
    assert len(cols) == 5 and (rel[cols] <= lc.PI_GAP + 2 * (BOUND + nz * U)).all()
    assert (np.delete(rel, cols) > 1e-6).all()


def test_extinction_is_the_second_moment_of_the_size_spectra(gpu_mixed, consts):
    """ext_x against (pi/2) sum_b D_b**2 N_b of kidmp_size_spectra_device on a log-spaced 256-bin grid: within twice the
    difference the two numpy references show for the same grid (a midpoint rule of 256 bins: DESIGN.md 4.5k)."""
    import torch
    edges = np.exp(np.linspace(np.log(2e-7), np.log(0.2), 257))
    D, dD = np.ascontiguousarray(np.sqrt(edges[:-1] * edges[1:])), np.ascontiguousarray(np.diff(edges))
    st = {k: np.ascontiguousarray(np.concatenate([lc.one_species(x)[k] for x in ref.SPECIES])) for k in ref.INPUTS}
    grids = {x: (D, dD) for x in ref.SPECIES}
    want = ssr.size_spectra(consts, st, grids=grids)
    o = ref.extinctions(consts, st)
    got = _lidar(gpu_mixed, st, None, want=ref.LOCAL[:5], summary=False)
    bins = gpu_mixed.size_spectra(_dev(st), ref.SPECIES, {x: (_cu(D), _cu(dD)) for x in ref.SPECIES})
    torch.cuda.synchronize()
    for i, x in enumerate(ref.SPECIES):
        has = o["has_" + x][i]
        mom = lambda N: (0.5 * np.pi) * np.sum(D[:, None] ** 2 * N, axis=0)     # noqa: E731
        cpu = np.abs(mom(want[x][i]) / np.where(has, o["ext_" + x][i], 1.0) - 1.0)[has].max()
        gpu = np.abs(mom(bins[x].cpu().numpy()[i]) / np.where(has, got["ext_" + x][i], 1.0) - 1.0)[has].max()
        print("ext_%s against 256 bins: references %.3e, device %.3e" % (x, cpu, gpu))
        assert has.sum() > 20 and gpu <= 2 * cpu and cpu < 0.05, x


# ---- 5. refusals ----
def test_refusals_write_nothing(gpu_mixed, gpu_warm, gpu_mixed_aero, sets):
    import torch
    from kid_amd.lidar import _LidarCfg, _LidarOut, library
    L = library()
    st = _take(sets["config3"][0], slice(0, 6))
    ncol, nz = 6, 120
    dz_np = sets["config3"][2]
    dev = {False: dict(_dev(st), dz=_cu(dz_np))}
    dev[True] = {k: v.float() for k, v in dev[False].items()}
    host = {False: torch.zeros(ncol * nz, dtype=torch.float64), True: torch.zeros(ncol * nz, dtype=torch.float32)}
    outs = {f32: {n: torch.full((ncol, nz), -7.0, dtype=torch.float32 if f32 else torch.float64, device="cuda:0") for n in ref.NAMES}
            for f32 in (False, True)}
    summ = torch.full((ncol, 8), -7.0, dtype=torch.float64, device="cuda:0")
    HOST = "a pageable host array"

    def cfg_of(**kw):
        d = dict(CFG, **kw)
        return _LidarCfg((C.c_double * 5)(*d["s_ratio"]), d["eta"], d["c_mol"], d["beta_detect"], d["trans_lost"])

    def call(m, f32=False, ncol=ncol, nz=nz, names=ref.NAMES, stride=0, cfg=None, summary=True, no_struct=False, **over):
        p = {k: v.data_ptr() for k, v in dev[f32].items()}
        p.update({k: host[f32].data_ptr() if v is HOST else v for k, v in over.items() if k in ref.INPUTS + ("dz",)})
        o = _LidarOut(**{n: (host[f32].data_ptr() if over.get("out_" + n) is HOST else outs[f32][n].data_ptr()) for n in names})
        c = cfg_of(**(cfg or {}))
        fn = L.kidmp32_lidar_profiles_device if f32 else L.kidmp_lidar_profiles_device
        s = host[False].data_ptr() if over.get("out_summary") is HOST else summ.data_ptr() if summary else None
        return fn(m._h if m is not None else None, ncol, nz, *[p[k] for k in ref.INPUTS], p["dz"], stride, C.byref(c),
                  None if no_struct else C.byref(o), s, None)

    nan, inf = float("nan"), float("inf")
    refused = [
        dict(t=None), dict(p=None), dict(qv=None), dict(qc=None), dict(qr=None), dict(nr=None), dict(dz=None),
        dict(qi=None), dict(ni=None), dict(qs=None), dict(qg=None),               # a mixed-phase context
        dict(nz=1), dict(nz=257), dict(ncol=-1), dict(stride=1), dict(stride=nz - 1), dict(stride=-nz),
        dict(names=(), summary=False), dict(no_struct=True, summary=False),      # nothing requested at all
        dict(cfg=dict(s_ratio=(17.0, 0.0, 21.0, 33.0, 27.0))), dict(cfg=dict(s_ratio=(17.0, 29.0, 21.0, 33.0, -27.0))),
        dict(cfg=dict(s_ratio=(nan, 29.0, 21.0, 33.0, 27.0))), dict(cfg=dict(eta=0.0)), dict(cfg=dict(eta=1.5)), dict(cfg=dict(eta=nan)),
        dict(cfg=dict(c_mol=-1e-40)), dict(cfg=dict(c_mol=inf)), dict(cfg=dict(c_mol=0.0)), dict(cfg=dict(beta_detect=nan)),
        dict(cfg=dict(trans_lost=inf)),
        dict(t=HOST), dict(qg=HOST), dict(dz=HOST), dict(out_ext=HOST), dict(out_sr_dn=HOST), dict(out_summary=HOST),
    ]
    for f32 in (False, True):
        for kw in refused:
            assert call(gpu_mixed, f32, **kw) == EINVAL, (f32, kw)
            assert L.kidmp_last_error(gpu_mixed._h), kw
        assert call(gpu_warm, f32, qr=None) == EINVAL and call(gpu_mixed_aero, f32, nc=None) == EINVAL
        assert call(None, f32) == ESTATE
    assert call(gpu_mixed, ncol=0) == 0 and call(gpu_mixed, ncol=0, t=None, names=(), summary=False) == 0
    gpu_mixed.set_column_nc(np.full(ncol + 1, 80.0))
    assert call(gpu_mixed) == EINVAL
    gpu_mixed.set_column_nc(None)
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == -7.0).all() for f32 in (False, True) for o in outs[f32].values()) and (summ.cpu().numpy() == -7.0).all()
    # the host entries refuse alike
    hout = {n: np.full((ncol, nz), -7.0) for n in ref.NAMES}
    hsum = np.full((ncol, 8), -7.0)

    def hcall(m, ncol=ncol, nz=nz, names=ref.NAMES, stride=0, cfg=None, **over):
        p = dict({k: st[k].ctypes.data for k in ref.INPUTS}, dz=dz_np.ctypes.data)
        p.update(over)
        o = _LidarOut(**{n: hout[n].ctypes.data for n in names})
        c = cfg_of(**(cfg or {}))
        return L.kidmp_lidar_profiles_host(m._h if m is not None else None, ncol, nz, *[p[k] for k in ref.INPUTS], p["dz"], stride, C.byref(c),
                                           C.byref(o), hsum.ctypes.data)

    for kw in (dict(t=None), dict(qc=None), dict(qi=None), dict(dz=None), dict(nz=1), dict(nz=257), dict(ncol=-1), dict(stride=7),
               dict(cfg=dict(eta=2.0)), dict(cfg=dict(c_mol=0.0))):
        assert hcall(gpu_mixed, **kw) == EINVAL, kw
    assert hcall(None) == ESTATE and hcall(gpu_mixed, ncol=0) == 0
    assert all((o == -7.0).all() for o in hout.values()) and (hsum == -7.0).all()
    # good calls afterwards still work; c_mol = 0 is refused for the ratios alone
    want = _lidar(gpu_mixed, st, dz_np)
    assert call(gpu_mixed) == 0 and hcall(gpu_mixed) == 0
    torch.cuda.synchronize()
    assert all(_same(outs[False][n].cpu().numpy(), want[n]) and _same(hout[n], want[n]) for n in ref.NAMES)
    assert (_bits(hsum) == _bits(want["summary"])).all()
    assert call(gpu_mixed, names=ref.NAMES[:12], cfg=dict(c_mol=0.0)) == 0
    assert call(gpu_warm, qi=None, ni=None, qs=None, qg=None, nc=None) == 0
    assert call(gpu_mixed, names=ref.LOCAL, summary=False, dz=None) == 0
    torch.cuda.synchronize()
