"""The Doppler spectrum on the MI355X (include/kidmp_dspectrum.h, kidmp::k_doppler_spectrum) against
tests/doppler_spectrum_ref.py.

Bound: per velocity slot (below and above included) an absolute C * (sum of z_b of that level over the species the output
covers), C = BOUND = 1e-12, the siblings' number for this class of arithmetic: per bin one or two fastmath exponentials of
1-3.5 ulp, a position whose rounding (|p| <= 257) moves at most 257 ulp of the bin's z_b between neighbours, and a sum of
up to 768 positive terms; and the condition of exp(-lam*D) itself, whose relative error is lam*D (up to 700) times that of
the slope, which kernel and checker form by different routes (cube root against **(1/3), lamr against 1/ilamr): a few
ulp of the slope are up to 5e-13 of a bin that sits under the 700 rule.  The tests print their measured maxima in units
of that scale.  Measured on the MI355X: configs 2, 3, 5 after one step 4.4e-15, the hand-built and random sets 4.6e-14,
the set that reaches the 700 rule 3.7e-13 (rain), the shape sweep 5.0e-13 (rain on a single diameter bin).

Everything else is an equality of bits, except the cross-checks against doppler_moments, whose bounds are the CPU
convergence figures of tests/test_doppler_spectrum_abi.py (doppler_spectrum_ref.FINE_BOUND), with nothing added.  The
second moment is compared after taking off what the linear deposit adds to it: a mass split f : 1-f between two bins dv
apart has the variance f(1-f) dv**2 about its own position, and the reference sums exactly that over the bins
(doppler_spectrum_ref.deposit_broadening)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import cases
import doppler_ref as dref
import doppler_spectrum_ref as ref
import effrad_cases as ec
import fall_cases as fc

pytestmark = pytest.mark.gpu

BOUND = 1e-12
EINVAL, ESTATE = -1, -5
SPECTRA = ("total", "rain", "snow", "graupel")
COVERS = {"total": "rsg", "rain": "r", "snow": "s", "graupel": "g", "below": "rsg", "above": "rsg"}
SET_NAMES = ["config3", "config5", "config2", "hand_built", "fall_hand_built", "random65_365", "random65_366", "edge_700"]
V0, DV, NV = -3.0, 0.25, 64                                   # -3 .. 12.75 m s-1: w of +-8 fills below and above


def only(st):
    return {k: np.ascontiguousarray(st[k]) for k in ref.INPUTS}


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _dev(st, dtype=None):
    return {k: _cu(v if dtype is None else v.astype(dtype)) for k, v in st.items() if v is not None}


def _grids_dev(grids):
    return None if grids is None else {x: (_cu(g[0]), _cu(g[1])) for x, g in grids.items()}


def _spectrum(m, st, v0=V0, dv=DV, nv=NV, w=None, grids=None, want=ref.NAMES, dtype=None):
    import torch
    out = m.doppler_spectrum(_dev(st, dtype), v0, dv, nv, None if w is None else _cu(w if dtype is None else w.astype(dtype)),
                             _grids_dev(grids), want)
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


def _after_one_step(m, st):
    """The state after one step of 10 s on the device (float64), as numpy arrays with the keys of INPUTS."""
    import torch
    dev = {k: _cu(v) for k, v in st.items()}
    ppt = torch.zeros(st["t"].shape[0], 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)
    torch.cuda.synchronize()
    return {k: dev[k].cpu().numpy() for k in ref.INPUTS}


def _edge_700():
    """Rain so fine that lamr*Dr passes 700 on the scheme's own bins (lamr = 3e5 .. 2.5e7 against Dr = 50 um .. 5 mm),
    beside a level of ordinary rain and snow."""
    nz = 8
    st = {k: np.zeros((2, nz)) for k in ref.INPUTS}
    st["t"][:], st["p"][:], st["qv"][:] = 275.0, 8.0e4, 4.0e-3
    st["qr"][0] = np.geomspace(2.0e-12, 1.0e-6, nz)
    st["nr"][0] = 1.0e7
    st["qr"][1, 3], st["nr"][1, 3], st["qs"][1, 3] = 1.0e-3, 5.0e3, 4.0e-4
    return st


@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = dref.constants(o)
    o.close()
    return c


@pytest.fixture(scope="module")
def own_grids(gpu_mixed):
    """The scheme's own bins as the context holds them: species -> (D, dD)."""
    from kid_amd import default_grid
    return {x: default_grid(gpu_mixed, x) for x in ref.SPECIES}


@pytest.fixture(scope="module")
def sets(gpu_mixed, gpu_warm):
    """name -> (state, w, warm), built once and left unchanged."""
    s = {
        "config3": (_after_one_step(gpu_mixed, cases.config3(64)), False),
        "config5": (_after_one_step(gpu_mixed, cases.config5(64)), False),
        "config2": (_after_one_step(gpu_warm, cases.config2(64)), True),
        "hand_built": (only(ec.stack(ec.hand_built())), False),
        "fall_hand_built": (only(fc.scan_state(65, 12, 765)), False),
        "edge_700": (_edge_700(), False),
    }
    for seed in (365, 366):
        s["random65_%d" % seed] = (only(ec.random_state(65, 33, seed)), False)
    rng = np.random.Generator(np.random.PCG64(2026))
    return {k: (st, np.ascontiguousarray(rng.uniform(-8.0, 8.0, st["t"].shape)), warm) for k, (st, warm) in s.items()}


@pytest.fixture(scope="module")
def refs(sets, consts, own_grids):
    return {k: ref.doppler_spectrum(consts, st, V0, DV, NV, w=w, default=own_grids) for k, (st, w, _) in sets.items()}


@pytest.fixture(autouse=True)
def _leave_contexts_as_found(gpu_mixed, gpu_warm):
    yield
    for m in (gpu_mixed, gpu_warm):
        m.set_host_chunk(0)


def check_parity(got, want, names=ref.NAMES):
    """Asserts the bound of the module docstring on every slot; returns name -> the largest error in units of the scale."""
    worst = {}
    for n in names:
        scale = sum(want["sum_" + x] for x in COVERS[n])
        g, w_ = got[n], want[n]
        assert np.isfinite(g).all() and (g >= 0).all(), n
        err = np.abs(g - w_)
        if g.ndim == 3:
            scale = scale[:, None, :]
        worst[n] = float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0)))
        assert (err <= BOUND * scale).all(), (n, worst[n])
    return worst


def check_zeros(got, want):
    """An absent species and an empty level are exact +0.0 in every slot."""
    lv = want["levels"]
    for n in got:
        present = np.zeros(lv["rhof"].shape, dtype=bool)
        for x in COVERS[n]:
            present |= lv[x]["present"]
        a = got[n] if got[n].ndim == 2 else got[n].transpose(0, 2, 1)
        assert not _bits(np.ascontiguousarray(a[~present])).any(), n


# ---- 1. parity and the structure of zeros on the sets ----
@pytest.mark.parametrize("name", SET_NAMES)
def test_parity_and_bits(request, sets, refs, own_grids, name):
    st, w, warm = sets[name]
    m = request.getfixturevalue("gpu_warm" if warm else "gpu_mixed")
    got = _spectrum(m, st, w=w)
    worst = check_parity(got, refs[name])
    print("doppler spectrum %s: max error / (sum z_b) %s" % (name, {k: "%.2e" % v for k, v in worst.items()}))
    check_zeros(got, refs[name])
    assert _same_all(_spectrum(m, st), _spectrum(m, st, w=np.zeros_like(w))), "w = None is w = 0"
    assert _same_all(got, _spectrum(m, st, w=w, grids=own_grids)), "the default grid handed in by the caller"
    lv = refs[name]["levels"]
    if name not in ("hand_built", "edge_700"):
        assert all(lv[x]["present"].any() for x in ("r" if warm else "rsg")), name
        assert (got["below"] > 0).any() and (got["above"] > 0).any() and (got["total"] > 0).any(), name
    total = got["total"].sum(axis=1) + got["below"] + got["above"]
    scale = sum(refs[name]["sum_" + x] for x in "rsg")
    assert (np.abs(total - scale) <= 2 * BOUND * scale).all(), "the deposit conserves the sum"


def test_the_700_rule(gpu_mixed, sets, refs, own_grids):
    st, w, _ = sets["edge_700"]
    lamr = refs["edge_700"]["levels"]["r"]["lam"][0]
    arg = lamr[:, None] * own_grids["r"][0][None, :]
    assert arg.max() > 5e4 and (arg > 700).sum() > 300 and (arg < 700).sum() > 100
    got = _spectrum(gpu_mixed, st, w=w, want=("rain", "below", "above"))
    assert lamr[0] * own_grids["r"][0][0] > 700 * (1 + 1e-9)
    everywhere = got["rain"].sum(axis=1) + got["below"] + got["above"]
    assert not _bits(everywhere[0, 0:1]).any()                # every bin of the level lies past the threshold: exact +0.0
    assert (everywhere[0, -3:] > 0).all() and everywhere[1, 3] > 0


# ---- 2. shapes: nz x ncol, with nv and nb spread over them ----
NZ_SWEEP = (2, 63, 64, 65, 120, 129, 256)
NCOL_SWEEP = (1, 5, 33)
NV_SWEEP = (1, 2, 63, 64, 65, 128, 256)
NB_SWEEP = (1, 3, 100, 256)


def _grid_of(nb, lo, hi):
    edges = np.geomspace(lo, hi, nb + 1)
    return np.ascontiguousarray(np.sqrt(edges[:-1] * edges[1:])), np.ascontiguousarray(edges[1:] - edges[:-1])


@pytest.mark.parametrize("iz", range(len(NZ_SWEEP)))
def test_shapes(gpu_mixed, consts, own_grids, iz):
    m, nz = gpu_mixed, NZ_SWEEP[iz]
    whole_st = only(fc.scan_state(nz, 33, 1200 + nz))
    rng = np.random.Generator(np.random.PCG64(nz))
    whole_w = np.ascontiguousarray(rng.uniform(-6.0, 6.0, whole_st["t"].shape))
    for ic, ncol in enumerate(NCOL_SWEEP):
        nv = NV_SWEEP[(iz + 3 * ic) % len(NV_SWEEP)]
        nbs = [NB_SWEEP[(iz + ic + i) % len(NB_SWEEP)] for i in range(3)]
        grids = {x: _grid_of(nb, lo, hi) for x, nb, lo, hi in zip("rsg", nbs, (5e-5, 2e-4, 2.5e-4), (5e-3, 2e-2, 5e-2)) if nb != 100}
        v0, dv = -2.0, 14.0 / nv
        idx = {1: np.array([5]), 5: np.array([0, 9, 30, 31, 32]), 33: np.arange(33)}[ncol]   # 30 .. 32: the hand-built ones
        st, w = _take(whole_st, idx), np.ascontiguousarray(whole_w[idx])
        got = _spectrum(m, st, v0, dv, nv, w, grids)
        want = ref.doppler_spectrum(consts, st, v0, dv, nv, w=w, grids=grids, default=own_grids)
        worst = check_parity(got, want)
        print("doppler spectrum nz=%d ncol=%d nv=%d nb=%s: %s" % (nz, ncol, nv, nbs, {k: "%.1e" % v for k, v in worst.items()}))
        check_zeros(got, want)
        assert got["total"].shape == (ncol, nv, nz) and got["below"].shape == (ncol, nz)
        assert _same_all(got, _spectrum(m, st, v0, dv, nv, w, grids)), "a repeated call"
        if ncol == 33:                                        # sub-batches and single columns, at other positions
            for sub in ([0, 7, 8, 9, 31], [32], [30], [4]):
                part = _spectrum(m, _take(st, sub), v0, dv, nv, np.ascontiguousarray(w[sub]), grids)
                assert _same_all(part, {k: v[sub] for k, v in got.items()}), (nz, sub)


# ---- 3. every subset of want; sentinels stay in what was not requested ----
def test_every_subset_and_sentinels(gpu_mixed, sets):
    import torch
    from kid_amd.dspectrum import _DSpectrumGrids, _DSpectrumOut, library
    m = gpu_mixed
    st, w = _take(sets["random65_365"][0], slice(0, 5)), np.ascontiguousarray(sets["random65_365"][1][:5])
    ncol, nz, nv = 5, 65, 40                                  # 42 slots: two tiles, the second one short
    full = _spectrum(m, st, V0, 0.4, nv, w)
    dev, dw = _dev(st), _cu(w)
    L = library()
    for r in range(1, len(ref.NAMES) + 1):
        for asked in itertools.combinations(ref.NAMES, r):
            outs = {n: torch.full((ncol, nz) if n in ("below", "above") else (ncol, nv, nz), -7.0, dtype=torch.float64, device="cuda:0")
                    for n in ref.NAMES}
            o = _DSpectrumOut(**{n: outs[n].data_ptr() for n in asked})
            rc = L.kidmp_doppler_spectrum_device(m._h, ncol, nz, *[dev[k].data_ptr() for k in ref.INPUTS], dw.data_ptr(), V0, 0.4, nv,
                                                 C.byref(_DSpectrumGrids()), C.byref(o), None)
            torch.cuda.synchronize()
            assert rc == 0, asked
            for n in ref.NAMES:
                a = outs[n].cpu().numpy()
                assert _same(a, full[n]) if n in asked else (a == -7.0).all(), (asked, n)
    part = _spectrum(m, st, V0, 0.4, nv, w, want="snow")
    assert sorted(part) == ["snow"] and _same(part["snow"], full["snow"])
    # qs and qg left out mean zero, in a mixed-phase context too
    zero = dict(st, qs=np.zeros_like(st["qs"]), qg=np.zeros_like(st["qg"]))
    left_out = {k: v for k, v in st.items() if k not in ("qs", "qg")}
    none = _spectrum(m, left_out, w=w)
    assert _same_all(_spectrum(m, zero, w=w), none) and not none["snow"].any() and not none["graupel"].any()
    assert _same(none["rain"], none["total"]), "rain alone: total adds the same terms in the same order"


# ---- 4. binary32 entries ----
def test_binary32_entries_round_once(gpu_mixed, gpu_warm, sets):
    scans = {"scan%d" % nz: (only(fc.scan_state(nz, 5, 1200 + nz)), np.linspace(-6.0, 6.0, 5 * nz).reshape(5, nz))
             for nz in (2, 129, 256)}                                                # one, three and four level groups
    for name, m in (("config3", gpu_mixed), ("random65_366", gpu_mixed), ("config2", gpu_warm)) + tuple((n, gpu_mixed) for n in scans):
        st0, w0 = scans[name] if name in scans else sets[name][:2]
        st = {k: v[:16].astype(np.float32) for k, v in st0.items()}
        w = np.ascontiguousarray(w0[:16].astype(np.float32))
        wide = {k: v.astype(np.float64) for k, v in st.items()}
        got = _spectrum(m, st, w=w)
        ref64 = _spectrum(m, wide, w=w.astype(np.float64))
        for n in ref.NAMES:
            assert got[n].dtype == np.float32 and _same(got[n], ref64[n].astype(np.float32)), (name, n)
        assert (got["total"] > 0).any()


# ---- 5. host entries ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_entries_equal_the_device_entry(gpu_mixed, sets, dtype):
    m = gpu_mixed
    st = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in sets["random65_365"][0].items()}
    w = np.ascontiguousarray(sets["random65_365"][1].astype(dtype))
    ncol = st["t"].shape[0]
    grids = {"s": _grid_of(37, 1e-4, 3e-2)}
    want_all = _spectrum(m, st, w=w, grids=grids)
    want_two = _spectrum(m, st, want=("snow", "above"))
    for chunk in (0, 1, 7, ncol):
        m.set_host_chunk(chunk)
        assert _same_all(m.doppler_spectrum_host(st, V0, DV, NV, w, grids, ref.NAMES), want_all), chunk
        assert _same_all(m.doppler_spectrum_host(st, V0, DV, NV, want=("snow", "above")), want_two), chunk
    m.set_host_chunk(7)
    out = {"rain": np.full((ncol, NV, 65), -7.0, dtype=dtype)}
    few = m.doppler_spectrum_host({k: v for k, v in st.items() if k != "qs"}, V0, DV, NV, w, want=("rain",), out=out)
    assert few["rain"] is out["rain"] and _same(few["rain"], want_all["rain"])


def test_host_entry_where_the_staging_cap_sets_the_chunk(gpu_mixed):
    """nv = nz = 256 and all four spectra are 2.1 MiB of staging per column: the 256 MiB cap allows 126 columns, so 130 columns
    with no chunk set (one chunk by kidmp_set_host_chunk's rule) go in two, 126 and 4, and give the device entry's bits."""
    import torch
    m, ncol, nz, nv = gpu_mixed, 130, 256, 256
    per_col = (8 * nz + (4 * nv + 2) * nz) * 8
    assert (256 << 20) // per_col < ncol <= 2048
    st = only(ec.random_state(nz, ncol, 512))
    rng = np.random.Generator(np.random.PCG64(513))
    w = np.ascontiguousarray(rng.uniform(-6.0, 6.0, (ncol, nz)))
    m.set_host_chunk(0)
    got = m.doppler_spectrum_host(st, V0, 0.0625, nv, w, None, ref.NAMES)
    dev = m.doppler_spectrum(_dev(st), V0, 0.0625, nv, _cu(w), None, ref.NAMES)
    torch.cuda.synchronize()
    for n in ref.NAMES:
        assert _same(got[n], dev[n].cpu().numpy()), n
    assert (got["total"][-1] > 0).any() and (got["total"][0] > 0).any()


# ---- 6. graph capture ----
def test_hip_graph_capture_and_replay(gpu_mixed):
    """Step, then doppler_spectrum, captured once and replayed twice, gives the eager bits."""
    import torch
    m, ncol = gpu_mixed, 20
    st = cases.config3(ncol, seed=cases.SEED + 21)

    def run(dev, ppt):
        m.batch_step(dev, 10.0, ppt)
        return m.doppler_spectrum({k: dev[k] for k in ref.INPUTS}, V0, DV, NV, dev["w"], want=ref.NAMES)

    graphed = {k: _cu(v) for k, v in st.items()}
    ppt_g = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d_g = run(graphed, ppt_g)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    eager = {k: _cu(v) for k, v in st.items()}
    ppt_e = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda")
    for _ in range(2):
        d_e = run(eager, ppt_e)
    torch.cuda.synchronize()
    for n in ref.NAMES:
        assert torch.equal(d_g[n], d_e[n]), n
    assert (d_e["total"] > 0).any()


# ---- 7. cross-checks on the device: the spectrum's moments against doppler_moments ----
def test_moments_of_the_spectrum_are_the_doppler_moments(gpu_mixed, consts):
    """On the caller-supplied fine grid of the CPU convergence measurement and its hand-built levels: dBZ of the summed
    spectrum against dbz, the first moment against vd, the second, less the broadening of the deposit, against
    sw**2 + vd**2."""
    import torch
    m = gpu_mixed
    cols = [ref.hand_levels(x) for x in "rsg"]
    st = {k: np.ascontiguousarray(np.concatenate([c[k] for c in cols])) for k in ref.INPUTS}
    grids = {x: ref.fine_grid() for x in "rsg"}
    v0, dv, nv = 0.0, 0.0625, 256                             # 0 .. 15.94 m s-1
    sp = _spectrum(m, st, v0, dv, nv, grids=grids, want=("total", "below", "above"))
    mom = m.doppler_moments(_dev(st), want=("dbz", "vd", "sw"))
    torch.cuda.synchronize()
    mom = {k: v.cpu().numpy() for k, v in mom.items()}
    b0, b1, b2 = ref.FINE_BOUND
    assert not sp["below"].any()
    S = sp["total"].sum(axis=1) + sp["above"]
    # dbz holds 1.E-22 for each of the two absent species (M:5127-5136); |ln(1+e)| <= 1.01 |e| for |e| <= 2.1e-4
    ddb = np.abs(10.0 * np.log10(1e18 * (S + 2.0e-22)) - mom["dbz"])
    print("spectrum against doppler_moments: max |dBZ difference| %.3e (bound %.3e)" % (ddb.max(), 10.0 / np.log(10.0) * b0 * 1.01))
    assert (ddb <= 10.0 / np.log(10.0) * b0 * 1.01).all()
    inside = sp["above"] <= 1e-13 * S                           # the broadest graupel reaches past 16 m s-1
    print("levels whose echo lies inside the velocity grid: %d of %d" % (inside.sum(), inside.size))
    assert inside.sum() >= 16
    v = (v0 + dv * np.arange(nv))[None, :, None]
    tot = sp["total"].sum(axis=1)
    m1 = (sp["total"] * v).sum(axis=1) / tot
    m2 = (sp["total"] * v * v).sum(axis=1) / tot
    e1 = np.abs(m1 / mom["vd"] - 1.0)[inside]
    want2 = mom["sw"] ** 2 + mom["vd"] ** 2
    # the linear deposit widens every line: the reference gives the broadening of these bins at these positions exactly
    widened = dv * dv * ref.deposit_broadening(consts, st, v0, dv, nv, grids=grids)
    assert (widened >= 0).all() and (widened <= 0.25 * dv * dv).all()
    e2 = np.abs((m2 - widened) / want2 - 1.0)[inside]
    print("first moment: max relative %.3e (bound %.3e); second, less the deposit's broadening (at most %.3e of it): %.3e (bound %.3e)"
          % (e1.max(), b1, (widened / want2)[inside].max(), e2.max(), b2))
    assert (e1 <= b1).all()
    assert (e2 <= b2).all()


# ---- 8. refusals ----
HOST = "a pageable host array"


def test_refusals_write_nothing(gpu_mixed, gpu_warm, sets):
    import torch
    from kid_amd.dspectrum import _DSpectrumGrids, _DSpectrumOut, library
    L = library()
    st = _take(sets["config3"][0], slice(0, 6))
    w_np = np.ascontiguousarray(sets["config3"][1][:6])
    ncol, nz, nv = 6, 120, 16
    dev = {False: dict(_dev(st), w=_cu(w_np))}
    dev[True] = {k: v.float() for k, v in dev[False].items()}
    host = {False: torch.zeros(ncol * nv, nz, dtype=torch.float64), True: torch.zeros(ncol * nv, nz, dtype=torch.float32)}
    shape = lambda n: (ncol, nz) if n in ("below", "above") else (ncol, nv, nz)   # noqa: E731
    outs = {f32: {n: torch.full(shape(n), -7.0, dtype=torch.float32 if f32 else torch.float64, device="cuda:0") for n in ref.NAMES}
            for f32 in (False, True)}
    dD = _cu(np.full(10, 1e-4))
    ALL = object()
    KEYS = ref.INPUTS + ("w",)

    def grids_of(g):
        s = _DSpectrumGrids()
        for i, (D_, dD_, nb) in (g or {}).items():
            s.D[i] = host[False].data_ptr() if D_ is HOST else (D_.data_ptr() if D_ is not None else None)
            s.dD[i] = dD_.data_ptr() if dD_ is not None else None
            s.nb[i] = nb
        return s

    def call(m, f32=False, ncol=ncol, nz=nz, out=ALL, v0=V0, dv=DV, nv=nv, grids=None, **over):
        p = {k: v.data_ptr() for k, v in dev[f32].items()}
        p.update({k: host[f32].data_ptr() if v is HOST else v for k, v in over.items()})
        if out is ALL:
            o = _DSpectrumOut(**{n: outs[f32][n].data_ptr() for n in ref.NAMES})
        else:
            o = _DSpectrumOut(**{n: (host[f32].data_ptr() if v is HOST else outs[f32][n].data_ptr()) for n, v in (out or {}).items()})
        fn = L.kidmp32_doppler_spectrum_device if f32 else L.kidmp_doppler_spectrum_device
        return fn(m._h if m is not None else None, ncol, nz, *[p[k] for k in KEYS], v0, dv, nv, C.byref(grids_of(grids)) if grids != "null" else None,
                  C.byref(o) if out is not None else None, None)

    refused = [
        dict(t=None), dict(p=None), dict(qv=None), dict(qr=None), dict(nr=None),
        dict(nz=1), dict(nz=257), dict(nz=0), dict(ncol=-1),
        dict(nv=0), dict(nv=257), dict(nv=-3), dict(dv=0.0), dict(dv=-1.0), dict(dv=float("nan")), dict(dv=float("inf")), dict(dv=1e-320),
        dict(v0=float("nan")), dict(v0=float("inf")),
        dict(out=None), dict(out={}),                                                              # nothing requested
        dict(grids={0: (dD, None, 10)}), dict(grids={2: (None, dD, 10)}), dict(grids={1: (dD, dD, 0)}), dict(grids={1: (dD, dD, 257)}),
        dict(grids={0: (HOST, dD, 10)}),
        dict(t=HOST), dict(nr=HOST), dict(qs=HOST), dict(qg=HOST), dict(w=HOST), dict(out={"total": HOST}), dict(out={"rain": None, "above": HOST}),
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
    hout = {f32: {n: np.full(shape(n), -7.0, dtype=np.float32 if f32 else np.float64) for n in ref.NAMES} for f32 in (False, True)}

    def hcall(m, f32=False, ncol=ncol, nz=nz, out=ALL, v0=V0, dv=DV, nv=nv, **over):
        p = {k: v.ctypes.data for k, v in hst[f32].items()}
        p.update(over)
        o = _DSpectrumOut(**{n: hout[f32][n].ctypes.data for n in (ref.NAMES if out is ALL else ())})
        fn = L.kidmp32_doppler_spectrum_host if f32 else L.kidmp_doppler_spectrum_host
        return fn(m._h if m is not None else None, ncol, nz, *[p[k] for k in KEYS], v0, dv, nv, None, C.byref(o) if out is not None else None)

    for f32 in (False, True):
        for kw in (dict(t=None), dict(p=None), dict(qv=None), dict(qr=None), dict(nr=None), dict(nz=1), dict(nz=257), dict(ncol=-1),
                   dict(nv=0), dict(nv=257), dict(dv=0.0), dict(dv=float("nan")), dict(v0=float("inf")), dict(out=None), dict(out={})):
            assert hcall(gpu_mixed, f32, **kw) == EINVAL, (f32, kw)
            assert L.kidmp_last_error(gpu_mixed._h), kw
        assert hcall(None, f32) == ESTATE and hcall(gpu_mixed, f32, ncol=0) == 0
    torch.cuda.synchronize()
    for f32 in (False, True):
        assert all((o.cpu().numpy() == -7.0).all() for o in outs[f32].values())                   # nothing was written
        assert all((o == -7.0).all() for o in hout[f32].values())
    # good calls afterwards still work, with any of the optional inputs left out and grids NULL
    for f32 in (False, True):
        dtype = np.float32 if f32 else None
        want = _spectrum(gpu_mixed, st, V0, DV, nv, w_np, dtype=dtype)
        assert call(gpu_mixed, f32) == 0 and hcall(gpu_mixed, f32) == 0
        torch.cuda.synchronize()
        assert all(_same(outs[f32][n].cpu().numpy(), want[n]) and _same(hout[f32][n], want[n]) for n in ref.NAMES)
        assert call(gpu_mixed, f32, qs=None, qg=None, w=None, grids="null", out={"below": None}) == 0 and hcall(gpu_warm, f32, qs=None, w=None) == 0
    torch.cuda.synchronize()
