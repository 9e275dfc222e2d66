"""The bright band on the MI355X (include/kidmp_brightband.h, kidmp::k_bright_band) against tests/bright_band_ref.py, on the
hand-built columns of tests/bright_band_cases.py.

Exact: k0; enh_* = 1.0, fmelt_* = +0.0 and the bits of kidmp_reflectivity_device's dbz at every level at or above k0 and
in every column without a melting level; every equality between two device results (subsets, positions, repeats, the host
entries, binary32 after one rounding, graph replay).  fmelt_* within 2 ulp of the reference (one IEEE division and one
subtraction on values the two sides form by different routes).

Against the numpy reference, at every element: enh_s, enh_g relative; dbz, dbz_s, dbz_g as the relative difference of the
reflectivity they stand for, |d dBZ| * ln(10)/10.  The bounds are four times the largest difference measured on the
MI355X over all shapes of this file (MEASURED below):
    enh_s  8.9e-16 (4 ulp)    enh_g  6.7e-16 (3 ulp)    dbz, dbz_s, dbz_g  6.6e-15 (1.4e-14 dB at 50 dBZ: two ulp of the dBZ)
far under the 1e-11 at which an explanation would be owed.  Kernel and reference form the slopes by different routes
(fastmath pow against numpy's **, lamg against 1/ilamg), and an ulp of a slope is up to lam*D ulp of exp(-lam*D) in a
bin; the ratio cancels most of it, since the same density weighs numerator and denominator.

The vacuum limit, cfg.eps_w = 1: E_x = (1 - fm_x)**2.  Bound max(4 x measured, 64 ulp), the measurement being what the
numpy reference gives for |E/(1 - fm)**2 - 1| on the same columns; the test forms it from the reference when it runs.  On
these columns it is 3.1e-15 (snow) and 8.4e-15 (graupel) with water as the matrix (cancellation in eps_p - 1, see
tests/test_bright_band_abi.py), the device giving the same figures, and 4.1e-2 and 0.19 with the ice-air core as the
matrix, where the limit is no identity (Maxwell-Garnett is not symmetric in matrix and inclusion; the table of
tests/test_bright_band_abi.py has the figures).  With the core as the matrix the limit therefore
pins little, and the comparison with the reference at the bounds above is made for both topologies.
"""
import ctypes as C

import numpy as np
import pytest

import bright_band_cases as bc
import bright_band_ref as ref
import doppler_ref as dref

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
ULP = 2.220446049250313e-16
# the largest differences from the reference measured on the MI355X over every shape and configuration of this file
MEASURED = {"enh_s": 8.9e-16, "enh_g": 6.7e-16, "dbz": 6.6e-15}
NZS = (2, 33, 64, 65, 120, 129, 200, 256)
SHAPES = [(nz, ncol) for nz in NZS for ncol in (1, 5)] + [(120, 257), (200, 18)]
NUMBERS = ref.PROFILES


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _dev(st, dtype=None):
    return {k: _cu(v if dtype is None else v.astype(dtype)) for k, v in st.items() if v is not None}


def _cfg(cfg):
    from kid_amd import BrightBandCfg
    return None if cfg is None else BrightBandCfg(**cfg)


def _bb(m, st, cfg=None, grids=None, want=ref.NAMES, dtype=None):
    import torch
    g = None if grids is None else {x: (_cu(a), _cu(b)) for x, (a, b) in grids.items()}
    out = m.bright_band(_dev(st, dtype), _cfg(cfg), g, want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _refl(m, st):
    import torch
    out = m.reflectivity(_dev(st))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_all(a, b):
    return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)


def _take(st, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}


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
def main_set(consts, own_grids):
    """The state most tests share, its built-in melting levels and its reference: 120 levels, two columns of every kind."""
    st, k0 = bc.batch(120, 2 * bc.KINDS, 2026)
    return st, k0, ref.bright_band(consts, st, default=own_grids)


@pytest.fixture(autouse=True)
def _leave_contexts_as_found(gpu_mixed, gpu_warm):
    yield
    for m in (gpu_mixed, gpu_warm):
        m.set_host_chunk(0)


def check_exact_parts(got, want, dry_dbz):
    """k0, the dry levels and fmelt."""
    assert got["k0"].dtype == np.int32 and np.array_equal(got["k0"], want["k0"])
    nz = got["dbz"].shape[1]
    dry = (want["k0"][:, None] < 0) | (np.arange(nz)[None, :] >= want["k0"][:, None])
    assert np.array_equal(_bits(got["dbz"])[dry], _bits(dry_dbz)[dry])
    for x in ref.SPECIES:
        e, f = got["enh_" + x], got["fmelt_" + x]
        assert (e[dry] == 1.0).all() and (_bits(f)[dry] == 0).all(), x
        assert np.array_equal(f > 0, want["fmelt_" + x] > 0) and (f >= 0).all() and (f <= 0.99).all()
        assert (np.abs(f - want["fmelt_" + x]) <= 2 * ULP * want["fmelt_" + x]).all(), x
        assert (e[f == 0] == 1.0).all() and np.isfinite(e).all() and (e > 0).all(), x


def check_parity(got, want):
    """Every number against the reference at the module's bounds; returns the measured maxima."""
    worst = {}
    for x in ref.SPECIES:
        n = "enh_" + x
        worst[n] = float(np.max(np.abs(got[n] / want[n] - 1.0)))
    d = max(float(np.max(np.abs(got[n] - want[n]))) for n in ("dbz", "dbz_s", "dbz_g"))
    worst["dbz"] = d * np.log(10.0) / 10.0
    print("measured", {k: "%.2e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 4 * MEASURED[k], (k, v)
    return worst


# ---- 1. shapes and cases ----
@pytest.mark.parametrize("nz, ncol", SHAPES, ids=lambda v: str(v))
def test_shapes_against_the_reference(gpu_mixed, consts, own_grids, nz, ncol):
    st, built = bc.batch(nz, ncol, 100 * nz + ncol, kinds=(0,) if (nz, ncol) == (2, 1) else None)
    want = ref.bright_band(consts, st, default=own_grids)
    assert np.array_equal(want["k0"], built)
    got = _bb(gpu_mixed, st)
    check_exact_parts(got, want, _refl(gpu_mixed, st))
    check_parity(got, want)
    if nz == 2:
        assert (got["k0"][built >= 0] == 1).all() and (got["fmelt_s"][built >= 0, 0] > 0).any()
    if nz == 200 and ncol >= 7:
        pairs = (got["fmelt_s"] > 0).sum(axis=1) + (got["fmelt_g"] > 0).sum(axis=1)
        assert pairs[6] == 2 * (nz - 1) > 64                                      # kind 6: every level below k0 melts
        assert got["k0"][8] == 130 and (got["fmelt_s"][8, 64:] == 0).all() and (got["fmelt_s"][8, 3:41] > 0).all()   # kind 8


def test_the_cases_of_the_main_set(gpu_mixed, main_set):
    st, built, want = main_set
    got = _bb(gpu_mixed, st)
    check_exact_parts(got, want, _refl(gpu_mixed, st))
    check_parity(got, want)
    k0 = got["k0"]
    assert k0[1] == 1 and k0[2] == 119 and k0[5] == -1 and k0[7] == -1
    c = 3                                                                          # only snow at k0: graupel below stays dry
    assert st["qg"][c, k0[c]] == 0 and (st["qg"][c, :k0[c]] > 1e-6).any()
    assert (got["enh_g"][c] == 1.0).all() and (got["fmelt_g"][c] == 0).all() and (got["fmelt_s"][c, :k0[c]] > 0).any()
    c = 4                                                                          # rs[k] > rs[k0]: the floor
    assert (got["fmelt_s"][c, k0[c] - 6:k0[c]] == 0.05).all()
    # the band is a band: snow's reflectivity is enhanced where it melts
    assert (got["enh_s"][got["fmelt_s"] > 0] > 1.0).all() and (got["enh_g"][got["fmelt_g"] > 0] > 1.0).all()


@pytest.mark.parametrize("topology", [ref.WATER_MATRIX, ref.ICE_MATRIX])
def test_both_topologies_and_callers_grids_against_the_reference(gpu_mixed, consts, own_grids, main_set, topology):
    st = main_set[0]
    edges = np.geomspace(1.0e-5, 0.08, 257)
    fine = (np.sqrt(edges[:-1] * edges[1:]), edges[1:] - edges[:-1])
    for grids in (None, {"s": fine}, {"g": (fine[0][:65], fine[1][:65]), "s": (own_grids["s"][0][40:41], own_grids["s"][1][40:41])},
                  {"s": (fine[0][::4], fine[1][::4] * 4.0), "g": fine}):
        cfg = ref.default_cfg(topology=topology)
        want = ref.bright_band(consts, st, cfg, grids, own_grids)
        got = _bb(gpu_mixed, st, cfg, grids)
        check_exact_parts(got, want, _refl(gpu_mixed, st))
        check_parity(got, want)
    other = ref.default_cfg(topology=topology, eps_w=complex(60.0, 30.0), eps_i=3.0, rho_w=990.0, rho_i=917.0)
    check_parity(_bb(gpu_mixed, st, other), ref.bright_band(consts, st, other, None, own_grids))
    # NULL is the defaults; kw2 is the carrier's normalisation and cancels in the ratio
    if topology == ref.WATER_MATRIX:
        assert _same_all(_bb(gpu_mixed, st, None), _bb(gpu_mixed, st, ref.default_cfg()))
        assert _same_all(_bb(gpu_mixed, st, None), _bb(gpu_mixed, st, ref.default_cfg(kw2=0.5)))


@pytest.mark.parametrize("topology", [ref.WATER_MATRIX, ref.ICE_MATRIX])
def test_the_vacuum_limit(gpu_mixed, consts, own_grids, main_set, topology):
    st = main_set[0]
    cfg = ref.default_cfg(eps_w=complex(1.0, 0.0), topology=topology)
    want = ref.bright_band(consts, st, cfg, None, own_grids)
    got = _bb(gpu_mixed, st, cfg)
    for x in ref.SPECIES:
        act = want["fmelt_" + x] > 0
        assert act.sum() > 30
        limit = (1.0 - want["fmelt_" + x][act]) ** 2
        measured = float(np.max(np.abs(want["enh_" + x][act] / limit - 1.0)))
        mine = float(np.max(np.abs(got["enh_" + x][act] / (1.0 - got["fmelt_" + x][act]) ** 2 - 1.0)))
        print("vacuum limit, topology %d, %s: the reference %.2e, the device %.2e" % (topology, x, measured, mine))
        assert mine <= max(4 * measured, 64 * ULP), (x, mine, measured)


def test_an_iiwarm_context_has_no_melting_level(gpu_warm, main_set):
    st = main_set[0]
    got = _bb(gpu_warm, st)
    assert (got["k0"] == -1).all() and _same(got["dbz"], _refl(gpu_warm, st))
    for x in ref.SPECIES:
        assert (got["enh_" + x] == 1.0).all() and (_bits(got["fmelt_" + x]) == 0).all()
    warm = {k: (None if k in ("qs", "qg") else v) for k, v in st.items()}
    assert _same(_bb(gpu_warm, warm, want=("dbz",))["dbz"], _refl(gpu_warm, warm))


# ---- 2. equalities of bits ----
def test_each_output_alone_subsets_and_sentinels(gpu_mixed, main_set):
    import torch
    from kid_amd.brightband import _BrightBandGrids, _BrightBandOut, library
    m, L = gpu_mixed, library()
    st = main_set[0]
    ncol, nz = st["t"].shape
    full = _bb(m, st)
    dev = _dev(st)
    outs = {n: torch.empty((ncol, nz), dtype=torch.float64, device="cuda:0") for n in NUMBERS}
    outs["k0"] = torch.empty(ncol, dtype=torch.int32, device="cuda:0")
    rng = np.random.Generator(np.random.PCG64(78))
    subsets = [(n,) for n in ref.NAMES] + [tuple(n for n in ref.NAMES if rng.uniform() < 0.4) or ("enh_g",) for _ in range(16)]
    g = _BrightBandGrids()
    for asked in subsets:
        for t in outs.values():
            t.fill_(-7)
        o = _BrightBandOut(**{n: outs[n].data_ptr() for n in asked})
        rc = L.kidmp_bright_band_device(m._h, ncol, nz, *[dev[k].data_ptr() for k in ref.INPUTS], None, C.byref(g), C.byref(o), None)
        torch.cuda.synchronize()
        assert rc == 0, asked
        for n in ref.NAMES:
            a = outs[n].cpu().numpy()
            assert _same(a, full[n]) if n in asked else (a == -7).all(), (asked, n)


def test_a_column_alone_at_any_position_and_again(gpu_mixed, main_set):
    st = main_set[0]
    ncol = st["t"].shape[0]
    whole = _bb(gpu_mixed, st)
    assert _same_all(_bb(gpu_mixed, st), whole)                                    # a second call
    for c in (0, 6, 8, ncol - 1):
        assert _same_all(_bb(gpu_mixed, _take(st, slice(c, c + 1))), {n: v[c:c + 1] for n, v in whole.items()}), c
    idx = (np.arange(ncol) * 7 + 3) % ncol                                         # other positions in another batch
    assert _same_all(_bb(gpu_mixed, _take(st, idx)), {n: v[idx] for n, v in whole.items()})
    rep = np.repeat(np.arange(ncol), 15)                                           # 270 columns: several workgroups
    assert _same_all(_bb(gpu_mixed, _take(st, rep)), {n: v[rep] for n, v in whole.items()})


def test_binary32_entries_round_once(gpu_mixed, main_set):
    for st0 in [main_set[0]] + [bc.batch(nz, 5, 100 * nz + 5)[0] for nz in (33, 129, 256)]:   # two, then one, three and four level groups
        st = {k: v.astype(np.float32) for k, v in st0.items()}
        got = _bb(gpu_mixed, st)
        ref64 = _bb(gpu_mixed, {k: v.astype(np.float64) for k, v in st.items()})
        for n in NUMBERS:
            assert got[n].dtype == np.float32 and _same(got[n], ref64[n].astype(np.float32)), (st["t"].shape[1], n)
        assert got["k0"].dtype == np.int32 and np.array_equal(got["k0"], ref64["k0"]) and (got["k0"] >= 0).any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_entries_equal_the_device_entry(gpu_mixed, own_grids, main_set, dtype):
    m = gpu_mixed
    st = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in main_set[0].items()}
    grids = {"g": (np.ascontiguousarray(own_grids["g"][0][::2]), np.ascontiguousarray(own_grids["g"][1][::2] * 2.0))}
    cfg = ref.default_cfg(topology=ref.ICE_MATRIX)
    want, want_g = _bb(m, st), _bb(m, st, cfg, grids)
    some = ("enh_s", "k0", "dbz_g")
    for chunk in (5, 7):
        m.set_host_chunk(chunk)
        assert _same_all(m.bright_band_host(st, want=ref.NAMES), want), chunk
        part = m.bright_band_host(st, want=some)
        assert sorted(part) == sorted(some) and all(_same(part[n], want[n]) for n in some), chunk
        assert _same_all(m.bright_band_host(st, _cfg(cfg), grids, ref.NAMES), want_g), chunk
    m.set_host_chunk(1)                                       # seven columns, one per chunk
    st7 = _take(st, np.arange(7))
    assert _same_all(m.bright_band_host(st7, _cfg(cfg), grids, ref.NAMES), _bb(m, st7, cfg, grids))


def test_hip_graph_replay_of_one_captured_launch(gpu_mixed, main_set):
    import torch
    from kid_amd.brightband import _BrightBandGrids, _BrightBandOut, library
    m, L = gpu_mixed, library()
    st = main_set[0]
    ncol, nz = st["t"].shape
    dev = _dev(st)
    names = ("dbz", "enh_s", "fmelt_g", "k0")
    out = {n: torch.full((ncol, nz), -7.0, dtype=torch.float64, device="cuda:0") for n in names[:3]}
    out["k0"] = torch.full((ncol,), -7, dtype=torch.int32, device="cuda:0")
    o, gr = _BrightBandOut(**{n: out[n].data_ptr() for n in names}), _BrightBandGrids()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = L.kidmp_bright_band_device(m._h, ncol, nz, *[dev[k].data_ptr() for k in ref.INPUTS], None, C.byref(gr), C.byref(o),
                                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    eager = _bb(m, st, want=names)
    for _ in range(2):
        for t in out.values():
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert all(_same(out[n].cpu().numpy(), eager[n]) for n in names)


# ---- 3. refusals ----
def test_refusals_write_nothing(gpu_mixed, main_set):
    import torch
    from kid_amd.brightband import _BrightBandCfg, _BrightBandGrids, _BrightBandOut, library
    L = library()
    st = _take(main_set[0], slice(0, 6))
    ncol, nz = 6, 120
    dev = {False: _dev(st)}
    dev[True] = {k: v.float() for k, v in dev[False].items()}
    host = {False: torch.zeros(ncol * nz, dtype=torch.float64), True: torch.zeros(ncol * nz, dtype=torch.float32)}
    outs = {f32: dict({n: torch.full((ncol, nz), -7.0, dtype=torch.float32 if f32 else torch.float64, device="cuda:0") for n in NUMBERS},
                      k0=torch.full((ncol,), -7, dtype=torch.int32, device="cuda:0")) for f32 in (False, True)}
    grid_dev = torch.ones(10, dtype=torch.float64, device="cuda:0")
    HOST = "a pageable host array"

    def cfg_of(**kw):
        d = ref.default_cfg(**kw)
        return _BrightBandCfg(d["eps_w"].real, d["eps_w"].imag, d["eps_i"], d["rho_w"], d["rho_i"], d["kw2"], d["topology"])

    def grids_of(spec):
        g = _BrightBandGrids()
        for i, (D, dD, nb) in (spec or {}).items():
            g.D[i] = host[False].data_ptr() if D is HOST else grid_dev.data_ptr() if D else None
            g.dD[i] = grid_dev.data_ptr() if dD else None
            g.nb[i] = nb
        return g

    def call(m, f32=False, ncol=ncol, nz=nz, names=ref.NAMES, cfg=None, grids=None, no_struct=False, **over):
        p = {k: v.data_ptr() for k, v in dev[f32].items()}
        p.update({k: host[f32].data_ptr() if v is HOST else v for k, v in over.items() if k in ref.INPUTS})
        o = _BrightBandOut(**{n: (host[f32].data_ptr() if over.get("out_" + n) is HOST else outs[f32][n].data_ptr()) for n in names})
        c, g = cfg_of(**(cfg or {})), grids_of(grids)
        fn = L.kidmp32_bright_band_device if f32 else L.kidmp_bright_band_device
        return fn(m._h if m is not None else None, ncol, nz, *[p[k] for k in ref.INPUTS], C.byref(c), C.byref(g),
                  None if no_struct else C.byref(o), None)

    nan, inf = float("nan"), float("inf")
    refused = [
        dict(t=None), dict(p=None), dict(qv=None), dict(qr=None), dict(nr=None),
        dict(nz=1), dict(nz=257), dict(ncol=-1), dict(names=()), dict(no_struct=True),
        dict(cfg=dict(eps_w=complex(nan, 1.0))), dict(cfg=dict(eps_w=complex(80.0, inf))), dict(cfg=dict(eps_i=nan)),
        dict(cfg=dict(rho_w=0.0)), dict(cfg=dict(rho_w=-1.0)), dict(cfg=dict(rho_i=0.0)), dict(cfg=dict(rho_i=inf)),
        dict(cfg=dict(kw2=0.0)), dict(cfg=dict(kw2=nan)), dict(cfg=dict(topology=2)), dict(cfg=dict(topology=-1)),
        dict(grids={0: (True, False, 10)}), dict(grids={1: (False, True, 10)}), dict(grids={0: (True, True, 0)}),
        dict(grids={1: (True, True, 257)}), dict(grids={0: (HOST, True, 10)}),
        dict(t=HOST), dict(qg=HOST), dict(out_dbz=HOST), dict(out_fmelt_g=HOST), dict(out_k0=HOST),
    ]
    for f32 in (False, True):
        for kw in refused:
            assert call(gpu_mixed, f32, **kw) == EINVAL, (f32, kw)
            assert L.kidmp_last_error(gpu_mixed._h), kw
        assert call(None, f32) == ESTATE
    assert call(gpu_mixed, ncol=0) == 0 and call(gpu_mixed, ncol=0, t=None, names=()) == 0
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == -7).all() for f32 in (False, True) for o in outs[f32].values())
    # the host entries refuse alike
    hout = dict({n: np.full((ncol, nz), -7.0) for n in NUMBERS}, k0=np.full(ncol, -7, dtype=np.int32))

    def hcall(m, ncol=ncol, nz=nz, names=ref.NAMES, cfg=None, **over):
        p = {k: st[k].ctypes.data for k in ref.INPUTS}
        p.update(over)
        o = _BrightBandOut(**{n: hout[n].ctypes.data for n in names})
        c, g = cfg_of(**(cfg or {})), _BrightBandGrids()
        return L.kidmp_bright_band_host(m._h if m is not None else None, ncol, nz, *[p[k] for k in ref.INPUTS], C.byref(c), C.byref(g), C.byref(o))

    for kw in (dict(t=None), dict(nr=None), dict(nz=1), dict(nz=257), dict(ncol=-1), dict(names=()), dict(cfg=dict(rho_i=0.0)),
               dict(cfg=dict(topology=7))):
        assert hcall(gpu_mixed, **kw) == EINVAL, kw
    assert hcall(None) == ESTATE and hcall(gpu_mixed, ncol=0) == 0
    assert all((o == -7).all() for o in hout.values())
    # good calls afterwards still work; qs and qg may be left out
    want = _bb(gpu_mixed, st)
    assert call(gpu_mixed) == 0 and hcall(gpu_mixed) == 0
    torch.cuda.synchronize()
    assert all(_same(outs[False][n].cpu().numpy(), want[n]) and _same(hout[n], want[n]) for n in ref.NAMES)
    assert call(gpu_mixed, qs=None, qg=None) == 0 and call(gpu_mixed, grids={0: (True, True, 10)}) == 0
    torch.cuda.synchronize()
    assert (outs[False]["k0"].cpu().numpy()[:5] >= 0).all()                        # a grid of ones: finite work, the level unchanged
