"""The size spectra on the MI355X (include/kidmp_spectra.h, kidmp::k_size_spectra) against tests/size_spectra_ref.py.

Bounds (none is a measured number): every parameter within BOUND = 1e-12 relative, the bound the sibling tests hold the
fall speeds to.  Every bin within BOUND * (1 + nu + lam*D_b) relative plus FLOOR = 1e-250 absolute: a relative error eps in
a slope moves EXP(-lam*D) by eps*lam*D and D**nu-like factors by nu*eps (nu_c for cloud water, 3 + mu_s for snow, whose
ratio r = smob/smoc enters as r**3 * r**mu_s, with lam = r*Lam0); the floor covers a term that sits on the 700 threshold
in one of the two and not in the other (the largest such term is ~1e-253).  Absent species, sub-batches, subsets, the
binary32 entries, the host entries and graph replay are equalities of bits.  The tests print their measured maxima."""
import ctypes as C
import math

import numpy as np
import pytest

import cases
import effrad_cases as ec
import fall_cases as fc
import size_spectra_ref as ref

pytestmark = pytest.mark.gpu

BOUND, FLOOR = 1e-12, 1e-250
NZ_SWEEP = (2, 63, 64, 65, 120, 129, 256)
NCOL_SWEEP = (1, 5, 33)
NB_SWEEP = (1, 3, 100, 256)
EINVAL, ESTATE = -1, -5
ALL = ref.SPECIES + ref.PARAMS
FROZEN = ("i", "s", "g")


@pytest.fixture(scope="module")
def consts():
    return ref.constants()


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _dev(st, dtype=None):
    return {k: _cu(v if dtype is None else v.astype(dtype)) for k, v in st.items() if v is not None}


def _only(st):
    return {k: np.ascontiguousarray(st[k]) for k in ref.INPUTS}


def _after_one_step(m, st):
    """The state after one step of 10 s on the device (float64), as numpy arrays with the keys of INPUTS."""
    import torch
    dev = {k: _cu(v) for k, v in st.items()}
    ppt = torch.zeros(st["t"].shape[0], 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)
    torch.cuda.synchronize()
    return {k: dev[k].cpu().numpy() for k in ref.INPUTS}


def _with_cloud(st, seed):
    """fall_cases.scan_state has no cloud water: add some, switched on and off per level like the other species."""
    rng = np.random.Generator(np.random.PCG64(seed))
    shape = st["t"].shape
    qc = np.where(rng.uniform(size=shape) < 0.5, np.exp(rng.uniform(np.log(1e-9), np.log(3e-3), shape)), 0.0)
    qc[-3:] = 0.0
    qc[-3, -1] = 5.0e-4
    return _only(dict(st, qc=qc, nc=np.exp(rng.uniform(np.log(1e1), np.log(1e11), shape))))


def _edge_700():
    """Two hand-built columns that reach the 700 rule on the scheme's own grids.  Ice: a number so large that M:1432-1438
    limit it to xDi = 5 um, lami = 8e5 and lami*Di up to 783.  Cloud water: so little of it that lamc = 1.6e7 and lamc*Dc
    runs from 16 to 1 600."""
    nz = 8
    st = {k: np.zeros((2, nz)) for k in ref.INPUTS}
    st["t"][:], st["p"][:], st["qv"][:] = 255.0, 6.0e4, 1.0e-3
    rho = ec.rho_of(255.0)
    st["qi"][0] = np.logspace(-11, -8, nz)
    st["ni"][0] = 1.0e9 / rho
    st["qc"][1] = np.logspace(-11.5, -9, nz)
    st["nc"][:] = 1.0e8
    return st


@pytest.fixture(scope="module")
def sets(gpu_mixed, gpu_warm):
    """name -> (state, warm), built once and left unchanged."""
    s = {
        "config3": (_after_one_step(gpu_mixed, cases.config3(24)), False),
        "config5": (_after_one_step(gpu_mixed, cases.config5(24)), False),
        "config2": (_after_one_step(gpu_warm, cases.config2(24)), True),
        "hand_built": (_only(ec.stack(ec.hand_built())), False),
        "fall_hand_built": (_with_cloud(fc.scan_state(65, 12, 765), 31), False),
        "edge_700": (_edge_700(), False),
    }
    for seed in (271, 272):
        s["random65_%d" % seed] = (_only(ec.random_state(65, 33, seed)), False)
    return s


@pytest.fixture(scope="module")
def refs(sets, consts):
    return {k: ref.size_spectra(consts, st, warm=warm) for k, (st, warm) in sets.items()}


@pytest.fixture(autouse=True)
def _leave_contexts_as_found(gpu_mixed, gpu_warm):
    yield
    for m in (gpu_mixed, gpu_warm):
        m.set_host_chunk(0)
        m.set_column_nc(None)


def _spectra(m, st, want=ALL, grids=None, dtype=None, **kw):
    import torch
    g = None if grids is None else {x: (_cu(D), _cu(dD)) for x, (D, dD) in grids.items()}
    out = m.size_spectra(_dev(st, dtype), want, g, **kw)
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


def check_parity(got, want, names=ALL):
    """Asserts the bounds of the module docstring and the exact zeros; returns the measured maxima relative to each bound."""
    worst = {}
    for n in names:
        g = got[n]
        assert np.isfinite(g).all() and not np.signbit(g).any(), n
        if n in ref.PARAMS:
            x = [s for s in ref.SPECIES if n in ref.PARAMS_OF[s]][0]
            has = want["has_" + x]
            assert not _bits(g)[~has].any(), n                                   # +0.0 where the species is absent
            assert (g[has] > 0).all(), n
            err = np.abs(g - want[n]) / np.where(has, np.abs(want[n]), 1.0)
            assert (err <= BOUND).all(), (n, float(err.max()))
            worst[n] = float(err.max() / BOUND) if err.size else 0.0
        else:
            has = np.broadcast_to(want["has_" + n][..., None, :], g.shape)
            assert not _bits(g)[~has].any(), n                                   # +0.0 in every bin of an absent species
            tol = BOUND * (1.0 + want[n + "_nu"] + want[n + "_arg"]) * np.abs(want[n]) + FLOOR
            err = np.abs(g - want[n])
            assert (err <= tol).all(), (n, float((err / tol).max()))
            worst[n] = float((err / tol).max()) if err.size else 0.0
    return worst


# ---- 1. parity on the sets ----
@pytest.mark.parametrize("name", ["config3", "config5", "config2", "hand_built", "fall_hand_built", "random65_271", "random65_272", "edge_700"])
def test_parity(request, sets, refs, name):
    st, warm = sets[name]
    m = request.getfixturevalue("gpu_warm" if warm else "gpu_mixed")
    got = _spectra(m, st)
    worst = check_parity(got, refs[name])
    print("size spectra %s: max error / bound %s" % (name, {k: "%.3f" % v for k, v in worst.items()}))
    if name.startswith("random") or name == "config3":
        assert all((got[x] > 0).any() for x in ref.SPECIES), name
    if warm:
        assert not any(got[n].any() for x in FROZEN for n in (x,) + ref.PARAMS_OF[x])


def test_the_700_rule(gpu_mixed, sets, refs):
    got, want = _spectra(gpu_mixed, sets["edge_700"][0], want=("i", "c", "lam_i", "lam_c")), refs["edge_700"]
    for x, col in (("i", 0), ("c", 1)):
        arg, N = want[x + "_arg"][col], got[x][col]
        assert arg.max() > 780 and (arg > 700).sum() > 10 and ((arg > 1) & (arg < 600)).sum() > 10, x
        clear = (arg > 700 * (1 + 1e-9)) | (arg == 0)
        assert not _bits(N)[clear].any(), x                                       # exact +0.0 past the threshold
        assert (N[(arg > 0) & (arg < 700 * (1 - 1e-9))] > 1e-300).all(), x        # a normal number below it
    assert want["c_arg"][1].max() > 1500


def test_default_grids_are_the_references(gpu_mixed, gpu_warm):
    from kid_amd import default_grid
    own = ref.default_grids()
    for x in ref.SPECIES:
        D, dD = default_grid(gpu_mixed, x)
        tol = 0.0 if x == "c" else 2e-14                                         # as test_reference_grids_equal_the_oracles
        assert D.shape == dD.shape == (100,) and np.abs(D / own[x][0] - 1).max() <= tol and np.abs(dD / own[x][1] - 1).max() <= tol, x
        assert _same(D, gpu_mixed.const("D" + x)) and _same(dD, gpu_mixed.const("dt" + x)), x
        assert _same(D, default_grid(gpu_warm, x)[0])


# ---- 2. shapes: levels, columns, bins ----
def _sweep_grids(nbs):
    """species -> (D, dD) with nbs[species] bins, log-spaced over the species' own range; None keeps the scheme's grid."""
    own = ref.default_grids()
    g = {}
    for x, nb in nbs.items():
        if nb is None:
            continue
        lo, hi = own[x][0][0], own[x][0][-1]
        edges = np.exp(np.linspace(np.log(lo), np.log(hi), nb + 1))
        g[x] = (np.ascontiguousarray(np.sqrt(edges[:-1] * edges[1:])), np.ascontiguousarray(np.diff(edges)))
    return g


@pytest.mark.parametrize("nz", NZ_SWEEP)
def test_level_and_column_shapes(gpu_mixed, consts, nz):
    m = gpu_mixed
    st = _only(ec.random_state(nz, max(NCOL_SWEEP), 900 + nz))
    grids = _sweep_grids(dict(c=None, i=3, r=256, s=1, g=100))
    whole = _spectra(m, st, grids=grids)
    assert [whole[x].shape[1] for x in ref.SPECIES] == [100, 3, 256, 1, 100] and whole["r"].shape == (33, 256, nz)
    check_parity(whole, ref.size_spectra(consts, st, grids=grids))
    assert _same_all(whole, _spectra(m, st, grids=grids)), "a repeated call"
    for ncol in NCOL_SWEEP[:-1]:
        idx = (np.arange(ncol) * 7 + nz) % 33                                    # other positions in another batch
        assert _same_all(_spectra(m, _take(st, idx), grids=grids), {k: v[idx] for k, v in whole.items()}), (nz, ncol)


@pytest.mark.parametrize("nb", NB_SWEEP)
def test_bin_counts(gpu_mixed, consts, nb):
    st = _only(ec.random_state(65, 5, 1100 + nb))
    grids = _sweep_grids({x: nb for x in ref.SPECIES})
    got = _spectra(gpu_mixed, st, grids=grids)
    assert all(got[x].shape == (5, nb, 65) for x in ref.SPECIES)
    check_parity(got, ref.size_spectra(consts, st, grids=grids))


def test_bits_do_not_depend_on_how_bins_are_dealt(gpu_mixed, consts):
    """4 100 columns fill the grid with one share of the bins per column; five of them alone are dealt bin by bin."""
    nz, ncol = 3, 4100
    st = _only(ec.random_state(nz, ncol, 1201))
    grids = _sweep_grids(dict(r=3, s=3))
    whole = _spectra(gpu_mixed, st, want=("r", "s", "n0_r"), grids=grids)
    check_parity(whole, ref.size_spectra(consts, st, want=("r", "s"), grids=grids), ("r", "s", "n0_r"))
    idx = np.array([0, 1027, 2048, 4095, 4099])
    assert _same_all(_spectra(gpu_mixed, _take(st, idx), want=("r", "s", "n0_r"), grids=grids), {k: v[idx] for k, v in whole.items()})


# ---- 3. options ----
def test_subsets_sentinels_and_the_default_grid_given_by_the_caller(gpu_mixed, sets):
    import torch
    from kid_amd import default_grid
    from kid_amd.spectra import _SpectraBins, _SpectraGrids, _SpectraOut, library
    m = gpu_mixed
    st, _ = sets["random65_271"]
    full = _spectra(m, st)
    for names in (("r",), ("lam_r",), ("nu_c", "s"), ref.PARAMS, ref.SPECIES[::-1], ("g", "n0_g"), ("c", "i")):
        part = _spectra(m, st, want=names)
        assert sorted(part) == sorted(names) and all(_same(part[n], full[n]) for n in names), names
    own = {x: default_grid(m, x) for x in ref.SPECIES}
    assert _same_all(_spectra(m, st, want=ref.SPECIES, grids=own), {x: full[x] for x in ref.SPECIES}), "the default grid, handed in"
    # `out`: written in place; what was not requested is untouched (the raw entry on sentinel-filled arrays)
    dev = _dev(st)
    pre = {"r": torch.full((33, 100, 65), -7.0, dtype=torch.float64, device="cuda:0")}
    res = m.size_spectra(dev, ("r", "lam_g"), out=pre)
    torch.cuda.synchronize()
    assert res["r"] is pre["r"] and _same(pre["r"].cpu().numpy(), full["r"]) and _same(res["lam_g"].cpu().numpy(), full["lam_g"])
    outs = {n: torch.full((33, 65) if n in ref.PARAMS else (33, 100, 65), -7.0, dtype=torch.float64, device="cuda:0") for n in ALL}
    asked = ("smoc", "n0_c", "i")
    par = _SpectraOut(**{n: outs[n].data_ptr() for n in asked if n in ref.PARAMS})
    bins = _SpectraBins(n_i=outs["i"].data_ptr())
    rc = library().kidmp_size_spectra_device(m._h, 33, 65, *[dev[k].data_ptr() for k in ref.INPUTS], C.byref(par), C.byref(bins), None, None)
    torch.cuda.synchronize()
    assert rc == 0
    for n in ALL:
        a = outs[n].cpu().numpy()
        assert _same(a, full[n]) if n in asked else (a == -7.0).all(), n
    # a grid structure whose members are all NULL is the default as well
    g = _SpectraGrids()
    assert library().kidmp_size_spectra_device(m._h, 33, 65, *[dev[k].data_ptr() for k in ref.INPUTS], None, C.byref(bins), C.byref(g), None) == 0
    torch.cuda.synchronize()
    assert _same(outs["i"].cpu().numpy(), full["i"])


def test_binary32_entries_round_once(gpu_mixed, gpu_warm, sets):
    grids = _sweep_grids(dict(r=7))
    randoms = {"random%d" % nz: _only(ec.random_state(nz, 5, 900 + nz)) for nz in (2, 129, 256)}  # one, three and four level groups
    for name, m in (("config3", gpu_mixed), ("random65_272", gpu_mixed), ("config2", gpu_warm)) + tuple((n, gpu_mixed) for n in randoms):
        st = {k: v.astype(np.float32) for k, v in (randoms[name] if name in randoms else sets[name][0]).items()}
        wide = {k: v.astype(np.float64) for k, v in st.items()}
        got = _spectra(m, st, grids=grids)
        ref64 = _spectra(m, wide, grids=grids)
        for n in ALL:
            with np.errstate(over="ignore"):                                     # n0_c can lie beyond binary32: +inf in both
                rounded = ref64[n].astype(np.float32)
            assert got[n].dtype == np.float32 and _same(got[n], rounded), (name, n)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_entries_equal_the_device_entry(gpu_mixed, sets, dtype):
    m = gpu_mixed
    st = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in sets["random65_271"][0].items()}
    ncol = st["t"].shape[0]
    grids = _sweep_grids(dict(i=5, g=256))
    want = _spectra(m, st, grids=grids)
    some = ("s", "lam_c", "g")
    for chunk in (0, 1, 7, ncol):
        m.set_host_chunk(chunk)
        assert _same_all(m.size_spectra_host(st, ALL, grids), want), chunk
        assert _same_all(m.size_spectra_host(st, some, grids), {n: want[n] for n in some}), chunk
    m.set_host_chunk(7)
    pre = {"r": np.full((ncol, 100, 65), -7.0, dtype=dtype)}
    res = m.size_spectra_host({k: v for k, v in st.items() if k != "nc"}, ("r",), out=pre)
    assert res["r"] is pre["r"] and _same(pre["r"], want["r"])


def test_hip_graph_replay_of_one_captured_launch(gpu_mixed, sets):
    import torch
    m = gpu_mixed
    st, _ = sets["config3"]
    names = ("r", "s", "lam_g", "nu_c", "c")
    dev = _dev(st)
    shapes = {n: (24, 120) if n in ref.PARAMS else (24, 100, 120) for n in names}
    out = {n: torch.full(shapes[n], -7.0, dtype=torch.float64, device="cuda:0") for n in names}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.size_spectra(dev, names, out=out)
    eager = _spectra(m, st, want=names)
    for _ in range(2):
        for o in out.values():
            o.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert all(_same(out[n].cpu().numpy(), eager[n]) for n in names)


def test_warm_context_ignores_and_omits_the_frozen_inputs(gpu_warm, sets):
    st, _ = sets["config2"]
    full = _spectra(gpu_warm, st)
    liquid = {k: v for k, v in st.items() if k not in ("qi", "ni", "qs", "qg", "nc")}
    assert _same_all(full, _spectra(gpu_warm, liquid))
    for x in FROZEN:
        assert not any(_bits(full[n]).any() for n in (x,) + ref.PARAMS_OF[x]), x   # +0.0
    some = _spectra(gpu_warm, liquid, want=("r", "lam_c"))
    assert sorted(some) == ["lam_c", "r"] and _same(some["r"], full["r"]) and (full["r"] > 0).any() and (full["c"] > 0).any()


def test_a_bound_droplet_number_changes_cloud_water_and_nothing_else(gpu_mixed, sets, consts):
    st, _ = sets["random65_272"]
    ncol = st["t"].shape[0]
    plain = _spectra(gpu_mixed, st)
    nd = np.exp(np.linspace(np.log(5.0), np.log(3000.0), ncol))                  # cm-3: nu_c runs from 15 down to 2
    gpu_mixed.set_column_nc(nd)
    bound = _spectra(gpu_mixed, st)
    gpu_mixed.set_column_nc(None)
    for n in ALL:
        if n in ("c",) + ref.PARAMS_OF["c"]:
            assert not _same(bound[n], plain[n]), n
        else:
            assert _same(bound[n], plain[n]), n
    want = ref.size_spectra(consts, st, want=("c",), Nt_c=(nd * 1.e6)[:, None])
    worst = check_parity(bound, want, ("c",) + ref.PARAMS_OF["c"])
    print("per-column droplet number: max error / bound %s" % {k: "%.3f" % v for k, v in worst.items()})
    assert set(np.unique(bound["nu_c"])) >= {0.0, 2.0, 15.0}
    assert _same_all(_spectra(gpu_mixed, st), plain), "unbound again"


def test_aerosol_aware_context_limits_the_droplet_number(gpu_mixed_aero, sets, consts):
    st = _only(ec.stack([ec.hand_built(64)[k] for k in ("nc_sweep", "qc_sweep")]))
    got = _spectra(gpu_mixed_aero, st, want=("c",) + ref.PARAMS_OF["c"])
    want = ref.size_spectra(consts, st, want=("c",), aero=True)
    worst = check_parity(got, want, ("c",) + ref.PARAMS_OF["c"])
    print("aerosol-aware: max error / bound %s" % {k: "%.3f" % v for k, v in worst.items()})
    assert len(np.unique(got["nu_c"])) > 3


# ---- 4. cross-checks against entries that already exist ----
def test_slopes_give_the_fall_speeds_and_the_radius_of_the_existing_entries(gpu_mixed, sets):
    import torch
    m = gpu_mixed
    st, _ = sets["random65_271"]
    dev = _dev(st)
    par = {k: v.cpu().numpy() for k, v in m.size_spectra(dev, ("lam_r", "lam_i", "lam_c", "nu_c")).items()}
    fall = {k: v.cpu().numpy() for k, v in m.fall_speeds({k: dev[k] for k in fc.KEYS}, want=("vt_r", "vt_i")).items()}
    re_qc = m.effective_radii(dev)[0].cpu().numpy()
    torch.cuda.synchronize()
    rho = 0.622 * st["p"] / (ref.fr.R * st["t"] * (np.maximum(1e-10, st["qv"]) + 0.622))
    rhof = np.sqrt(ref.fr.RHO_NOT / rho)
    crg6, org3, cig3, oig2 = math.gamma(5.0), 1.0 / math.gamma(4.0), math.gamma(5.0), 1.0 / math.gamma(4.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        has = (par["lam_r"] > 0) & (st["qr"] * rho > ref.R1)
        lamr = par["lam_r"]
        vtr = rhof * ref.fr.av_r * crg6 * org3 * lamr ** 4.0 / (lamr + ref.fr.fv_r) ** 5.0       # cre(3) = 4, cre(6) = 5
        e_r = np.abs(vtr / fall["vt_r"] - 1)[has]
        has_i = (par["lam_i"] > 0) & (st["qi"] * rho > ref.R1)
        vti = rhof * ref.fr.av_i * cig3 * oig2 / par["lam_i"]
        e_i = np.abs(vti / fall["vt_i"] - 1)[has_i]
        has_c = (par["lam_c"] > 0) & (st["qv"] >= 1e-10)                         # calc_effectRad does not clamp qv
        re = np.maximum(2.51e-6, np.minimum(0.5 * (3.0 + par["nu_c"]) / par["lam_c"], 50e-6))
        e_c = np.abs(re / re_qc - 1)[has_c]
    print("cross-checks: vt_r %.2e over %d levels, vt_i %.2e over %d, re_qc %.2e over %d" % (e_r.max(), e_r.size, e_i.max(), e_i.size, e_c.max(), e_c.size))
    assert e_r.size > 300 and e_i.size > 300 and e_c.size > 300
    assert e_r.max() <= BOUND and e_i.max() <= BOUND and e_c.max() <= BOUND
    assert (re[has_c] > 2.51e-6).any() and (re[has_c] < 50e-6).any()


# ---- 5. refusals ----
HOST = "a pageable host array"


def test_refusals_write_nothing(gpu_mixed, gpu_warm, gpu_mixed_aero, sets):
    import torch
    from kid_amd.spectra import _SpectraBins, _SpectraGrids, _SpectraOut, library
    L = library()
    st = _take(sets["config3"][0], slice(0, 6))
    ncol, nz, nb = 6, 120, 4
    D_np, dD_np = _sweep_grids(dict(r=nb))["r"]
    dev = {False: dict(_dev(st), D=_cu(D_np), dD=_cu(dD_np))}
    dev[True] = {k: (v.float() if k in ref.INPUTS else v) for k, v in dev[False].items()}
    host = {False: torch.zeros(ncol * 100 * nz, dtype=torch.float64), True: torch.zeros(ncol * 100 * nz, dtype=torch.float32)}
    outs = {f32: {n: torch.full((ncol, nz) if n in ref.PARAMS else (ncol, 100, nz), -7.0, dtype=torch.float32 if f32 else torch.float64,
                                device="cuda:0") for n in ALL} for f32 in (False, True)}
    DEFAULT = object()

    def call(m, f32=False, ncol=ncol, nz=nz, names=ALL, grid=DEFAULT, no_structs=False, **over):
        p = {k: v.data_ptr() for k, v in dev[f32].items()}
        p.update({k: host[f32].data_ptr() if v is HOST else v for k, v in over.items() if k in ref.INPUTS})
        o = {n: (host[f32].data_ptr() if over.get("out_" + n) is HOST else outs[f32][n].data_ptr()) for n in names}
        par = _SpectraOut(**{n: a for n, a in o.items() if n in ref.PARAMS})
        bins = _SpectraBins(**{"n_" + n: a for n, a in o.items() if n in ref.SPECIES})
        g = _SpectraGrids()
        if grid is not DEFAULT:                                                  # (D, dD, nb) of rain
            g.D[2], g.dD[2], g.nb[2] = [host[False].data_ptr() if a is HOST else a for a in grid]
        fn = L.kidmp32_size_spectra_device if f32 else L.kidmp_size_spectra_device
        return fn(m._h if m is not None else None, ncol, nz, *[p[k] for k in ref.INPUTS], None if no_structs else C.byref(par),
                  None if no_structs else C.byref(bins), C.byref(g), None)

    D, dD = dev[False]["D"].data_ptr(), dev[False]["dD"].data_ptr()
    refused = [
        dict(t=None), dict(p=None), dict(qv=None), dict(qc=None), dict(qr=None), dict(nr=None),
        dict(qi=None), dict(ni=None), dict(qs=None), dict(qg=None),               # a frozen output is wanted in a mixed-phase context
        dict(nz=1), dict(nz=257), dict(ncol=-1),
        dict(names=()), dict(no_structs=True),                                   # nothing requested at all
        dict(grid=(D, dD, 0)), dict(grid=(D, dD, 257)), dict(grid=(D, dD, -1)), dict(grid=(D, None, nb)), dict(grid=(None, dD, nb)),
        dict(t=HOST), dict(qg=HOST), dict(qc=HOST), dict(out_r=HOST), dict(out_lam_c=HOST), dict(grid=(HOST, dD, nb)), dict(grid=(D, HOST, nb)),
    ]
    for f32 in (False, True):
        for kw in refused:
            assert call(gpu_mixed, f32, **kw) == EINVAL, (f32, kw)
            assert L.kidmp_last_error(gpu_mixed._h), kw
        assert call(gpu_warm, f32, qr=None) == EINVAL and call(gpu_mixed_aero, f32, nc=None) == EINVAL
        assert call(None, f32) == ESTATE
    assert call(gpu_mixed, ncol=0) == 0 and call(gpu_mixed, ncol=0, t=None, names=()) == 0
    gpu_mixed.set_column_nc(np.full(ncol + 1, 80.0))
    assert call(gpu_mixed) == EINVAL and call(gpu_mixed, names=("r", "lam_i")) == 0   # the binding is cloud water's alone
    gpu_mixed.set_column_nc(None)
    torch.cuda.synchronize()
    for f32 in (False, True):
        assert all((o.cpu().numpy() == -7.0).all() for n, o in outs[f32].items() if not (n in ("r", "lam_i") and not f32))
    # the host entries refuse alike
    hout = {n: np.full((ncol, nz) if n in ref.PARAMS else (ncol, 100, nz), -7.0) for n in ALL}

    def hcall(m, ncol=ncol, nz=nz, names=ALL, grid=DEFAULT, **over):
        p = {k: st[k].ctypes.data for k in ref.INPUTS}
        p.update(over)
        par = _SpectraOut(**{n: hout[n].ctypes.data for n in names if n in ref.PARAMS})
        bins = _SpectraBins(**{"n_" + n: hout[n].ctypes.data for n in names if n in ref.SPECIES})
        g = _SpectraGrids()
        if grid is not DEFAULT:
            g.D[2], g.dD[2], g.nb[2] = grid
        return L.kidmp_size_spectra_host(m._h if m is not None else None, ncol, nz, *[p[k] for k in ref.INPUTS], C.byref(par), C.byref(bins),
                                         C.byref(g))

    for kw in (dict(t=None), dict(qc=None), dict(qi=None), dict(qg=None), dict(nz=1), dict(nz=257), dict(ncol=-1), dict(names=()),
               dict(grid=(D_np.ctypes.data, dD_np.ctypes.data, 257)), dict(grid=(D_np.ctypes.data, None, nb))):
        assert hcall(gpu_mixed, **kw) == EINVAL, kw
    assert hcall(None) == ESTATE and hcall(gpu_mixed, ncol=0) == 0
    assert all((o == -7.0).all() for o in hout.values())
    # good calls afterwards still work; inputs that no wanted output reads may be left out
    want = _spectra(gpu_mixed, st)
    assert call(gpu_mixed) == 0 and hcall(gpu_mixed) == 0
    torch.cuda.synchronize()
    assert all(_same(outs[False][n].cpu().numpy(), want[n]) and _same(hout[n], want[n]) for n in ALL)
    assert call(gpu_mixed, names=("r", "c", "n0_r"), qi=None, ni=None, qs=None, qg=None, nc=None) == 0
    assert call(gpu_warm, qi=None, ni=None, qs=None, qg=None, nc=None) == 0
    assert call(gpu_mixed, names=("r", "lam_r"), grid=(D, dD, nb)) == 0
    torch.cuda.synchronize()
    narrow = _spectra(gpu_mixed, st, want=("r",), grids={"r": (D_np, dD_np)})["r"]
    assert _same(outs[False]["r"].cpu().numpy().reshape(-1)[:ncol * nb * nz].reshape(ncol, nb, nz), narrow)
