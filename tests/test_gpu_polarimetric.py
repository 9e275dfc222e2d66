"""The polarimetric radar on the MI355X (include/kidmp_polarimetric.h, kidmp::k_polarimetric) against
tests/polarimetric_ref.py, which takes the library's own table through kidmp_pol_table_get and restates the load, the
ascending-bin sums and the carriers in the kernel's order.  The states are those of tests/mie_radar_cases.py: seven kinds
of column (mixed-phase with a melting level, warm rain, cold snow and graupel without rain, every species at every level
below the top, snow alone at the melting level, a dry column, every species at every level), picked round-robin.

Exact: the sphere limit (every axis ratio 1: dbz_h and dbz_h_x are kidmp_reflectivity_device's and
kidmp_doppler_moments_device's closed-form bits, every zdr and kdp is +0.0, rhohv is 1.0, for the looped species and the
uniform one alike); absent species and an iiwarm context; kw2 changes no bit, the wavelength none but kdp's; every
equality between two device results (subsets, positions, repeats, binary32 after one rounding, the host entries, graph
replay); refusals write nothing.

Against the restatement, at every element: dbz_h* and zdr* as the relative difference of the linear quantity they stand
for (|d dB| ln(10)/10), kdp* relative where the reference is not zero, rhohv absolute.  The bound is four times MEASURED,
the largest difference over every shape, grid and context of this file on the MI355X:
    dbz_h, dbz_h_x 6.6e-15 (6.54e-15)    zdr, zdr_x 2.1e-15 (2.06e-15)    kdp, kdp_x 3.0e-15 (2.97e-15)    rhohv 1.7e-15 (1.67e-15)
so the bounds are 2.6e-14, 8.4e-15, 1.2e-14 and 6.8e-15.  Kernel and reference form the slopes by different routes (fastmath
pow and cube root against numpy's **), and an ulp of a slope is up to lam*D ulp of exp(-lam*D) in a bin; every output is a
ratio of two sums weighed by the same density, which cancels most of it, and dbz_h is the two ulp of a dBZ near 50 that
tests/test_gpu_mie_radar.py records.  All are far below 1e-11.  (sigma = 10 rad: zdr measured 0.0 exactly.)

force_quadrature = 1 against the default table, for graupel: the uniform route takes the ratios of the first bin's rows,
the other the ratios of the sums, which are the same number up to the rounding of each bin's rows.  The measurement is what
the restatement gives for the two routes on the 120-level state of this file (QUADRATURE: dbz_h 3.3e-15, zdr 1.3e-15,
kdp 2.2e-15 relative, rhohv 1.3e-15); the device's two tables differ by at most four times that.

With only rain present dbz_h is not dbz_h_r bit for bit: as in kidmp_reflectivity_device an absent species still adds its
1.E-22 to the sum (M:5127-5136), which the sphere limit's bit equality needs; the test holds dbz_h to
10 log10(zh_r + 2e-22) formed from dbz_h_r.
"""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import doppler_ref as dref
import polarimetric_ref as ref
import refl_oracle as ro
from mie_radar_cases import state

pytestmark = pytest.mark.gpu

# the largest differences from the restatement measured on the MI355X (see the module docstring)
MEASURED = {"dbz_h": 6.6e-15, "zdr": 2.1e-15, "kdp": 3.0e-15, "rhohv": 1.7e-15}
# the restatement's uniform route against its quadrature, graupel
QUADRATURE = {"dbz_h": 3.3e-15, "zdr": 1.3e-15, "kdp": 2.2e-15, "rhohv": 1.3e-15}
NZS = (2, 33, 64, 65, 120, 129, 200, 256)
SHAPES = [(nz, ncol) for nz in NZS for ncol in (1, 5)] + [(120, 257), (200, 18)]
WORST = {k: 0.0 for k in MEASURED}
SPHERES = dict(axis_r=(1.0, 0.0, 0.0, 0.0, 0.0), axis_s=1.0, axis_g=1.0)


def bound(kind):
    return 4.0 * MEASURED[kind]


def _kp():
    return importlib.import_module("kid_amd.polarimetric")


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _dev(st, dtype=None):
    return {k: _cu(v if dtype is None else v.astype(dtype)) for k, v in st.items() if v is not None}


def _run(m, table, st, want=ref.NAMES, dtype=None):
    import torch
    out = m.polarimetric(table, _dev(st, dtype), want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_all(a, b):
    return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)


def _take(st, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}


def _state(nz, ncol=7):
    """ncol columns [ncol, nz] of the seven kinds, starting with the one that holds every species at every level."""
    st = state(nz)[0]
    idx = (6 + np.arange(ncol)) % 7
    return {k: np.ascontiguousarray(st[k][idx]) for k in ref.INPUTS}


def _get(table):
    return {x: table.get(x) for x in ref.SPECIES}


@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = dref.constants(o)
    o.close()
    return c


@pytest.fixture(scope="module")
def tables(gpu_mixed):
    """name -> (PolTable, its rows as the device holds them): the defaults, the defaults with every species walking its
    bins, and spheres."""
    from kid_amd import PolCfg
    out = {}
    for name, kw in (("default", {}), ("quadrature", dict(force_quadrature=True)), ("spheres", SPHERES)):
        t = gpu_mixed.pol_table(None, PolCfg(**kw))
        out[name] = (t, _get(t))
    yield out
    for t, _ in out.values():
        t.close()


@pytest.fixture(scope="module")
def main_set(consts, tables):
    st = _state(120)
    return st, ref.polarimetric(consts, 0.10, tables["default"][1], st)


@pytest.fixture(autouse=True)
def _leave_contexts_as_found(gpu_mixed, gpu_warm):
    yield
    for m in (gpu_mixed, gpu_warm):
        m.set_host_chunk(0)


def differences(got, want):
    """The largest difference of every kind between two sets of outputs, at every element."""
    worst = {k: 0.0 for k in MEASURED}
    for n in ref.NAMES:
        if n not in got:
            continue
        g, w = got[n], want[n]
        assert np.isfinite(g).all(), n
        if n.startswith("dbz_h") or n.startswith("zdr"):
            kind, d = ("dbz_h" if n.startswith("dbz_h") else "zdr"), np.abs(g - w) * (math.log(10.0) / 10.0)
        elif n.startswith("kdp"):
            assert (g[w == 0.0] == 0.0).all(), n
            kind, d = "kdp", np.abs(g - w) / np.where(w != 0.0, np.abs(w), 1.0)
        else:
            kind, d = "rhohv", np.abs(g - w)
        worst[kind] = max(worst[kind], float(d.max()))
    return worst


def check_parity(got, want):
    """Every output against the restatement at the module's bounds; prints the measured maxima and keeps the file's."""
    worst = differences(got, want)
    for k, v in worst.items():
        WORST[k] = max(WORST[k], v)
    print("measured", {k: "%.2e" % v for k, v in worst.items()}, "so far", {k: "%.2e" % v for k, v in WORST.items()})
    for k, v in worst.items():
        assert v <= bound(k), (k, v)


def check_identities(got, st):
    """What holds on any state."""
    for x, q, lim in (("r", "qr", 1e-12), ("s", "qs", 1e-6), ("g", "qg", 1e-6)):
        absent = ~(st[q] > lim)
        assert (_bits(got["kdp_" + x])[absent] == 0).all() and (_bits(got["zdr_" + x])[absent] == 0).all(), x
        assert (got["dbz_h_" + x][absent] == got["dbz_h_" + x][absent][:1]).all() if absent.any() else True
        assert (got["kdp_" + x] >= 0).all() and (got["zdr_" + x] >= 0).all(), x       # oblate, symmetry axis vertical in the mean
    assert (got["rhohv"] <= 1.0).all() and (got["rhohv"] > 0.9).all() and np.isfinite(got["rhohv"]).all()
    assert _same(got["kdp"], (got["kdp_r"] + got["kdp_s"]) + got["kdp_g"])


# ---- 1. shapes and grids against the restatement ----
@pytest.mark.parametrize("nz, ncol", SHAPES)
def test_shapes_against_the_restatement(gpu_mixed, consts, tables, nz, ncol):
    table, rows = tables["default"]
    st = _state(nz, ncol)
    want = ref.polarimetric(consts, 0.10, rows, st)
    got = _run(gpu_mixed, table, st)
    assert sorted(got) == sorted(ref.NAMES) and all(v.shape == (ncol, nz) for v in got.values())
    check_parity(got, want)
    check_identities(got, st)
    rain = st["qr"] > 1e-12
    if rain.any():                                               # the shapes matter: rain's zdr leaves 0 by a tenth of a dB somewhere
        assert got["zdr_r"][rain].max() > 0.1 and got["kdp_r"][rain].max() > 0.0


@pytest.mark.parametrize("nb", [1, 65, 256])
def test_the_callers_grids(gpu_mixed, consts, nb):
    from kid_amd import PolCfg
    st = _state(65)
    edges = {"r": (5e-5, 6e-3), "s": (2e-4, 2e-2), "g": (2.5e-4, 4e-2)}
    grids = {}
    for x, (lo, hi) in edges.items():
        e = np.exp(np.linspace(np.log(lo), np.log(hi), nb + 1))
        grids[x] = (np.ascontiguousarray(np.sqrt(e[:-1] * e[1:])), np.ascontiguousarray(e[1:] - e[:-1]))
    for quad in (False, True):
        with gpu_mixed.pol_table(None, PolCfg(force_quadrature=quad), grids) as t:
            rows = _get(t)
            for x in ref.SPECIES:
                assert rows[x][2].shape == (7, nb) and _same(rows[x][0], grids[x][0]) and _same(rows[x][1], grids[x][1])
                assert rows[x][3] == (x == "g" and not quad)
            got = _run(gpu_mixed, t, st)
        check_parity(got, ref.polarimetric(consts, 0.10, rows, st))
        check_identities(got, st)


def test_the_table_is_the_host_entrys(gpu_mixed, tables):
    """kidmp_pol_table_get returns what kidmp_pol_bins forms on the scheme's own bins, bit for bit; graupel alone is
    uniform, never under force_quadrature; the scalars are the ratios of the first bin's rows."""
    from kid_amd import MieCfg, PolCfg, default_grid, pol_bins
    for name, kw in (("default", {}), ("quadrature", dict(force_quadrature=True)), ("spheres", SPHERES)):
        t, rows = tables[name]
        for x in ref.SPECIES:
            D, dD = default_grid(gpu_mixed, x)
            assert _same(rows[x][0], np.asarray(D)) and _same(rows[x][1], np.asarray(dD))
            assert _same(rows[x][2], pol_bins(MieCfg(), PolCfg(**kw), x, rows[x][0])), (name, x)
            assert rows[x][3] == (x == "g" and name != "quadrature"), (name, x)
            assert _same(rows[x][4], ref.scalars(rows[x][2])), (name, x)
        mie, pol = t.cfg
        assert (mie.wavelength, mie.rho_i, pol.axis_s, pol.force_quadrature) == (0.10, 900.0, kw.get("axis_s", 0.75), name == "quadrature")
    sph = tables["spheres"][1]
    for x in ref.SPECIES:
        assert sph[x][4].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0] and (_bits(sph[x][4])[3:] == 0).all()


def test_force_quadrature_against_the_default_table(gpu_mixed, consts, tables, main_set):
    """Graupel by its scalars and by its bins: the two routes of the restatement differ by QUADRATURE, the device's by at
    most four times that; rain and snow keep their bits."""
    st, want = main_set
    (t_def, rows_def), (t_quad, rows_quad) = tables["default"], tables["quadrature"]
    route = differences(ref.polarimetric(consts, 0.10, rows_def, st), ref.polarimetric(consts, 0.10, rows_def, st, quadrature=True))
    print("the restatement's two routes", {k: "%.2e" % v for k, v in route.items()})
    for k in QUADRATURE:
        assert route[k] <= QUADRATURE[k], (k, route[k])
    a, b = _run(gpu_mixed, t_def, st), _run(gpu_mixed, t_quad, st)
    for n in ("dbz_h_r", "dbz_h_s", "zdr_r", "zdr_s", "kdp_r", "kdp_s"):
        assert _same(a[n], b[n]), n
    dev = differences(a, b)
    print("the device's two tables", {k: "%.2e" % v for k, v in dev.items()})
    for k in QUADRATURE:
        assert dev[k] <= 4.0 * QUADRATURE[k], (k, dev[k])
    check_parity(b, ref.polarimetric(consts, 0.10, rows_quad, st))
    assert (a["zdr_g"][st["qg"] > 1e-6] > 0.05).all()            # graupel is not a sphere in either


# ---- 2. exact ----
@pytest.mark.parametrize("quad", [False, True])
@pytest.mark.parametrize("sigma", [(0.0, 0.0, 0.0), (0.3, 1.0, 2.0)])
def test_sphere_limit_is_the_reflectivity(gpu_mixed, sigma, quad):
    import torch
    from kid_amd import PolCfg
    for nz in (65, 200):
        st = _state(nz)
        with gpu_mixed.pol_table(None, PolCfg(sigma=sigma, force_quadrature=quad, **SPHERES)) as t:
            assert t.get("g")[3] == (not quad)
            got = _run(gpu_mixed, t, st)
        dev = _dev(st)
        plain = gpu_mixed.reflectivity(dev)
        parts = gpu_mixed.doppler_moments(dev, want=("dbz_r", "dbz_s", "dbz_g"))
        torch.cuda.synchronize()
        assert _same(got["dbz_h"], plain.cpu().numpy())
        for x in ref.SPECIES:
            assert _same(got["dbz_h_" + x], parts["dbz_" + x].cpu().numpy()), x
        for n in ref.NAMES:
            if n.startswith("zdr") or n.startswith("kdp"):
                assert (_bits(got[n]) == 0).all(), n
        assert (got["rhohv"] == 1.0).all()


def test_absent_species_and_an_iiwarm_context(gpu_mixed, gpu_warm, consts):
    st = _state(64)
    with gpu_warm.pol_table() as t:
        rows = _get(t)
        got = _run(gpu_warm, t, st)
        none = _run(gpu_warm, t, {k: v for k, v in st.items() if k not in ("qs", "qg")})
    assert _same_all(got, none)
    want = ref.polarimetric(consts, 0.10, rows, st, warm=True)
    check_parity(got, want)
    for x in "sg":
        assert (_bits(got["kdp_" + x]) == 0).all() and (_bits(got["zdr_" + x]) == 0).all()
        assert (got["dbz_h_" + x] == got["dbz_h_" + x][0, 0]).all() and abs(got["dbz_h_" + x][0, 0] + 40.0) < 1e-9   # ze = 1.E-22
    assert _same(got["kdp"], got["kdp_r"])
    # only rain: Zh = (zh_r + 1.E-22) + 1.E-22, the closed form's floor of an absent species (see the module docstring)
    zh_r = 10.0 ** (got["dbz_h_r"] / 10.0 - 18.0)
    assert (np.abs(got["dbz_h"] - 10.0 * np.log10((zh_r + 2.0e-22) * 1e18)) * (math.log(10.0) / 10.0) <= 1e-12).all()
    rain = st["qr"] > 1e-12
    assert (np.abs(got["zdr"] - got["zdr_r"])[rain & (got["dbz_h_r"] > 0.0)] < 1e-3).all()
    # the same on the mixed-phase context with snow and graupel left out, and with them zero
    with gpu_mixed.pol_table() as t:
        a = _run(gpu_mixed, t, {k: v for k, v in st.items() if k not in ("qs", "qg")})
        b = _run(gpu_mixed, t, dict(st, qs=np.zeros_like(st["qs"]), qg=np.zeros_like(st["qg"])))
    assert _same_all(a, got) and _same_all(b, got)


def test_kw2_changes_nothing_and_the_wavelength_only_kdp(gpu_mixed, tables, main_set):
    from kid_amd import MieCfg
    st, _ = main_set
    base = _run(gpu_mixed, tables["default"][0], st)
    with gpu_mixed.pol_table(MieCfg(kw2=0.5)) as t:
        assert _same_all(_run(gpu_mixed, t, st), base)
    with gpu_mixed.pol_table(MieCfg(wavelength=0.05)) as t:
        half = _run(gpu_mixed, t, st)
        assert all(_same(t.get(x)[2], tables["default"][1][x][2]) for x in ref.SPECIES)
    for n in ref.NAMES:
        if n.startswith("kdp"):
            assert (np.abs(half[n] - 2.0 * base[n]) <= 2.0 * np.spacing(2.0 * base[n])).all(), n   # twice, within 2 ulp
        else:
            assert _same(half[n], base[n]), n
    assert (half["kdp"] > 0).any()


def test_bits_do_not_depend_on_batch_position_request_or_repeat(gpu_mixed, tables, main_set):
    import torch
    table = tables["default"][0]
    st, _ = main_set
    whole = _run(gpu_mixed, table, st)
    assert _same_all(_run(gpu_mixed, table, st), whole)                           # a repeated call
    for c in range(7):                                                            # each column alone
        one = _run(gpu_mixed, table, _take(st, slice(c, c + 1)))
        assert _same_all(one, {n: v[c:c + 1] for n, v in whole.items()}), c
    for c in (0, 6):                                                              # at every position of a batch of 7
        for pos in range(7):
            idx = np.array([(pos + 1 + i) % 7 for i in range(7)])
            idx[pos] = c
            got = _run(gpu_mixed, table, _take(st, idx))
            assert all(_same(got[n][pos], whole[n][c]) for n in ref.NAMES), (c, pos)
    dev = _dev(st)
    rng = np.random.Generator(np.random.PCG64(26))
    subsets = [(n,) for n in ref.NAMES] + [tuple(n for n in ref.NAMES if rng.uniform() < 0.4) for _ in range(8)]
    for names in subsets:                                                         # each output alone and random subsets
        if not names:
            continue
        out = {n: torch.full((7, 120), -7.0, dtype=torch.float64, device="cuda:0") for n in ref.NAMES}
        res = gpu_mixed.polarimetric(table, dev, want=names, out={n: out[n] for n in names})
        torch.cuda.synchronize()
        assert sorted(res) == sorted(names)
        for n in ref.NAMES:
            a = out[n].cpu().numpy()
            assert _same(a, whole[n]) if n in names else (a == -7.0).all(), (names, n)    # untouched buffers keep the sentinel
    rep = np.repeat(np.arange(7), 39)[:270]                                       # 270 columns: several workgroups
    got = _run(gpu_mixed, table, _take(st, rep))
    assert _same_all(got, {n: v[rep] for n, v in whole.items()})


def test_binary32_entries_round_once(gpu_mixed, tables, main_set):
    table = tables["default"][0]
    for st in [main_set[0]] + [_state(nz, 5) for nz in (2, 129, 256)]:             # two, then one, three and four level groups
        st32 = {k: v.astype(np.float32) for k, v in st.items()}
        got = _run(gpu_mixed, table, st32)
        ref64 = _run(gpu_mixed, table, {k: v.astype(np.float64) for k, v in st32.items()})
        for n in ref.NAMES:
            assert got[n].dtype == np.float32 and _same(got[n], ref64[n].astype(np.float32)), (st["t"].shape[1], n)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_entry_in_chunks_equals_the_device_entry(gpu_mixed, tables, main_set, dtype):
    m, table = gpu_mixed, tables["default"][0]
    st = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in main_set[0].items()}
    ncol = st["t"].shape[0]
    st17 = _take(st, np.arange(17) % ncol)
    want = _run(m, table, st17)
    for chunk in (5, 7):
        m.set_host_chunk(chunk)
        assert _same_all(m.polarimetric_host(table, st17, want=ref.NAMES), want), chunk
    some = ("rhohv", "kdp_s", "zdr")
    part = m.polarimetric_host(table, {k: v for k, v in st17.items() if k != "qg"}, want=some)
    no_g = _run(m, table, {k: v for k, v in st17.items() if k != "qg"}, want=some)
    assert sorted(part) == sorted(some) and _same_all(part, no_g)
    m.set_host_chunk(1)                                       # seven columns, one per chunk
    st7 = _take(st, np.arange(7) % ncol)
    assert _same_all(m.polarimetric_host(table, st7, want=ref.NAMES), _run(m, table, st7))


def test_hip_graph_replay_of_one_captured_launch(gpu_mixed, tables, main_set):
    import torch
    kp = _kp()
    m, L = gpu_mixed, kp.library()
    table = tables["default"][0]
    st, _ = main_set
    ncol, nz = st["t"].shape
    dev = _dev(st)
    names = ("zdr", "kdp_g", "rhohv", "dbz_h_r")
    out = {n: torch.full((ncol, nz), -7.0, dtype=torch.float64, device="cuda:0") for n in names}
    o = kp._PolOut(**{n: out[n].data_ptr() for n in names})
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = L.kidmp_polarimetric_device(m._h, table._t, ncol, nz, *[dev[k].data_ptr() for k in ref.INPUTS], C.byref(o),
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    eager = _run(m, table, st, want=names)
    for _ in range(2):
        for t in out.values():
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert all(_same(out[n].cpu().numpy(), eager[n]) for n in names)


def test_refusals_write_nothing(gpu_mixed, gpu_warm, tables, main_set):
    import torch
    from kid_amd import KidmpError, MieCfg, PolCfg
    kp = _kp()
    L = kp.library()
    table = tables["default"][0]
    st, _ = main_set
    ncol, nz = st["t"].shape
    dev = _dev(st)
    out = torch.full((ncol, nz), -7.0, dtype=torch.float64, device="cuda:0")
    host = torch.zeros(ncol * nz, dtype=torch.float64)

    def call(m=gpu_mixed, tab=table._t, ncol=ncol, nz=nz, names=("zdr",), **over):
        p = {k: v.data_ptr() for k, v in dev.items()}
        p.update(over)
        o = kp._PolOut(**{n: out.data_ptr() for n in names})
        return L.kidmp_polarimetric_device(m._h if m is not None else None, tab, ncol, nz, *[p[k] for k in ref.INPUTS], C.byref(o), None)

    with gpu_warm.pol_table() as other:
        refused = [dict(t=None), dict(p=None), dict(qv=None), dict(qr=None), dict(nr=None), dict(nz=1), dict(nz=257), dict(ncol=-1),
                   dict(names=()), dict(tab=None), dict(tab=other._t), dict(t=host.data_ptr()), dict(qg=host.data_ptr())]
        for kw in refused:
            assert call(**kw) == -1, kw
            assert L.kidmp_last_error(gpu_mixed._h), kw
    assert call(m=None) == -5 and call(ncol=0) == 0
    o = kp._PolOut(zdr=host.data_ptr())
    assert L.kidmp_polarimetric_device(gpu_mixed._h, table._t, ncol, nz, *[dev[k].data_ptr() for k in ref.INPUTS], C.byref(o), None) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all() and (host.numpy() == 0).all()
    nan = float("nan")
    for kw in (dict(axis_s=0.0), dict(axis_g=1.5), dict(axis_r_min=nan), dict(sigma=(0.1, -0.1, 0.1)), dict(axis_r=(1.0, nan, 0.0, 0.0, 0.0))):
        with pytest.raises(KidmpError, match="PolTable"):
            gpu_mixed.pol_table(None, PolCfg(**kw))
    with pytest.raises(KidmpError, match="PolTable"):
        gpu_mixed.pol_table(MieCfg(rho_i=0.0))
    h = C.c_void_p(1)
    bad = kp._PolCfg()
    L.kidmp_pol_defaults(C.byref(bad))
    bad.axis_g = 0.0
    assert L.kidmp_pol_table_create(gpu_mixed._h, None, C.byref(bad), None, C.byref(h)) == -1 and h.value is None
    assert call(qs=None, qg=None) == 0                           # and a good call works afterwards
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all()


# ---- 3. the physics, on hand-built rain columns ----
LAMS = (3000.0, 2500.0, 2000.0, 1750.0, 1500.0)                  # rain's slope 1/m, one per level
N0 = 8.0e6                                                       # Marshall-Palmer's intercept, 1/m**4


def _rain_columns(consts):
    """Two columns of len(LAMS) levels: rain alone with the slope LAMS[k] and the intercept N0 at level k."""
    nz = len(LAMS)
    shape = (2, nz)
    st = {k: np.zeros(shape) for k in ref.INPUTS}
    st["t"][:] = 285.0
    st["p"][:] = np.linspace(95000.0, 90000.0, nz)
    st["qv"][:] = 8.0e-3
    rho = ro.load(consts, st["qv"], st["qr"], st["nr"], st["qs"], st["qg"], st["t"], st["p"])["rho"]
    lam = np.broadcast_to(np.array(LAMS), shape)
    n = N0 / lam                                                 # mu_r = 0: N0_r = nr*lamr, lamr**3 = 6 am_r nr/rr
    st["nr"] = n / rho
    st["qr"] = (6.0 * ro.am_r * n / lam ** 3) / rho
    v = ro.load(consts, st["qv"], st["qr"], st["nr"], st["qs"], st["qg"], st["t"], st["p"])
    assert np.allclose(1.0 / v["ilamr"], lam, rtol=1e-12) and np.allclose(v["N0_r"], N0, rtol=1e-12)
    return st


def _fine_grid():
    """256 rain bins to 8 mm: the scheme's own end at 4.9 mm, short of the drops that carry zdr at lam = 1500 1/m."""
    dD = np.full(256, 8e-3 / 256)
    return {"r": (np.ascontiguousarray((np.arange(256) + 0.5) * dD), dD)}


def test_rain_at_no_canting(gpu_mixed, consts):
    from kid_amd import PolCfg
    st = _rain_columns(consts)
    with gpu_mixed.pol_table(None, PolCfg(sigma=(0.0, 0.0, 0.0)), _fine_grid()) as t:
        rows = _get(t)
        got = _run(gpu_mixed, t, st)
    check_parity(got, ref.polarimetric(consts, 0.10, rows, st))
    assert (got["zdr_r"] > 0).all() and (got["kdp_r"] > 0).all() and (got["rhohv"] < 1.0).all() and (got["rhohv"] > 0.97).all()
    assert (np.diff(got["zdr_r"], axis=1) > 0).all()             # rises as lamr falls at fixed N0_r
    print("zdr_r", got["zdr_r"][0], "kdp_r", got["kdp_r"][0], "rhohv", got["rhohv"][0])
    assert abs(got["zdr_r"][0, 0] - 0.95) < 0.005 and abs(got["zdr_r"][0, -1] - 2.7) < 0.05
    assert (np.diff(got["kdp_r"], axis=1) > 0).all() and _same(got["kdp"], got["kdp_r"])
    assert (np.abs(got["zdr"] - got["zdr_r"]) < 1e-4).all()      # nothing but rain's floor of 1.E-22 beside it


def test_rain_tumbling_at_random(gpu_mixed, consts):
    """sigma = 10 rad: q = exp(-200) is nothing beside 1, s_h and s_v are the same bits, zdr is 0 and kdp below 1e-80."""
    from kid_amd import PolCfg
    st = _rain_columns(consts)
    with gpu_mixed.pol_table(None, PolCfg(sigma=(10.0, 10.0, 10.0))) as t:
        rows = _get(t)
        got = _run(gpu_mixed, t, st)
    want = ref.polarimetric(consts, 0.10, rows, st)
    assert (_bits(want["zdr_r"]) == 0).all() and (_bits(want["zdr"]) == 0).all()
    assert (np.abs(got["zdr_r"]) * (math.log(10.0) / 10.0) <= bound("zdr")).all() and (np.abs(got["zdr"]) * (math.log(10.0) / 10.0) <= bound("zdr")).all()
    assert (got["kdp_r"] < 1e-80).all() and (got["kdp_r"] > 0).all() and (got["kdp"] < 1e-80).all()
    assert (got["rhohv"] <= 1.0).all() and (got["rhohv"] > 0.9).all()
    check_parity(got, want)


def test_zz_the_files_maxima(main_set):
    """Prints the largest differences from the restatement over the parity checks that ran before: what MEASURED records."""
    print("largest over the file", {k: "%.2e" % v for k, v in WORST.items()})
    for k, v in WORST.items():
        assert v <= bound(k), (k, v)
