"""The cloud radar on the MI355X (include/kidmp_mie.h, kidmp::k_mie_radar) against tests/mie_radar_ref.py, which takes the
library's own table through kidmp_mie_table_get and restates the load, the ascending-bin sums, the carriers and the scans
in the kernel's order.  Seven columns per state (tests/mie_radar_cases.py): five kinds of tests/bright_band_cases.py (mixed-phase with a melting level,
warm rain, cold snow and graupel without rain, every level below the top rainy and snowy and with graupel, snow alone at
the melting level) with cloud water added to the first, a dry column, and one column with every species at every level.

Exact: every equality between two device results (subsets, positions, repeats, the host entries, binary32 after one
rounding, graph replay, the NaN-filled surroundings); mie_x = 1.0 where the species is absent; dbz_up = dbz - pia_up as one
subtraction of the device's own two numbers; ze_x of kidmp_reflectivity_device at the long-wavelength limit up to the
derived bound.

Against the numpy restatement, per output, the bound is max(4 x measured, 64 ulp); MEASURED below holds the largest
difference in ulp over every shape, wavelength and grid of this file on the MI355X: mie_x, ext, pia_up, pia_down and
pia_total relative to the reference, dbz and dbz_x as the relative difference of the reflectivity they stand for
(|d dBZ| ln(10)/10), vd relative to |vd + w| + |w|:
    mie_x 15.9    dbz, dbz_x 29.5 (6.6e-15: two ulp of a dBZ near 50)    ext 6.9    pia_* 6.4    vd 6.7
so the bounds are 64 ulp for all but dbz, and 118 ulp for dbz.  The identities between device results are held at the
bound of pia_*, in ulp of pia_total: pia_up + pia_down - pia_total measured at most 2.4, the path a k_gas profile adds
against (20/ln 10) sum k_gas dz measured 0.6; ext with k_gas is the bits of ext without it plus k_gas.  Kernel and reference form the slopes by different routes (fastmath
pow and cube root against numpy's **), and an ulp of a slope is up to lam*D ulp of exp(-lam*D) in a bin; every output is
a ratio of two sums weighed by the same density, which cancels most of it.
"""
import ctypes as C

import numpy as np
import pytest

import bright_band_cases as bc
import doppler_ref as dref
import mie_radar_ref as ref
from mie_radar_cases import CFGS, state

pytestmark = pytest.mark.gpu

ULP = 2.220446049250313e-16
# the largest differences from the restatement measured on the MI355X, in ulp (see the module docstring)
MEASURED = {"mie": 15.9, "dbz": 29.5, "ext": 6.9, "pia": 6.4, "vd": 6.7}
NZS = (2, 63, 64, 65, 120, 129, 256)


def bound(kind):
    return max(4.0 * MEASURED[kind], 64.0) * ULP


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _dev(st, dtype=None):
    return {k: _cu(v if dtype is None else v.astype(dtype)) for k, v in st.items() if v is not None}


def _run(m, table, st, dz=None, w=None, k_gas=None, want=ref.NAMES, dtype=None):
    import torch
    opt = lambda a: None if a is None else _cu(a if dtype is None else a.astype(dtype))   # noqa: E731
    out = m.mie_radar(table, _dev(st, dtype), opt(dz), opt(w), opt(k_gas), want)
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


@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = dref.constants(o)
    o.close()
    return c


@pytest.fixture(scope="module")
def tables(gpu_mixed):
    """name -> (MieTable, the configuration, species -> (D, dD, rows) as the device holds them)."""
    from kid_amd import MieCfg
    out = {}
    for name, kw in CFGS.items():
        t = gpu_mixed.mie_table(MieCfg(**kw))
        out[name] = (t, ref.cfg_of(**kw), {x: t.get(x) for x in ref.SPECIES})
    yield out
    for t, _, _ in out.values():
        t.close()


@pytest.fixture(scope="module")
def main_set(consts, tables):
    st, dz, w, k_gas = state(120)
    _, cfg, rows = tables["w"]
    return st, dz, w, k_gas, ref.mie_radar(consts, cfg, rows, st, dz, w, k_gas)


@pytest.fixture(autouse=True)
def _leave_contexts_as_found(gpu_mixed, gpu_warm):
    yield
    for m in (gpu_mixed, gpu_warm):
        m.set_host_chunk(0)


def check_parity(got, want, w):
    """Every output against the restatement at the module's bounds; prints and returns the measured maxima in ulp."""
    worst = {"mie": 0.0, "dbz": 0.0, "ext": 0.0, "pia": 0.0, "vd": 0.0}
    rel = lambda a, b: float(np.max(np.abs(a - b) / np.where(b != 0, np.abs(b), 1.0)))   # noqa: E731
    for x in ref.SPECIES:
        worst["mie"] = max(worst["mie"], rel(got["mie_" + x], want["mie_" + x]))
        worst["dbz"] = max(worst["dbz"], float(np.max(np.abs(got["dbz_" + x] - want["dbz_" + x]))) * np.log(10.0) / 10.0)
    worst["dbz"] = max(worst["dbz"], float(np.max(np.abs(got["dbz"] - want["dbz"]))) * np.log(10.0) / 10.0)
    worst["ext"] = rel(got["ext"], want["ext"])
    for n in ("pia_up", "pia_down", "pia_total"):
        if n in got:
            worst["pia"] = max(worst["pia"], rel(got[n], want[n]))
    wind = 0.0 if w is None else w
    worst["vd"] = float(np.max(np.abs(got["vd"] - want["vd"]) / np.maximum(np.abs(want["vd"] + wind) + np.abs(wind), 1e-300)))
    print("measured ulp", {k: "%.1f" % (v / ULP) for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= bound(k), (k, v / ULP)
    return worst


def check_identities(got, st, k_gas_alone=None):
    """What holds exactly or by construction on any state."""
    for x, q, lim in (("r", "qr", 1e-12), ("s", "qs", 1e-6), ("g", "qg", 1e-6)):
        absent = ~(st[q] > lim)
        assert (got["mie_" + x][absent] == 1.0).all() and np.isfinite(got["mie_" + x]).all() and (got["mie_" + x] > 0).all(), x
    assert (got["ext"] >= 0).all() and np.isfinite(got["ext"]).all()
    assert _same(got["dbz_up"], got["dbz"] - got["pia_up"]) and _same(got["dbz_down"], got["dbz"] - got["pia_down"])
    tot = got["pia_total"][:, None]
    gap = np.abs(got["pia_up"] + got["pia_down"] - tot) / np.maximum(tot, 1e-300)
    print("pia_up + pia_down - pia_total, ulp of the total: %.1f" % (float(gap.max()) / ULP))
    assert (gap <= bound("pia")).all()
    assert (got["pia_up"] >= 0).all() and (got["pia_down"] >= 0).all()
    no_echo = ~((st["qr"] > 1e-12) | (st["qs"] > 1e-6) | (st["qg"] > 1e-6))
    assert (_bits(got["vd"])[no_echo] == 0).all()


# ---- 1. shapes, wavelengths, cases ----
@pytest.mark.parametrize("name", sorted(CFGS))
@pytest.mark.parametrize("nz", NZS)
def test_shapes_against_the_restatement(gpu_mixed, consts, tables, nz, name):
    table, cfg, rows = tables[name]
    st, dz, w, k_gas = state(nz)
    want = ref.mie_radar(consts, cfg, rows, st, dz, w, k_gas)
    got = _run(gpu_mixed, table, st, dz, w, k_gas)
    assert sorted(got) == sorted(ref.NAMES) and got["pia_total"].shape == (7,)
    check_parity(got, want, w)
    check_identities(got, st)
    # Mie matters at these wavelengths: rain's ratio leaves 1 by more than a tenth somewhere
    assert (np.abs(got["mie_r"][st["qr"] > 1e-12] - 1.0) > 0.1).any()


def test_the_dry_column_and_the_gas_path(gpu_mixed, consts, tables, main_set):
    table, cfg, rows = tables["w"]
    st, dz, w, k_gas, want = main_set
    got = _run(gpu_mixed, table, st, dz, w, k_gas)
    dry = 5
    for x in ref.SPECIES:
        assert (got["mie_" + x][dry] == 1.0).all()
    assert _same(got["ext"][dry], k_gas) and (_bits(got["vd"][dry]) == 0).all()
    assert (got["dbz"][dry] == got["dbz"][dry, 0]).all() and abs(got["dbz"][dry, 0] - 10.0 * np.log10(3e-22 * 1e18)) < 1e-9
    only_gas = ref.PIA * float(np.sum(k_gas * dz))
    assert abs(got["pia_total"][dry] / only_gas - 1.0) <= bound("pia")
    # a k_gas profile adds its own path: with and without it, per column
    bare = _run(gpu_mixed, table, st, dz, w, None, want=("pia_total", "ext", "pia_up"))
    assert (_bits(bare["ext"][dry]) == 0).all() and bare["pia_total"][dry] == 0.0 and (bare["pia_up"][dry] == 0).all()
    assert _same(got["ext"], bare["ext"] + k_gas[None, :])                        # one addition in the kernel: exact
    added = got["pia_total"] - bare["pia_total"]
    print("k_gas path, ulp of the total: %.1f" % (float(np.max(np.abs(added - only_gas) / got["pia_total"])) / ULP))
    assert (np.abs(added - only_gas) <= bound("pia") * got["pia_total"]).all()
    # per-column k_gas [ncol, nz] gives the bits of the shared profile
    full = _run(gpu_mixed, table, st, np.tile(dz, (7, 1)), w, np.tile(k_gas, (7, 1)))
    assert _same_all(full, got)


@pytest.mark.parametrize("which", ["illustrative", "defaults"])
def test_long_wavelength_limit_is_the_reflectivity(gpu_mixed, consts, main_set, which):
    """A table at 100 m: dbz differs from kidmp_reflectivity_device's by at most 10 log10(1 + delta) plus rounding, delta the
    largest |s_mie/s_ray - 1| of that table.  Derived, not measured.  With the illustrative W-band permittivities delta is
    0.196 (|K|**2/kw2 and rho_i differ from the scheme's constants: 0.78 dB); with the default configuration only rain's
    |K_w|**2/kw2 - 1 = 0.0042 is left (0.018 dB), which an error of a few per cent in any species' ratio would break."""
    import torch
    from kid_amd import MieCfg
    st = main_set[0]
    kw = dict(CFGS["w"], wavelength=100.0) if which == "illustrative" else dict(wavelength=100.0)
    with gpu_mixed.mie_table(MieCfg(**kw)) as t:
        rows = {x: t.get(x) for x in ref.SPECIES}
        got = _run(gpu_mixed, t, st, want=("dbz", "mie_r", "mie_s", "mie_g"))
    delta = ref.rayleigh_gap(rows)
    print("delta", delta)
    assert 0.1 < delta < 0.3 if which == "illustrative" else 0.004 < delta < 0.0045
    plain = gpu_mixed.reflectivity(_dev({k: st[k] for k in bc.INPUTS}))
    torch.cuda.synchronize()
    plain = plain.cpu().numpy()
    assert (np.abs(got["dbz"] - plain) <= 10.0 * np.log10(1.0 + delta) + bound("dbz") * 10.0 / np.log(10.0)).all()
    for x in ref.SPECIES:
        assert (np.abs(got["mie_" + x] - 1.0) <= delta * (1.0 + bound("mie"))).all(), x


def test_scheme_wavelength_with_scheme_constants_returns_the_reflectivity(gpu_mixed, main_set):
    """At the defaults' 10 cm with snow and graupel (|K_i|**2 = 0.176, rho_i = 900: s_mie -> s_ray in the Rayleigh limit) the
    ratios of snow and graupel stay within the Mie correction of their largest particles; rain's |K_w|**2/kw2 = 1.004."""
    st = main_set[0]
    with gpu_mixed.mie_table() as t:
        got = _run(gpu_mixed, t, st, want=("mie_r", "mie_s", "mie_g"))
    assert (np.abs(got["mie_r"] - 1.0) < 0.15).all() and (np.abs(got["mie_s"] - 1.0) < 0.5).all()


# ---- 2. memory and bits ----
def test_bits_do_not_depend_on_batch_position_request_or_repeat(gpu_mixed, tables, main_set):
    table = tables["w"][0]
    st, dz, w, k_gas, _ = main_set
    whole = _run(gpu_mixed, table, st, dz, w, k_gas)
    assert _same_all(_run(gpu_mixed, table, st, dz, w, k_gas), whole)             # a repeated call
    for c in range(7):                                                            # each column alone
        one = _run(gpu_mixed, table, _take(st, slice(c, c + 1)), dz, w[c:c + 1], k_gas)
        assert _same_all(one, {n: v[c:c + 1] for n, v in whole.items()}), c
    for c in (0, 6):                                                              # at every position of a batch of 7
        for pos in range(7):
            idx = np.array([(pos + 1 + i) % 7 for i in range(7)])
            idx[pos] = c
            got = _run(gpu_mixed, table, _take(st, idx), dz, w[idx], k_gas)
            assert all(_same(got[n][pos], whole[n][c]) for n in ref.NAMES), (c, pos)
    for n in ref.NAMES:                                                           # each output alone
        alone = _run(gpu_mixed, table, st, dz, w, k_gas, want=(n,))
        assert sorted(alone) == [n] and _same(alone[n], whole[n]), n
    rep = np.repeat(np.arange(7), 40)                                             # 280 columns: several workgroups
    got = _run(gpu_mixed, table, _take(st, rep), dz, w[rep], k_gas)
    assert _same_all(got, {n: v[rep] for n, v in whole.items()})


def test_the_middle_of_a_nan_filled_tensor(gpu_mixed, tables, main_set):
    """Inputs and outputs are the middle thirds of NaN-filled allocations: the result is the usual one and both guards of
    every output stay NaN."""
    import torch
    from kid_amd.mie import _MieOut, library
    m, L = gpu_mixed, library()
    table = tables["w"][0]
    st, dz, w, k_gas, _ = main_set
    ncol, nz = st["t"].shape
    whole = _run(m, table, st, dz, w, k_gas)

    def middle(a):
        buf = torch.full((3 * a.size,), float("nan"), dtype=torch.float64, device="cuda:0")
        buf[a.size:2 * a.size] = _cu(a.reshape(-1))
        return buf
    ins = {k: middle(st[k]) for k in ref.INPUTS}
    extra = {"dz": middle(dz), "w": middle(w), "k_gas": middle(k_gas)}
    outs = {n: torch.full((3 * (ncol if n == "pia_total" else ncol * nz),), float("nan"), dtype=torch.float64, device="cuda:0") for n in ref.NAMES}
    mid = lambda t: t.data_ptr() + 8 * (t.numel() // 3)   # noqa: E731
    o = _MieOut(**{n: mid(t) for n, t in outs.items()})
    rc = L.kidmp_mie_radar_device(m._h, table._t, ncol, nz, *[mid(ins[k]) for k in ref.INPUTS], mid(extra["dz"]), 0, mid(extra["w"]),
                                  mid(extra["k_gas"]), 0, C.byref(o), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for n, t in outs.items():
        a = t.cpu().numpy()
        k = a.size // 3
        assert np.isnan(a[:k]).all() and np.isnan(a[2 * k:]).all(), n
        assert _same(a[k:2 * k].reshape(whole[n].shape), whole[n]), n


# ---- 3. the other entries ----
def test_binary32_entries_round_once(gpu_mixed, tables, main_set):
    table = tables["w"][0]
    f = lambda a: a.astype(np.float32)   # noqa: E731
    for st, dz, w, k_gas in [main_set[:4]] + [state(nz) for nz in (2, 129, 256)]:     # two, then one, three and four level groups
        st32 = {k: f(v) for k, v in st.items()}
        got = _run(gpu_mixed, table, st32, f(dz), f(w), f(k_gas))
        ref64 = _run(gpu_mixed, table, {k: v.astype(np.float64) for k, v in st32.items()}, f(dz).astype(np.float64), f(w).astype(np.float64),
                     f(k_gas).astype(np.float64))
        for n in ref.NAMES:
            assert got[n].dtype == np.float32 and _same(got[n], ref64[n].astype(np.float32)), (st["t"].shape[1], n)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_entry_in_chunks_equals_the_device_entry(gpu_mixed, tables, main_set, dtype, monkeypatch):
    from padded_rows import with_padded
    from kid_amd.mie import library
    m, table = gpu_mixed, tables["ka"][0]
    st, dz, w, k_gas, _ = main_set
    st5 = {k: np.ascontiguousarray(v[:5].astype(dtype)) for k, v in st.items()}
    dz_, w_, kg_ = dz.astype(dtype), np.ascontiguousarray(w[:5].astype(dtype)), k_gas.astype(dtype)
    want = _run(m, table, st5, dz_, w_, kg_)
    m.set_host_chunk(2)
    assert _same_all(m.mie_radar_host(table, st5, dz_, w_, kg_, want=ref.NAMES), want)
    some = ("pia_total", "mie_s", "dbz_down")
    part = m.mie_radar_host(table, st5, dz_, None, kg_, want=some)
    assert sorted(part) == sorted(some) and all(_same(part[n], want[n]) for n in some)
    per_col = m.mie_radar_host(table, st5, np.ascontiguousarray(np.tile(dz_, (5, 1))), w_, np.ascontiguousarray(np.tile(kg_, (5, 1))), want=ref.NAMES)
    assert _same_all(per_col, want)
    # seven columns with a dz and a k_gas of their own: one per chunk, then in chunks of 3, 3 and 1 with the rows of dz and
    # k_gas nz + 5 apart (dz_col_stride, k_gas_col_stride)
    idx = np.arange(7) % st["t"].shape[0]
    st7 = {k: np.ascontiguousarray(v[idx].astype(dtype)) for k, v in st.items()}
    scale = np.linspace(0.5, 2.0, 7)[:, None]
    dz7, w7, kg7 = np.ascontiguousarray((dz * scale).astype(dtype)), np.ascontiguousarray(w[idx].astype(dtype)), np.ascontiguousarray((k_gas / scale).astype(dtype))
    want7 = _run(m, table, st7, dz7, w7, kg7)
    m.set_host_chunk(1)
    assert _same_all(m.mie_radar_host(table, st7, dz7, w7, kg7, want=ref.NAMES), want7)
    m.set_host_chunk(3)
    seen = with_padded(monkeypatch, library(), "kidmp_mie_radar_host" if dtype == np.float64 else "kidmp32_mie_radar_host", {12: dz7, 15: kg7})
    assert _same_all(m.mie_radar_host(table, st7, dz7, w7, kg7, want=ref.NAMES), want7) and seen == [(12, 125), (15, 125)]


def test_hip_graph_replay_of_one_captured_launch(gpu_mixed, tables, main_set):
    import torch
    from kid_amd.mie import _MieOut, library
    m, L = gpu_mixed, library()
    table = tables["w"][0]
    st, dz, w, k_gas, _ = main_set
    ncol, nz = st["t"].shape
    dev = _dev(st)
    ddz, dw, dkg = _cu(dz), _cu(w), _cu(k_gas)
    names = ("dbz_up", "mie_g", "vd", "pia_total")
    out = {n: torch.full((ncol,) if n == "pia_total" else (ncol, nz), -7.0, dtype=torch.float64, device="cuda:0") for n in names}
    o = _MieOut(**{n: out[n].data_ptr() for n in names})
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = L.kidmp_mie_radar_device(m._h, table._t, ncol, nz, *[dev[k].data_ptr() for k in ref.INPUTS], ddz.data_ptr(), 0, dw.data_ptr(),
                                      dkg.data_ptr(), 0, C.byref(o), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    eager = _run(m, table, st, dz, w, k_gas, want=names)
    for _ in range(2):
        for t in out.values():
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert all(_same(out[n].cpu().numpy(), eager[n]) for n in names)


@pytest.mark.parametrize("nb", [1, 65, 256])
def test_the_callers_grids(gpu_mixed, consts, nb):
    from kid_amd import MieCfg
    st, dz, w, k_gas = state(65)
    edges = {"r": (5e-5, 6e-3), "s": (2e-4, 2e-2), "g": (2.5e-4, 4e-2)}
    grids = {}
    for x, (lo, hi) in edges.items():
        e = np.exp(np.linspace(np.log(lo), np.log(hi), nb + 1))
        grids[x] = (np.ascontiguousarray(np.sqrt(e[:-1] * e[1:])), np.ascontiguousarray(e[1:] - e[:-1]))
    with gpu_mixed.mie_table(MieCfg(**CFGS["w"]), grids) as t:
        rows = {x: t.get(x) for x in ref.SPECIES}
        for x in ref.SPECIES:
            assert rows[x][2].shape == (5, nb) and _same(rows[x][0], grids[x][0]) and _same(rows[x][1], grids[x][1])
        got = _run(gpu_mixed, t, st, dz, w, k_gas)
    want = ref.mie_radar(consts, ref.cfg_of(**CFGS["w"]), rows, st, dz, w, k_gas)
    check_parity(got, want, w)
    check_identities(got, st)


def test_an_iiwarm_context_has_no_snow_or_graupel(gpu_warm, consts):
    from kid_amd import MieCfg
    st, dz, w, k_gas = state(64)
    with gpu_warm.mie_table(MieCfg(**CFGS["ka"])) as t:
        rows = {x: t.get(x) for x in ref.SPECIES}
        got = _run(gpu_warm, t, st, dz, w, k_gas)
        none = _run(gpu_warm, t, {k: v for k, v in st.items() if k not in ("qs", "qg")}, dz, w, k_gas)
    assert _same_all(got, none)
    assert (got["mie_s"] == 1.0).all() and (got["mie_g"] == 1.0).all()
    want = ref.mie_radar(consts, ref.cfg_of(**CFGS["ka"]), rows, st, dz, w, k_gas, warm=True)
    check_parity(got, want, w)


def test_the_table_is_the_host_entrys(gpu_mixed, tables):
    """kidmp_mie_table_get returns what kidmp_mie_bins forms on the scheme's own bins, bit for bit."""
    from kid_amd import MieCfg, default_grid, mie_bins
    for name, (t, _, rows) in tables.items():
        for x in ref.SPECIES:
            D, dD = default_grid(gpu_mixed, x)
            assert _same(rows[x][0], np.asarray(D)) and _same(rows[x][1], np.asarray(dD))
            assert _same(rows[x][2], mie_bins(MieCfg(**CFGS[name]), x, rows[x][0])), (name, x)


def test_refusals_write_nothing(gpu_mixed, gpu_warm, tables, main_set):
    import torch
    from kid_amd.mie import _MieOut, library
    L = library()
    table = tables["w"][0]
    st, dz, w, k_gas, _ = main_set
    ncol, nz = st["t"].shape
    dev = _dev(st)
    ddz = _cu(dz)
    out = torch.full((ncol, nz), -7.0, dtype=torch.float64, device="cuda:0")
    host = torch.zeros(ncol * nz, dtype=torch.float64)

    def call(m=gpu_mixed, tab=table._t, ncol=ncol, nz=nz, dz=ddz.data_ptr(), stride=0, kstride=0, names=("dbz_up",), **over):
        p = {k: v.data_ptr() for k, v in dev.items()}
        p.update(over)
        o = _MieOut(**{n: out.data_ptr() for n in names})
        return L.kidmp_mie_radar_device(m._h if m is not None else None, tab, ncol, nz, *[p[k] for k in ref.INPUTS], dz, stride, None, None,
                                        kstride, C.byref(o), None)

    with gpu_warm.mie_table() as other:
        refused = [dict(t=None), dict(p=None), dict(qv=None), dict(qr=None), dict(nr=None), dict(nz=1), dict(nz=257), dict(ncol=-1),
                   dict(names=()), dict(dz=None), dict(stride=nz - 1), dict(kstride=1), dict(tab=None), dict(tab=other._t),
                   dict(t=host.data_ptr()), dict(qc=host.data_ptr()), dict(dz=host.data_ptr())]
        for kw in refused:
            assert call(**kw) == -1, kw
            assert L.kidmp_last_error(gpu_mixed._h), kw
    assert call(m=None) == -5 and call(ncol=0) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()
    assert call(qc=None, qs=None, qg=None) == 0 and call(dz=None, names=("dbz",)) == 0
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all()
