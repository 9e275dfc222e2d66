"""The microwave radiometer on the MI355X (include/kidmp_radiometer.h, kidmp::k_radiometer) against tests/radiometer_ref.py,
which takes the library's own table through kidmp_radiometer_table_get and restates the load, the ascending-bin sums, the
carriers, the layers, the two scans in the kernel's Kogge-Stone and carry order and the closure.  Seven columns per state
(tests/radiometer_cases.py): five of tests/mie_radar_cases.py and two whose levels hold, in turn, nothing, snow alone, rain
alone, cloud water alone and graupel alone.  Two tables: an absorbing one (illustrative W-band permittivities, run with a
gas profile) and the default one (10 cm, Im(eps_i) = 0, run without), so that the conservative branch (ta == 0 < b), the
non-scattering branch (b == 0 < ta) and the identity (ta == b == 0) are all taken; the test counts them.

Exact: every equality between two device results (subsets, positions, repeats, the host entries, binary32 after one
rounding, graph replay, the NaN-filled surroundings); tb_toa and tb_ground as the bits of tb_up[nz-1] and tb_down[0]; the
transparent column.

Against the numpy restatement, per output, the bound is max(4 x measured, 64 ulp) in ulp of the value (tau_abs: of
tau_abs); MEASURED below holds the largest difference over every shape, table and grid of this file on the MI355X:
    k_abs, k_bsc 26    refl, trans 28    tb_up, tb_down, tb_toa, tb_ground 23    tau_abs 6
so every bound is 4 x measured: 104, 112 and 92 ulp, and 64 ulp for tau_abs.  None comes near 1e4 ulp.
Kernel and reference form the slopes and the exponentials by different routes (fastmath against numpy), and an ulp of a
slope is up to lam*D ulp of exp(-lam*D) in a bin; k_abs and k_bsc are ratios of two sums weighed by the same density, which
cancels most of it.  The closure's denominators 1 - Rt* Rb_S stay above 0.86 on these columns: nothing is near-singular.
The identities between device results are held at the bound of tb_*: equilibrium measured 29 ulp of T0, the
non-scattering column against the Schwarzschild sum of numpy's cumsum 3 ulp (optical paths up to 2.7).
"""
import ctypes as C

import numpy as np
import pytest

import doppler_ref as dref
import radiometer_cases as rc
import radiometer_ref as ref

pytestmark = pytest.mark.gpu

ULP = 2.220446049250313e-16
# the largest differences from the restatement measured on the MI355X, in ulp (see the module docstring)
MEASURED = {"k": 26.0, "layer": 28.0, "tb": 23.0, "tau": 6.0}
KIND = {"k_abs": "k", "k_bsc": "k", "refl": "layer", "trans": "layer", "tb_up": "tb", "tb_down": "tb", "tb_toa": "tb", "tb_ground": "tb",
        "tau_abs": "tau"}
T0 = 273.15


def bound(kind):
    return max(4.0 * MEASURED[kind], 64.0)


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _dev(st, dtype=None):
    return {k: _cu(v if dtype is None else v.astype(dtype)) for k, v in st.items() if v is not None}


def _rcfg(kw):
    from kid_amd import RadiometerCfg
    return None if kw is None else RadiometerCfg(**kw)


def _run(m, table, st, dz=None, k_gas=None, t_sfc=None, rcfg=rc.RCFG, want=ref.NAMES, dtype=None):
    import torch
    opt = lambda a: None if a is None else _cu(a if dtype is None else a.astype(dtype))   # noqa: E731
    out = m.radiometer(table, _dev(st, dtype), opt(dz), opt(k_gas), opt(t_sfc), _rcfg(rcfg), want)
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
    """name -> (RadiometerTable, the configuration, species -> (D, dD, rows) as the device holds them)."""
    from kid_amd import MieCfg
    out = {}
    for name, kw in rc.TABLES.items():
        t = gpu_mixed.radiometer_table(MieCfg(**kw))
        out[name] = (t, rc.cfg_of(name), {x: t.get(x) for x in ref.SPECIES})
    yield out
    for t, _, _ in out.values():
        t.close()


@pytest.fixture(scope="module")
def main_set(consts, tables):
    """The absorbing table at 129 levels: three level groups, the last one level long."""
    st, dz, k_gas, t_sfc = rc.state(129)
    _, cfg, rows = tables["absorbing"]
    return st, dz, k_gas, t_sfc, ref.radiometer(consts, cfg, rows, st, dz, k_gas, t_sfc, **rc.RCFG)


@pytest.fixture(autouse=True)
def _leave_contexts_as_found(gpu_mixed, gpu_warm):
    yield
    for m in (gpu_mixed, gpu_warm):
        m.set_host_chunk(0)


def check_parity(got, want):
    """Every output against the restatement at the module's bounds; prints and returns the measured maxima in ulp."""
    worst = {k: 0.0 for k in MEASURED}
    where = {}
    for n in ref.NAMES:
        if n not in got:
            continue
        u = ref.ulps(got[n], want[n])
        assert np.isfinite(got[n]).all(), n
        w = float(np.max(u))
        if w >= worst[KIND[n]]:
            worst[KIND[n]], where[KIND[n]] = w, (n,) + tuple(int(i) for i in np.unravel_index(int(np.argmax(u)), u.shape))
    print("measured ulp", {k: "%.1f" % v for k, v in worst.items()}, where,
          "smallest closure denominator %.4f" % min(float(want["d_up"].min()), float(want["d_down"].min())))
    for k, v in worst.items():
        assert v <= bound(k), (k, v, where.get(k))
    return worst


def check_identities(got):
    """What holds exactly or by construction on any state."""
    assert _same(got["tb_toa"], got["tb_up"][:, -1]) and _same(got["tb_ground"], got["tb_down"][:, 0])
    for n in ("k_abs", "k_bsc", "refl", "trans", "tau_abs"):
        assert (got[n] >= 0).all(), n
    assert (got["refl"] + got["trans"] <= 1.0 + 4 * ULP).all() and (got["trans"] <= 1.0).all()
    assert (got["tb_up"] > 0).all() and (got["tb_down"] > 0).all()


# ---- 1. shapes, tables, cases ----
@pytest.mark.parametrize("name", sorted(rc.TABLES))
@pytest.mark.parametrize("nz", rc.NZS)
def test_shapes_against_the_restatement(gpu_mixed, consts, tables, nz, name):
    table, cfg, rows = tables[name]
    st, dz, k_gas, t_sfc = rc.state(nz)
    kg = k_gas if rc.USES_GAS[name] else None
    want = ref.radiometer(consts, cfg, rows, st, dz, kg, t_sfc, **rc.RCFG)
    got = _run(gpu_mixed, table, st, dz, kg, t_sfc)
    assert sorted(got) == sorted(ref.NAMES) and all(got[n].shape == (7,) for n in ref.SUMMARY)
    # the branches of the layer that this table can take are taken, on the device's own coefficients
    dzf = np.broadcast_to(dz, got["k_abs"].shape)
    conservative, non_scattering, identity = rc.branches(got["k_abs"] * dzf, got["k_bsc"] * dzf)
    print("levels: conservative %d, non-scattering %d, identity %d" % (conservative, non_scattering, identity))
    assert (conservative, non_scattering, identity) == rc.branches(want["ta"], want["b"])
    assert non_scattering > 0 and (name == "absorbing" or (conservative > 0 and identity > 0))
    assert (st["qg"] > 1e-6).any() and (got["k_bsc"][st["qg"] > 1e-6] > 0).all()
    check_parity(got, want)
    check_identities(got)


@pytest.mark.parametrize("nb", [1, 65, 256])
def test_the_callers_grids(gpu_mixed, consts, nb):
    from kid_amd import MieCfg
    st, dz, k_gas, t_sfc = rc.state(65)
    edges = {"r": (5e-5, 6e-3), "s": (2e-4, 2e-2), "g": (2.5e-4, 4e-2)}
    grids = {}
    for x, (lo, hi) in edges.items():
        e = np.exp(np.linspace(np.log(lo), np.log(hi), nb + 1))
        grids[x] = (np.ascontiguousarray(np.sqrt(e[:-1] * e[1:])), np.ascontiguousarray(e[1:] - e[:-1]))
    for name in sorted(rc.TABLES):
        kg = k_gas if rc.USES_GAS[name] else None
        with gpu_mixed.radiometer_table(MieCfg(**rc.TABLES[name]), grids) as t:
            rows = {x: t.get(x) for x in ref.SPECIES}
            for x in ref.SPECIES:
                assert rows[x][2].shape == (3, nb) and _same(rows[x][0], grids[x][0]) and _same(rows[x][1], grids[x][1])
            got = _run(gpu_mixed, t, st, dz, kg, t_sfc)
        check_parity(got, ref.radiometer(consts, rc.cfg_of(name), rows, st, dz, kg, t_sfc, **rc.RCFG))
        check_identities(got)


# ---- 2. identities between device results ----
@pytest.mark.parametrize("name", sorted(rc.TABLES))
def test_equilibrium(gpu_mixed, tables, name):
    """Everything at T0 -- the levels, the surface, the sky: any emissivity, any hydrometeors, and every face shows T0."""
    st, dz, k_gas, _ = rc.state(129)
    st = dict(st, t=np.full_like(st["t"], T0))
    worst = 0.0
    for em in (1.0, 0.6, 0.0):
        got = _run(gpu_mixed, tables[name][0], st, dz, k_gas if rc.USES_GAS[name] else None, np.full(7, T0),
                   dict(mu=0.6, emissivity=em, t_cosmic=T0), want=("tb_up", "tb_down"))
        worst = max(worst, float(np.max(ref.ulps(got["tb_up"], T0))), float(np.max(ref.ulps(got["tb_down"], T0))))
    print("equilibrium, ulp of T0: %.1f" % worst)
    assert worst <= bound("tb")


def test_transparent_column(gpu_mixed, tables):
    """No hydrometeors and no gas: the sky below, the surface and the reflected sky above, to the bit."""
    st, dz, _, t_sfc = rc.state(65)
    for k in ("qc", "qr", "nr", "qs", "qg"):
        st[k][:] = 0.0
    em, tc = 0.85, 2.725
    got = _run(gpu_mixed, tables["default"][0], st, dz, None, t_sfc, dict(mu=0.6, emissivity=em, t_cosmic=tc))
    assert (got["tb_down"] == tc).all() and (got["tb_ground"] == tc).all()
    up = em * t_sfc + (1.0 - em) * tc
    assert _same(got["tb_up"], np.ascontiguousarray(np.broadcast_to(up[:, None], got["tb_up"].shape))) and _same(got["tb_toa"], up)
    assert (_bits(got["refl"]) == 0).all() and (got["trans"] == 1.0).all() and (_bits(got["tau_abs"]) == 0).all()
    assert (_bits(got["k_abs"]) == 0).all() and (_bits(got["k_bsc"]) == 0).all()
    # t_sfc left out: the column's t at level 0
    none = _run(gpu_mixed, tables["default"][0], st, dz, None, None, dict(mu=0.6, emissivity=em, t_cosmic=tc), want=("tb_toa",))
    assert _same(none["tb_toa"], em * st["t"][:, 0] + (1.0 - em) * tc)


def test_non_scattering_column_is_schwarzschild(gpu_mixed, tables):
    """Cloud water and gas alone: tb_ground and tb_toa are the Schwarzschild sums, formed here with numpy's cumsum; more
    cloud water warms the ground radiometer's view of a cold sky."""
    st, dz, k_gas, t_sfc = rc.state(65)
    rng = np.random.Generator(np.random.PCG64(3))
    for k in ("qr", "nr", "qs", "qg"):
        st[k][:] = 0.0
    st["qc"] = np.where(rng.uniform(size=st["qc"].shape) < 0.6, 4.0e-4 * rng.uniform(0.2, 2.0, st["qc"].shape), 0.0)
    mu, em, tc = 0.6, 0.85, 2.725
    cfg = dict(mu=mu, emissivity=em, t_cosmic=tc)
    got = _run(gpu_mixed, tables["absorbing"][0], st, dz, k_gas, t_sfc, cfg)
    assert (_bits(got["k_bsc"]) == 0).all() and (_bits(got["refl"]) == 0).all() and (got["k_abs"] > 0).all()
    tau = got["k_abs"] * dz / mu
    a = -np.expm1(-tau)
    below = np.cumsum(tau, axis=1) - tau                                  # the optical path between the ground and level k
    above = np.cumsum(tau[:, ::-1], axis=1)[:, ::-1] - tau                # between level k and space
    total = np.sum(tau, axis=1)
    ground = np.sum(a * st["t"] * np.exp(-below), axis=1) + tc * np.exp(-total)
    toa = np.sum(a * st["t"] * np.exp(-above), axis=1) + (em * t_sfc + (1.0 - em) * ground) * np.exp(-total)
    worst = max(float(np.max(ref.ulps(got["tb_ground"], ground))), float(np.max(ref.ulps(got["tb_toa"], toa))))
    print("Schwarzschild sum by cumsum, ulp: %.1f (tau up to %.2f)" % (worst, float(total.max())))
    assert worst <= bound("tb")
    more = _run(gpu_mixed, tables["absorbing"][0], dict(st, qc=2.0 * st["qc"]), dz, k_gas, t_sfc, cfg, want=("tb_ground",))
    assert (more["tb_ground"] > got["tb_ground"]).all()


def test_scattering_over_an_emitting_surface(gpu_mixed, tables):
    """Snow alone aloft, Im(eps_i) = 0, a black surface: the snow emits nothing and scatters the surface's emission back
    down, so tb_toa falls below ts, and further as qs doubles."""
    st, dz, _, t_sfc = rc.state(65)
    for k in ("qc", "qr", "nr", "qg"):
        st[k][:] = 0.0
    st["t"][:] = np.linspace(268.0, 230.0, 65)
    st["qs"][:] = 0.0
    st["qs"][:, 30:50] = np.linspace(2.0e-4, 1.0e-3, 7)[:, None]
    cfg = dict(mu=0.6, emissivity=1.0, t_cosmic=2.725)
    one = _run(gpu_mixed, tables["default"][0], st, dz, None, t_sfc, cfg, want=("tb_toa", "k_abs", "k_bsc"))
    two = _run(gpu_mixed, tables["default"][0], dict(st, qs=2.0 * st["qs"]), dz, None, t_sfc, cfg, want=("tb_toa",))
    assert (_bits(one["k_abs"]) == 0).all() and (one["k_bsc"][:, 30:50] > 0).all()
    print("ts - tb_toa, K:", t_sfc - one["tb_toa"], t_sfc - two["tb_toa"])
    assert (one["tb_toa"] < t_sfc).all() and (two["tb_toa"] < one["tb_toa"]).all()


# ---- 3. memory and bits ----
def test_bits_do_not_depend_on_batch_position_request_or_repeat(gpu_mixed, tables, main_set):
    table = tables["absorbing"][0]
    st, dz, k_gas, t_sfc, _ = main_set
    whole = _run(gpu_mixed, table, st, dz, k_gas, t_sfc)
    assert _same_all(_run(gpu_mixed, table, st, dz, k_gas, t_sfc), whole)         # a repeated call
    for c in range(7):                                                            # each column alone
        one = _run(gpu_mixed, table, _take(st, slice(c, c + 1)), dz, k_gas, t_sfc[c:c + 1])
        assert _same_all(one, {n: v[c:c + 1] for n, v in whole.items()}), c
    for c in (0, 6):                                                              # at every position of a batch of 7
        for pos in range(7):
            idx = np.array([(pos + 1 + i) % 7 for i in range(7)])
            idx[pos] = c
            got = _run(gpu_mixed, table, _take(st, idx), dz, k_gas, np.ascontiguousarray(t_sfc[idx]))
            assert all(_same(got[n][pos], whole[n][c]) for n in ref.NAMES), (c, pos)
    for n in ref.NAMES:                                                           # each output alone
        alone = _run(gpu_mixed, table, st, dz, k_gas, t_sfc, want=(n,))
        assert sorted(alone) == [n] and _same(alone[n], whole[n]), n
    no_dz = _run(gpu_mixed, table, st, None, k_gas, t_sfc, want=("k_abs", "k_bsc"))   # the optics need no dz
    assert _same(no_dz["k_abs"], whole["k_abs"]) and _same(no_dz["k_bsc"], whole["k_bsc"])
    rep = np.repeat(np.arange(7), 40)                                             # 280 columns: several workgroups
    got = _run(gpu_mixed, table, _take(st, rep), dz, k_gas, np.ascontiguousarray(t_sfc[rep]))
    assert _same_all(got, {n: v[rep] for n, v in whole.items()})
    full = _run(gpu_mixed, table, st, np.tile(dz, (7, 1)), np.tile(k_gas, (7, 1)), t_sfc)   # per-column dz and k_gas
    assert _same_all(full, whole)


def _out_shape(n, ncol, nz):
    return (ncol,) if n in ref.SUMMARY else (ncol, nz)


def test_the_middle_of_a_nan_filled_tensor(gpu_mixed, tables, main_set):
    """Inputs and outputs are the middle thirds of NaN-filled allocations: the result is the usual one and both guards of
    every output stay NaN."""
    import torch
    from kid_amd.radiometer import _RadiometerCfg, _RadiometerOut, library
    m, L = gpu_mixed, library()
    table = tables["absorbing"][0]
    st, dz, k_gas, t_sfc, _ = main_set
    ncol, nz = st["t"].shape
    whole = _run(m, table, st, dz, k_gas, t_sfc)

    def middle(a):
        buf = torch.full((3 * a.size,), float("nan"), dtype=torch.float64, device="cuda:0")
        buf[a.size:2 * a.size] = _cu(a.reshape(-1))
        return buf
    ins = {k: middle(st[k]) for k in ref.INPUTS}
    extra = {"dz": middle(dz), "k_gas": middle(k_gas), "t_sfc": middle(t_sfc)}
    outs = {n: torch.full((3 * int(np.prod(_out_shape(n, ncol, nz))),), float("nan"), dtype=torch.float64, device="cuda:0") for n in ref.NAMES}
    mid = lambda t: t.data_ptr() + 8 * (t.numel() // 3)   # noqa: E731
    o = _RadiometerOut(**{n: mid(t) for n, t in outs.items()})
    r = _RadiometerCfg(**rc.RCFG)
    rcode = L.kidmp_radiometer_device(m._h, table._t, C.byref(r), ncol, nz, *[mid(ins[k]) for k in ref.INPUTS], mid(extra["dz"]), 0,
                                      mid(extra["k_gas"]), 0, mid(extra["t_sfc"]), C.byref(o), torch.cuda.current_stream().cuda_stream)
    assert rcode == 0
    torch.cuda.synchronize()
    for n, t in outs.items():
        a = t.cpu().numpy()
        k = a.size // 3
        assert np.isnan(a[:k]).all() and np.isnan(a[2 * k:]).all(), n
        assert _same(a[k:2 * k].reshape(whole[n].shape), whole[n]), n


# ---- 4. the other entries ----
def test_binary32_entries_round_once(gpu_mixed, tables, main_set):
    table = tables["absorbing"][0]
    f = lambda a: a.astype(np.float32)   # noqa: E731
    d = lambda a: f(a).astype(np.float64)   # noqa: E731
    for st, dz, k_gas, t_sfc in [main_set[:4]] + [rc.state(nz) for nz in (2, 65, 256)]:   # three, then one, two and four level groups
        st32 = {k: f(v) for k, v in st.items()}
        got = _run(gpu_mixed, table, st32, f(dz), f(k_gas), f(t_sfc))
        ref64 = _run(gpu_mixed, table, {k: d(v) for k, v in st.items()}, d(dz), d(k_gas), d(t_sfc))
        for n in ref.NAMES:
            assert got[n].dtype == np.float32 and _same(got[n], ref64[n].astype(np.float32)), (st["t"].shape[1], n)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_entry_in_chunks_equals_the_device_entry(gpu_mixed, tables, main_set, dtype, monkeypatch):
    from padded_rows import with_padded
    from kid_amd.radiometer import library
    from kid_amd import RadiometerCfg
    m, table = gpu_mixed, tables["default"][0]
    st, dz, k_gas, t_sfc, _ = main_set
    st5 = {k: np.ascontiguousarray(v[:5].astype(dtype)) for k, v in st.items()}
    dz_, kg_, ts_ = dz.astype(dtype), k_gas.astype(dtype), np.ascontiguousarray(t_sfc[:5].astype(dtype))
    want = _run(m, table, st5, dz_, kg_, ts_)
    r = RadiometerCfg(**rc.RCFG)
    m.set_host_chunk(2)
    assert _same_all(m.radiometer_host(table, st5, dz_, kg_, ts_, r, want=ref.NAMES), want)
    some = ("tb_ground", "k_bsc", "tau_abs")
    part = m.radiometer_host(table, st5, dz_, kg_, ts_, r, want=some)
    assert sorted(part) == sorted(some) and all(_same(part[n], want[n]) for n in some)
    per_col = m.radiometer_host(table, st5, np.ascontiguousarray(np.tile(dz_, (5, 1))), np.ascontiguousarray(np.tile(kg_, (5, 1))), ts_, r,
                                want=ref.NAMES)
    assert _same_all(per_col, want)
    bare = m.radiometer_host(table, st5, dz_, None, None, None, want=("tb_toa",))      # no gas, t_sfc and rcfg left out
    assert _same(bare["tb_toa"], _run(m, table, st5, dz_, None, None, None, want=("tb_toa",))["tb_toa"])
    # seven columns with a dz and a k_gas of their own: one per chunk, then in chunks of 3, 3 and 1 with the rows of dz and
    # k_gas nz + 5 apart (dz_col_stride, k_gas_col_stride)
    idx = np.arange(7) % st["t"].shape[0]
    st7 = {k: np.ascontiguousarray(v[idx].astype(dtype)) for k, v in st.items()}
    scale = np.linspace(0.5, 2.0, 7)[:, None]
    dz7, kg7, ts7 = np.ascontiguousarray((dz * scale).astype(dtype)), np.ascontiguousarray((k_gas / scale).astype(dtype)), np.ascontiguousarray(t_sfc[idx].astype(dtype))
    want7 = _run(m, table, st7, dz7, kg7, ts7)
    m.set_host_chunk(1)
    assert _same_all(m.radiometer_host(table, st7, dz7, kg7, ts7, r, want=ref.NAMES), want7)
    m.set_host_chunk(3)
    seen = with_padded(monkeypatch, library(), "kidmp_radiometer_host" if dtype == np.float64 else "kidmp32_radiometer_host", {13: dz7, 15: kg7})
    assert _same_all(m.radiometer_host(table, st7, dz7, kg7, ts7, r, want=ref.NAMES), want7) and seen == [(13, 134), (15, 134)]


def test_hip_graph_replay_of_one_captured_launch(gpu_mixed, tables, main_set):
    import torch
    from kid_amd.radiometer import _RadiometerCfg, _RadiometerOut, library
    m, L = gpu_mixed, library()
    table = tables["absorbing"][0]
    st, dz, k_gas, t_sfc, _ = main_set
    ncol, nz = st["t"].shape
    dev = _dev(st)
    ddz, dkg, dts = _cu(dz), _cu(k_gas), _cu(t_sfc)
    names = ("tb_up", "trans", "tb_ground", "tau_abs")
    out = {n: torch.full(_out_shape(n, ncol, nz), -7.0, dtype=torch.float64, device="cuda:0") for n in names}
    o = _RadiometerOut(**{n: out[n].data_ptr() for n in names})
    r = _RadiometerCfg(**rc.RCFG)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rcode = L.kidmp_radiometer_device(m._h, table._t, C.byref(r), ncol, nz, *[dev[k].data_ptr() for k in ref.INPUTS], ddz.data_ptr(), 0,
                                          dkg.data_ptr(), 0, dts.data_ptr(), C.byref(o), torch.cuda.current_stream().cuda_stream)
    assert rcode == 0
    eager = _run(m, table, st, dz, k_gas, t_sfc, want=names)
    for _ in range(2):
        for t in out.values():
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert all(_same(out[n].cpu().numpy(), eager[n]) for n in names)


def test_an_iiwarm_context_has_no_snow_or_graupel(gpu_warm, consts):
    from kid_amd import MieCfg
    st, dz, k_gas, t_sfc = rc.state(64)
    with gpu_warm.radiometer_table(MieCfg(**rc.TABLES["absorbing"])) as t:
        rows = {x: t.get(x) for x in ref.SPECIES}
        got = _run(gpu_warm, t, st, dz, k_gas, t_sfc)
        none = _run(gpu_warm, t, {k: v for k, v in st.items() if k not in ("qs", "qg")}, dz, k_gas, t_sfc)
    assert _same_all(got, none)
    check_parity(got, ref.radiometer(consts, rc.cfg_of("absorbing"), rows, st, dz, k_gas, t_sfc, warm=True, **rc.RCFG))


def test_the_table_is_the_host_entrys(gpu_mixed, tables):
    """kidmp_radiometer_table_get returns what kidmp_radiometer_bins forms on the scheme's own bins, bit for bit."""
    from kid_amd import MieCfg, default_grid, radiometer_bins
    for name, (t, _, rows) in tables.items():
        for x in ref.SPECIES:
            D, dD = default_grid(gpu_mixed, x)
            assert _same(rows[x][0], np.asarray(D)) and _same(rows[x][1], np.asarray(dD))
            assert _same(rows[x][2], radiometer_bins(MieCfg(**rc.TABLES[name]), x, rows[x][0])), (name, x)
        c = t.cfg
        assert (c.wavelength, c.eps_w, c.eps_i) == (MieCfg(**rc.TABLES[name]).wavelength, MieCfg(**rc.TABLES[name]).eps_w, MieCfg(**rc.TABLES[name]).eps_i)


def test_refusals_write_nothing(gpu_mixed, gpu_warm, tables, main_set):
    import torch
    from kid_amd.radiometer import _RadiometerCfg, _RadiometerOut, library
    L = library()
    table = tables["absorbing"][0]
    st, dz, k_gas, t_sfc, _ = main_set
    ncol, nz = st["t"].shape
    dev = _dev(st)
    ddz = _cu(dz)
    out = torch.full((ncol, nz), -7.0, dtype=torch.float64, device="cuda:0")
    host = torch.zeros(ncol * nz, dtype=torch.float64)
    nan, inf = float("nan"), float("inf")

    def call(m=gpu_mixed, tab=table._t, ncol=ncol, nz=nz, dz=ddz.data_ptr(), stride=0, kstride=0, names=("tb_up",), t_sfc=None, rcfg=rc.RCFG, **over):
        p = {k: v.data_ptr() for k, v in dev.items()}
        p.update(over)
        o = _RadiometerOut(**{n: out.data_ptr() for n in names})
        r = None if rcfg is None else C.byref(_RadiometerCfg(**rcfg))
        return L.kidmp_radiometer_device(m._h if m is not None else None, tab, r, ncol, nz, *[p[k] for k in ref.INPUTS], dz, stride, None,
                                         kstride, t_sfc, C.byref(o), None)

    good = dict(rc.RCFG)
    with gpu_warm.radiometer_table() as other:
        refused = [dict(t=None), dict(p=None), dict(qv=None), dict(qr=None), dict(nr=None), dict(nz=1), dict(nz=257), dict(ncol=-1),
                   dict(names=()), dict(dz=None), dict(dz=None, names=("tau_abs",)), dict(dz=None, names=("refl",)), dict(stride=nz - 1),
                   dict(kstride=1), dict(tab=None), dict(tab=other._t), dict(t=host.data_ptr()), dict(qc=host.data_ptr()),
                   dict(dz=host.data_ptr()), dict(t_sfc=host.data_ptr())]
        refused += [dict(rcfg=dict(good, **kw)) for kw in (dict(mu=0.0), dict(mu=-0.5), dict(mu=1.0000001), dict(mu=nan), dict(emissivity=-1e-9),
                                                           dict(emissivity=1.0000001), dict(emissivity=nan), dict(t_cosmic=-1.0),
                                                           dict(t_cosmic=inf), dict(t_cosmic=nan))]
        for kw in refused:
            assert call(**kw) == -1, kw
            assert L.kidmp_last_error(gpu_mixed._h), kw
    assert call(m=None) == -5 and call(ncol=0) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()
    assert call(qc=None, qs=None, qg=None, rcfg=None) == 0 and call(dz=None, names=("k_abs",)) == 0
    torch.cuda.synchronize()
    assert np.isfinite(out.cpu().numpy()).all()
