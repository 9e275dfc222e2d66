"""Several channels of the radiometer and of the cloud radar in one launch on the MI355X (include/kidmp_multichannel.h,
kidmp::k_radiometer_multi, kidmp::k_mie_radar_multi).

Every comparison in this file is an equality of bits; nothing takes a tolerance.  The reference is the single-channel entry
(radiometer, mie_radar) with the channel's own table, closure and gas profile, which tests/test_gpu_radiometer.py and
tests/test_gpu_mie_radar.py hold to the numpy restatements.  Slab c of every output of a multi-channel call must equal it,
whatever the number of channels, the channel's place in the list, the other tables, the tile, the batch and the request.

States and the sixteen configurations: tests/multichannel_cases.py.  The single-channel references are formed once per
(kind, grid, nz, dtype) and shared by the tests.
"""
import ctypes as C

import numpy as np
import pytest

import multichannel_cases as mcc

pytestmark = pytest.mark.gpu

RAD_NAMES = ("k_abs", "k_bsc", "refl", "trans", "tb_up", "tb_down", "tb_toa", "tb_ground", "tau_abs")
MIE_NAMES = ("dbz", "dbz_up", "dbz_down", "dbz_r", "dbz_s", "dbz_g", "mie_r", "mie_s", "mie_g", "ext", "pia_up", "pia_down", "vd", "pia_total")


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _dev(st, dtype=None):
    return {k: _cu(v if dtype is None else v.astype(dtype)) for k, v in st.items() if v is not None}


def _opt(a, dtype=None):
    return None if a is None else _cu(a if dtype is None else a.astype(dtype))


def _host(out):
    import torch
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


def _rcfgs(n, first=0):
    from kid_amd import RadiometerCfg
    return [RadiometerCfg(**kw) for kw in mcc.rcfgs()[first:first + n]]


@pytest.fixture(scope="module")
def tables(gpu_mixed):
    """(kind, grid) -> the sixteen tables of tests/multichannel_cases.py, kind "rad" or "mie"."""
    from kid_amd import MieCfg
    out = {}
    for grid, g in mcc.GRIDS.items():
        out["rad", grid] = [gpu_mixed.radiometer_table(MieCfg(**kw), g) for kw in mcc.configs()]
        out["mie", grid] = [gpu_mixed.mie_table(MieCfg(**kw), g) for kw in mcc.configs()]
    yield out
    for ts in out.values():
        for t in ts:
            t.close()


@pytest.fixture(autouse=True)
def _leave_contexts_as_found(gpu_mixed, gpu_warm):
    yield
    for m in (gpu_mixed, gpu_warm):
        m.set_host_chunk(0)


def rad_singles(m, tabs, st, dz, kgs, t_sfc, rcfgs, want=RAD_NAMES, dtype=None):
    """The single-channel entry channel by channel: a list of dicts.  kgs: None, [nz] for all, or [nch, ...] per channel."""
    d, ddz, dts = _dev(st, dtype), _opt(dz, dtype), _opt(t_sfc, dtype)
    per = kgs is not None and kgs.ndim > 1 and kgs.shape[0] == len(tabs)          # the tests give the singles no [ncol, nz]
    return [_host(m.radiometer(t, d, ddz, _opt(kgs[c] if per else kgs, dtype), dts, rcfgs[c], want)) for c, t in enumerate(tabs)]


def _per_channel(kgs, nch, ncol):
    """[nch, nz] as it is, but [nch, ncol, nz] where nch == ncol would have it read as [ncol, nz]."""
    if kgs is not None and kgs.ndim == 2 and kgs.shape[0] == nch == ncol:
        return np.ascontiguousarray(np.repeat(kgs[:, None, :], ncol, axis=1))
    return kgs


def rad_multi(m, tabs, st, dz, kgs, t_sfc, rcfgs, want=RAD_NAMES, dtype=None, out=None):
    kgs = _per_channel(kgs, len(tabs), st["t"].shape[0])
    return _host(m.radiometer_multi(list(tabs), _dev(st, dtype), _opt(dz, dtype), _opt(kgs, dtype), _opt(t_sfc, dtype), rcfgs, want, out))


def mie_singles(m, tabs, st, dz, w, kgs, want=MIE_NAMES, dtype=None):
    d, ddz, dw = _dev(st, dtype), _opt(dz, dtype), _opt(w, dtype)
    per = kgs is not None and kgs.ndim > 1 and kgs.shape[0] == len(tabs)          # the tests give the singles no [ncol, nz]
    return [_host(m.mie_radar(t, d, ddz, dw, _opt(kgs[c] if per else kgs, dtype), want)) for c, t in enumerate(tabs)]


def mie_multi(m, tabs, st, dz, w, kgs, want=MIE_NAMES, dtype=None, out=None):
    kgs = _per_channel(kgs, len(tabs), st["t"].shape[0])
    return _host(m.mie_radar_multi(list(tabs), _dev(st, dtype), _opt(dz, dtype), _opt(w, dtype), _opt(kgs, dtype), want, out))


def assert_slabs(multi, singles, names=None, first=0):
    """Slab c of every output of `multi` holds the bits of singles[first + c]."""
    for n, a in multi.items():
        if names is not None and n not in names:
            continue
        for c in range(a.shape[0]):
            assert _same(np.ascontiguousarray(a[c]), singles[first + c][n]), (n, c)


_REFS = {}


def rad_reference(m, tables, grid, nz, dtype=None):
    """(state, the sixteen single-channel results) of the radiometer at nz levels on a grid: formed once, never changed."""
    key = ("rad", grid, nz, dtype)
    if key not in _REFS:
        st, dz, k_gas, t_sfc = mcc.radiometer_state(nz)
        kgs = mcc.k_gas_per_channel(k_gas)
        _REFS[key] = ((st, dz, kgs, t_sfc), rad_singles(m, tables["rad", grid], st, dz, kgs, t_sfc, _rcfgs(16), dtype=dtype))
    return _REFS[key]


def mie_reference(m, tables, grid, nz, dtype=None):
    key = ("mie", grid, nz, dtype)
    if key not in _REFS:
        st, dz, w, k_gas = mcc.radar_state(nz)
        kgs = mcc.k_gas_per_channel(k_gas)
        _REFS[key] = ((st, dz, w, kgs), mie_singles(m, tables["mie", grid], st, dz, w, kgs, dtype=dtype))
    return _REFS[key]


# ---- 1., 2. every output, slab by slab, across the tile ----
@pytest.mark.parametrize("grid", sorted(mcc.GRIDS))
@pytest.mark.parametrize("nz", mcc.NZS)
def test_radiometer_slabs_are_the_single_channel_bits(gpu_mixed, tables, nz, grid):
    from kid_amd import multichannel_tile
    (st, dz, kgs, t_sfc), ref = rad_reference(gpu_mixed, tables, grid, nz)
    tile = multichannel_tile("radiometer", nz)
    counts = mcc.channel_counts(tile)
    print("nz %d: tile %d, channel counts %s" % (nz, tile, counts))
    assert 1 <= tile <= 16 and any(n > tile for n in counts)
    for nch in counts:
        got = rad_multi(gpu_mixed, tables["rad", grid][:nch], st, dz, kgs[:nch], t_sfc, _rcfgs(nch))
        assert sorted(got) == sorted(RAD_NAMES)
        assert all(got[n].shape == ((nch, 7) if n in ("tb_toa", "tb_ground", "tau_abs") else (nch, 7, nz)) for n in got)
        assert_slabs(got, ref)
    # the channels differ: the test would not see a wrong row pointer otherwise
    assert not _same(ref[0]["k_abs"], ref[1]["k_abs"]) and not _same(ref[3]["tb_toa"], ref[4]["tb_toa"])


@pytest.mark.parametrize("grid", sorted(mcc.GRIDS))
@pytest.mark.parametrize("nz", mcc.NZS)
def test_radar_slabs_are_the_single_channel_bits(gpu_mixed, tables, nz, grid):
    from kid_amd import multichannel_tile
    (st, dz, w, kgs), ref = mie_reference(gpu_mixed, tables, grid, nz)
    tile = multichannel_tile("radar", nz)
    counts = mcc.channel_counts(tile, beyond=False)
    print("nz %d: tile %d, channel counts %s" % (nz, tile, counts))
    assert 1 <= tile <= 16 and any(n > tile for n in counts)
    for nch in counts:
        got = mie_multi(gpu_mixed, tables["mie", grid][:nch], st, dz, w, kgs[:nch])
        assert sorted(got) == sorted(MIE_NAMES)
        assert all(got[n].shape == ((nch, 7) if n == "pia_total" else (nch, 7, nz)) for n in got)
        assert_slabs(got, ref)
    assert not _same(ref[0]["dbz"], ref[1]["dbz"]) and not _same(ref[3]["ext"], ref[4]["ext"])


# ---- 3. independence ----
def test_radiometer_bits_do_not_depend_on_the_list_the_request_the_batch_or_a_repeat(gpu_mixed, tables):
    import torch
    from kid_amd import multichannel_tile
    m, nz = gpu_mixed, 129
    (st, dz, kgs, t_sfc), ref = rad_reference(m, tables, "scheme", nz)
    tabs = tables["rad", "scheme"]
    nch = 2 * multichannel_tile("radiometer", nz) + 1
    nch = min(nch, 16)
    r = _rcfgs(16)
    whole = rad_multi(m, tabs[:nch], st, dz, kgs[:nch], t_sfc, r[:nch])
    back = rad_multi(m, tabs[:nch][::-1], st, dz, np.ascontiguousarray(kgs[:nch][::-1]), t_sfc, r[:nch][::-1])     # reversed
    assert _same_all({n: np.ascontiguousarray(v[::-1]) for n, v in back.items()}, whole)
    twice = rad_multi(m, [tabs[2], tabs[5], tabs[2]], st, dz, np.ascontiguousarray(kgs[[2, 5, 2]]), t_sfc, [r[2], r[5], r[2]])
    for n, v in twice.items():                                                         # the same table twice
        assert _same(v[0], v[2]) and _same(np.ascontiguousarray(v[0]), ref[2][n]) and _same(np.ascontiguousarray(v[1]), ref[5][n]), n
    for want in (("tb_toa",), ("k_abs", "k_bsc"), ("tau_abs",), ("refl", "trans"), ("tb_down", "tb_ground"), ("tb_up", "k_bsc", "tau_abs")):
        part = rad_multi(m, tabs[:nch], st, dz, kgs[:nch], t_sfc, r[:nch], want=want)
        assert sorted(part) == sorted(want) and all(_same(part[n], whole[n]) for n in want), want
    no_dz = rad_multi(m, tabs[:nch], st, None, kgs[:nch], t_sfc, r[:nch], want=("k_abs", "k_bsc"))
    assert _same(no_dz["k_abs"], whole["k_abs"]) and _same(no_dz["k_bsc"], whole["k_bsc"])
    for idx in (slice(4, 5), np.array([6, 0, 3])):                                     # 1 and 3 of the 7 columns
        some = rad_multi(m, tabs[:nch], _take(st, idx), dz, kgs[:nch], np.ascontiguousarray(t_sfc[idx]), r[:nch])
        assert _same_all(some, {n: np.ascontiguousarray(v[:, idx]) for n, v in whole.items()})
    # k_gas [nch, ncol, nz], [ncol, nz] and [nz], and one closure for all channels
    full = rad_multi(m, tabs[:nch], st, np.tile(dz, (7, 1)), np.ascontiguousarray(np.repeat(kgs[:nch, None, :], 7, axis=1)), t_sfc, r[:nch])
    assert _same_all(full, whole)
    one_gas = rad_multi(m, tabs[:3], st, dz, kgs[1], t_sfc, r[1])
    per_col = rad_multi(m, tabs[:3], st, dz, np.ascontiguousarray(np.tile(kgs[1], (7, 1))), t_sfc, [r[1]] * 3)
    single = rad_singles(m, tabs[:3], st, dz, kgs[1], t_sfc, [r[1]] * 3)
    assert_slabs(one_gas, single)
    assert _same_all(per_col, one_gas)
    out = {n: torch.full(tuple(v.shape), -7.0, dtype=torch.float64, device="cuda:0") for n, v in whole.items()}   # a repeated call into out=
    for _ in range(2):
        got = m.radiometer_multi(tabs[:nch], _dev(st), _cu(dz), _cu(kgs[:nch]), _cu(t_sfc), r[:nch], RAD_NAMES, out)
        assert all(got[n] is out[n] for n in out)
        assert _same_all(_host(out), whole)


def test_radar_bits_do_not_depend_on_the_list_the_request_the_batch_or_a_repeat(gpu_mixed, tables):
    import torch
    from kid_amd import multichannel_tile
    m, nz = gpu_mixed, 129
    (st, dz, w, kgs), ref = mie_reference(m, tables, "scheme", nz)
    tabs = tables["mie", "scheme"]
    nch = min(2 * multichannel_tile("radar", nz) + 1, 16)
    whole = mie_multi(m, tabs[:nch], st, dz, w, kgs[:nch])
    back = mie_multi(m, tabs[:nch][::-1], st, dz, w, np.ascontiguousarray(kgs[:nch][::-1]))
    assert _same_all({n: np.ascontiguousarray(v[::-1]) for n, v in back.items()}, whole)
    twice = mie_multi(m, [tabs[1], tabs[4], tabs[1]], st, dz, w, np.ascontiguousarray(kgs[[1, 4, 1]]))
    for n, v in twice.items():
        assert _same(v[0], v[2]) and _same(np.ascontiguousarray(v[0]), ref[1][n]) and _same(np.ascontiguousarray(v[1]), ref[4][n]), n
    for want in (("dbz",), ("dbz_s", "mie_s"), ("mie_g",), ("dbz_r",), ("ext",), ("vd",), ("pia_total",), ("dbz_up", "pia_down"), ("dbz_g", "vd", "pia_up")):
        part = mie_multi(m, tabs[:nch], st, dz, w, kgs[:nch], want=want)
        assert sorted(part) == sorted(want) and all(_same(part[n], whole[n]) for n in want), want
    no_dz = mie_multi(m, tabs[:nch], st, None, w, kgs[:nch], want=("dbz", "ext", "vd"))
    assert all(_same(no_dz[n], whole[n]) for n in no_dz)
    for idx in (slice(4, 5), np.array([6, 0, 3])):
        some = mie_multi(m, tabs[:nch], _take(st, idx), dz, np.ascontiguousarray(w[idx]), kgs[:nch])
        assert _same_all(some, {n: np.ascontiguousarray(v[:, idx]) for n, v in whole.items()})
    full = mie_multi(m, tabs[:nch], st, np.tile(dz, (7, 1)), w, np.ascontiguousarray(np.repeat(kgs[:nch, None, :], 7, axis=1)))
    assert _same_all(full, whole)
    out = {n: torch.full(tuple(v.shape), -7.0, dtype=torch.float64, device="cuda:0") for n, v in whole.items()}
    for _ in range(2):
        m.mie_radar_multi(tabs[:nch], _dev(st), _cu(dz), _cu(w), _cu(kgs[:nch]), MIE_NAMES, out)
        assert _same_all(_host(out), whole)


# ---- 4. other contexts and states ----
def test_an_iiwarm_context_absent_species_and_a_dry_column(gpu_warm, gpu_mixed, tables):
    from kid_amd import MieCfg, multichannel_tile
    nz = 65
    nch = multichannel_tile("radiometer", nz) + 1
    cfgs = [MieCfg(**kw) for kw in mcc.configs()[:nch]]
    st, dz, k_gas, t_sfc = mcc.radiometer_state(nz)
    kgs, r = mcc.k_gas_per_channel(k_gas, nch), _rcfgs(nch)
    rad = [gpu_warm.radiometer_table(c) for c in cfgs]
    mie = [gpu_warm.mie_table(c) for c in cfgs]
    try:
        got = rad_multi(gpu_warm, rad, st, dz, kgs, t_sfc, r)
        assert_slabs(got, rad_singles(gpu_warm, rad, st, dz, kgs, t_sfc, r))
        bare = {k: v for k, v in st.items() if k not in ("qs", "qg")}
        assert _same_all(rad_multi(gpu_warm, rad, bare, dz, kgs, t_sfc, r), got)
        rst, rdz, w, _ = mcc.radar_state(nz)
        got = mie_multi(gpu_warm, mie, rst, rdz, w, kgs)
        assert_slabs(got, mie_singles(gpu_warm, mie, rst, rdz, w, kgs))
    finally:
        for t in rad + mie:
            t.close()
    # the mixed-phase context: qc, qs and qg absent; t_sfc and k_gas absent
    m = gpu_mixed
    bare = {k: v for k, v in st.items() if k not in ("qc", "qs", "qg")}
    tabs = tables["rad", "scheme"][:nch]
    assert_slabs(rad_multi(m, tabs, bare, dz, None, None, r), rad_singles(m, tabs, bare, dz, None, None, r))
    rbare = {k: v for k, v in rst.items() if k not in ("qc", "qs", "qg")}
    tabs = tables["mie", "scheme"][:nch]
    assert_slabs(mie_multi(m, tabs, rbare, rdz, None, None), mie_singles(m, tabs, rbare, rdz, None, None))
    # a dry column (column 5 of the radar's state) alone, and a state without any hydrometeor
    dry = _take(rst, slice(5, 6))
    assert not any((dry[k] != 0).any() for k in ("qc", "qr", "nr", "qs", "qg"))
    got = mie_multi(m, tabs, dry, rdz, np.ascontiguousarray(w[5:6]), kgs)
    assert_slabs(got, mie_singles(m, tabs, dry, rdz, np.ascontiguousarray(w[5:6]), kgs))
    assert (got["mie_r"] == 1.0).all() and (_bits(got["vd"]) == 0).all()
    tabs = tables["rad", "scheme"][:nch]
    got = rad_multi(m, tabs, dry, rdz, kgs, None, r)
    assert_slabs(got, rad_singles(m, tabs, dry, rdz, kgs, None, r))
    assert (_bits(got["k_bsc"]) == 0).all()


# ---- 5. binary32 ----
def test_binary32_entries(gpu_mixed, tables):
    from kid_amd import multichannel_tile
    m, f = gpu_mixed, np.float32
    for nz in mcc.NZS:                                                            # every level-group count
        (st, dz, kgs, t_sfc), ref = rad_reference(m, tables, "scheme", nz, dtype=f)
        nch = multichannel_tile("radiometer", nz) + 1
        got = rad_multi(m, tables["rad", "scheme"][:nch], st, dz, kgs[:nch], t_sfc, _rcfgs(nch), dtype=f)
        assert all(v.dtype == f for v in got.values())
        assert_slabs(got, ref)
        (st, dz, w, kgs), ref = mie_reference(m, tables, "scheme", nz, dtype=f)
        nch = multichannel_tile("radar", nz) + 1
        got = mie_multi(m, tables["mie", "scheme"][:nch], st, dz, w, kgs[:nch], dtype=f)
        assert all(v.dtype == f for v in got.values())
        assert_slabs(got, ref)


# ---- 6. the host entries ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_entries_in_chunks_equal_the_device_entries(gpu_mixed, tables, dtype, monkeypatch):
    from padded_rows import with_padded
    from kid_amd import multichannel_tile
    from kid_amd.multichannel import library
    entry = lambda what: "%s_%s_multi_host" % ("kidmp" if dtype == np.float64 else "kidmp32", what)   # noqa: E731
    m, nz = gpu_mixed, 129
    f = lambda a: None if a is None else np.ascontiguousarray(a.astype(dtype))   # noqa: E731
    (st, dz, kgs, t_sfc), _ = rad_reference(m, tables, "scheme", nz)
    nch = multichannel_tile("radiometer", nz) + 1
    tabs, r = tables["rad", "scheme"][:nch], _rcfgs(nch)
    st_ = {k: f(v) for k, v in st.items()}
    want = rad_multi(m, tabs, st, dz, kgs[:nch], t_sfc, r, dtype=dtype)
    full_gas = np.ascontiguousarray(np.repeat(kgs[:nch, None, :], 7, axis=1))
    for chunk in (0, 1, 2, 3):
        m.set_host_chunk(chunk)
        assert _same_all(m.radiometer_multi_host(tabs, st_, f(dz), f(kgs[:nch]), f(t_sfc), r, RAD_NAMES), want), chunk
        per_col = m.radiometer_multi_host(tabs, st_, f(np.tile(dz, (7, 1))), f(full_gas), f(t_sfc), r, RAD_NAMES)
        assert _same_all(per_col, want), chunk
    with monkeypatch.context() as mp:                                                  # chunks of 3, 3 and 1, the rows of dz nz + 5 apart
        dz7 = f(np.tile(dz, (7, 1)))
        seen = with_padded(mp, library(), entry("radiometer"), {14: dz7})
        assert _same_all(m.radiometer_multi_host(tabs, st_, dz7, f(full_gas), f(t_sfc), r, RAD_NAMES), want) and seen == [(14, nz + 5)]
    some = ("tb_ground", "k_bsc", "tau_abs")
    part = m.radiometer_multi_host(tabs, st_, f(dz), f(kgs[:nch]), f(t_sfc), r, some)
    assert sorted(part) == sorted(some) and all(_same(part[n], want[n]) for n in some)
    bare = m.radiometer_multi_host(tabs, st_, f(dz))                                   # no gas, no t_sfc, the default closures
    assert _same(bare["tb_toa"], rad_multi(m, tabs, st, dz, None, None, None, want=("tb_toa",), dtype=dtype)["tb_toa"])

    (st, dz, w, kgs), _ = mie_reference(m, tables, "scheme", nz)
    nch = multichannel_tile("radar", nz) + 1
    tabs = tables["mie", "scheme"][:nch]
    st_ = {k: f(v) for k, v in st.items()}
    want = mie_multi(m, tabs, st, dz, w, kgs[:nch], dtype=dtype)
    full_gas = np.ascontiguousarray(np.repeat(kgs[:nch, None, :], 7, axis=1))
    for chunk in (0, 1, 2, 3):
        m.set_host_chunk(chunk)
        assert _same_all(m.mie_radar_multi_host(tabs, st_, f(dz), f(w), f(kgs[:nch]), MIE_NAMES), want), chunk
        assert _same_all(m.mie_radar_multi_host(tabs, st_, f(np.tile(dz, (7, 1))), f(w), f(full_gas), MIE_NAMES), want), chunk
    with monkeypatch.context() as mp:
        dz7 = f(np.tile(dz, (7, 1)))
        seen = with_padded(mp, library(), entry("mie_radar"), {13: dz7})
        assert _same_all(m.mie_radar_multi_host(tabs, st_, dz7, f(w), f(full_gas), MIE_NAMES), want) and seen == [(13, nz + 5)]
    part = m.mie_radar_multi_host(tabs, st_, f(dz), None, f(kgs[1]), ("pia_total", "dbz_s"))
    dev = mie_multi(m, tabs, st, dz, None, kgs[1], want=("pia_total", "dbz_s"), dtype=dtype)
    assert _same_all(part, dev)


# ---- 7. guarded buffers ----
def test_outputs_in_the_middle_of_nan_filled_tensors(gpu_mixed, tables):
    import torch
    from kid_amd import multichannel_tile
    m, nz = gpu_mixed, 65
    nan = float("nan")

    def guarded(shapes):
        bufs = {n: torch.full((3 * int(np.prod(s)),), nan, dtype=torch.float64, device="cuda:0") for n, s in shapes.items()}
        return bufs, {n: b[b.numel() // 3:2 * (b.numel() // 3)].view(shapes[n]) for n, b in bufs.items()}

    def check(bufs, ref):
        torch.cuda.synchronize()
        for n, b in bufs.items():
            a = b.cpu().numpy()
            k = a.size // 3
            assert np.isnan(a[:k]).all() and np.isnan(a[2 * k:]).all(), n
            mid = a[k:2 * k].reshape((-1,) + ref[0][n].shape)
            assert not np.isnan(mid).any(), n                                         # every element of every slab written
            for c in range(mid.shape[0]):
                assert _same(np.ascontiguousarray(mid[c]), ref[c][n]), (n, c)

    (st, dz, kgs, t_sfc), ref = rad_reference(m, tables, "scheme", nz)
    nch = multichannel_tile("radiometer", nz) + 1
    bufs, out = guarded({n: (nch, 7) if n in ("tb_toa", "tb_ground", "tau_abs") else (nch, 7, nz) for n in RAD_NAMES})
    m.radiometer_multi(tables["rad", "scheme"][:nch], _dev(st), _cu(dz), _cu(kgs[:nch]), _cu(t_sfc), _rcfgs(nch), RAD_NAMES, out)
    check(bufs, ref)
    (st, dz, w, kgs), ref = mie_reference(m, tables, "scheme", nz)
    nch = multichannel_tile("radar", nz) + 1
    bufs, out = guarded({n: (nch, 7) if n == "pia_total" else (nch, 7, nz) for n in MIE_NAMES})
    m.mie_radar_multi(tables["mie", "scheme"][:nch], _dev(st), _cu(dz), _cu(w), _cu(kgs[:nch]), MIE_NAMES, out)
    check(bufs, ref)


# ---- 8. refusals ----
def test_refusals_write_nothing(gpu_mixed, gpu_warm, tables):
    import torch
    from kid_amd import KidmpError, RadiometerCfg
    from kid_amd.mie import _MieOut
    from kid_amd.multichannel import library
    from kid_amd.radiometer import _RadiometerCfg, _RadiometerOut
    m, L, nz, nch = gpu_mixed, library(), 65, 3
    st, dz, k_gas, t_sfc = mcc.radiometer_state(nz)
    kgs = mcc.k_gas_per_channel(k_gas, nch)
    dev, ddz, dkg = _dev(st), _cu(dz), _cu(kgs)
    nan = float("nan")
    rad, mie = tables["rad", "scheme"], tables["mie", "scheme"]
    rout = {n: torch.full((nch, 7) if n in ("tb_toa", "tb_ground", "tau_abs") else (nch, 7, nz), nan, dtype=torch.float64, device="cuda:0")
            for n in RAD_NAMES}
    mout = {n: torch.full((nch, 7) if n == "pia_total" else (nch, 7, nz), nan, dtype=torch.float64, device="cuda:0") for n in MIE_NAMES}
    good = [RadiometerCfg(**kw) for kw in mcc.rcfgs(nch)]
    bad = good[:2] + [RadiometerCfg(mu=0.0)]
    with gpu_warm.radiometer_table() as other_rad, gpu_warm.mie_table() as other_mie:
        # through Python: refused before the library is called, or by it
        for tabs in ([rad[0], tables["rad", "caller"][1], rad[2]], [rad[0], other_rad, rad[2]], [], rad[:16] + rad[:1], [rad[0], None, rad[2]]):
            with pytest.raises(KidmpError):
                m.radiometer_multi(tabs, dev, ddz, None, None, None, RAD_NAMES, rout if len(tabs) == nch else None)
        with pytest.raises(KidmpError):
            m.radiometer_multi(rad[:nch], dev, ddz, dkg, None, bad, RAD_NAMES, rout)
        with pytest.raises(KidmpError):
            m.radiometer_multi(rad[:nch], dev, ddz, dkg, None, good[:2], RAD_NAMES, rout)
        for shape in ((nch + 1, nz), (nch, 7, nz + 1), (nch, 6, nz), (nz + 1,), (1, nch, 7, nz)):
            with pytest.raises(KidmpError):
                m.radiometer_multi(rad[:nch], dev, ddz, torch.zeros(shape, dtype=torch.float64, device="cuda:0"), None, good, RAD_NAMES, rout)
            with pytest.raises(KidmpError):
                m.mie_radar_multi(mie[:nch], dev, ddz, None, torch.zeros(shape, dtype=torch.float64, device="cuda:0"), MIE_NAMES, mout)
        for tabs in ([mie[0], tables["mie", "caller"][1], mie[2]], [mie[0], other_mie, mie[2]], [], mie[:16] + mie[:1], [mie[0], None, mie[2]],
                     [mie[0], rad[1], mie[2]]):
            with pytest.raises(KidmpError):
                m.mie_radar_multi(tabs, dev, ddz, None, None, MIE_NAMES, mout if len(tabs) == nch else None)

        # the library itself
        ro = _RadiometerOut(**{n: t.data_ptr() for n, t in rout.items()})
        mo = _MieOut(**{n: t.data_ptr() for n, t in mout.items()})
        ptrs = [dev[k].data_ptr() for k in ("t", "p", "qv", "qc", "qr", "nr", "qs", "qg")]
        handles = lambda ts: (C.c_void_p * max(len(ts), 1))(*[None if t is None else t._t for t in ts])   # noqa: E731
        cfgs = lambda rs: (_RadiometerCfg * len(rs))(*[_RadiometerCfg(r.mu, r.emissivity, r.t_cosmic) for r in rs])   # noqa: E731

        def rcall(tabs=rad[:nch], n=nch, r=good, ch_stride=nz, col_stride=0, h=m._h, null_tables=False):
            return L.kidmp_radiometer_multi_device(h, None if null_tables else handles(tabs), n, cfgs(r), 7, nz, *ptrs, ddz.data_ptr(), 0,
                                                   dkg.data_ptr(), col_stride, ch_stride, None, C.byref(ro), None)

        def mcall(tabs=mie[:nch], n=nch, ch_stride=nz, col_stride=0, h=m._h, null_tables=False):
            return L.kidmp_mie_radar_multi_device(h, None if null_tables else handles(tabs), n, 7, nz, *ptrs, ddz.data_ptr(), 0, None,
                                                  dkg.data_ptr(), col_stride, ch_stride, C.byref(mo), None)

        for call, ts, caller, other in ((rcall, rad, tables["rad", "caller"], other_rad), (mcall, mie, tables["mie", "caller"], other_mie)):
            refused = [dict(n=0), dict(n=17, tabs=ts[:16] + ts[:1]), dict(n=-1), dict(null_tables=True), dict(tabs=[ts[0], None, ts[2]]),
                       dict(tabs=[ts[0], other, ts[2]]), dict(tabs=[ts[0], ts[1], caller[2]]), dict(tabs=[caller[0], ts[1], ts[2]]),
                       dict(ch_stride=nz - 1), dict(ch_stride=1), dict(ch_stride=-nz), dict(col_stride=nz, ch_stride=6 * nz + nz - 1),
                       dict(col_stride=nz - 1)]
            for kw in refused:
                assert call(**kw) == -1, (call.__name__, kw)
                assert L.kidmp_last_error(m._h), kw
            assert call(h=None) == -5
        assert rcall(r=bad) == -1 and rcall(r=[good[0], RadiometerCfg(emissivity=1.5), good[2]]) == -1
        assert rcall(r=[good[0], good[1], RadiometerCfg(t_cosmic=nan)]) == -1
    torch.cuda.synchronize()
    for n, t in list(rout.items()) + list(mout.items()):
        assert torch.isnan(t).all(), n
    # and the same calls, left alone, succeed and fill every element
    assert rcall() == 0 and mcall() == 0 and rcall(ch_stride=0) == 0 and mcall(col_stride=0, ch_stride=0) == 0
    torch.cuda.synchronize()
    for n, t in list(rout.items()) + list(mout.items()):
        assert not torch.isnan(t).any(), n
