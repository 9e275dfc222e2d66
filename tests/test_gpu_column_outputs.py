"""The column outputs on the MI355X: calc_effectRad (M:4834-4935) and calc_refl10cm (M:4946-5244) of a column from one read
of its state (kidmp::k_column_outputs, kid_amd/csrc/thompson_reflectivity.hip), the generalised pointwise radii kernel and
their C ABI / Python entries, against Oracle.calc_effectRad and tests/refl_oracle.py.

No tolerance is new: radii 1e-12 relative (test_effective_radii_match_oracle), dBZ 3e-13 dB (BOUND_DB of
test_gpu_reflectivity.py); everything else is equality of bits.  The tests print their measured maxima."""
import ctypes as C

import numpy as np
import pytest

import cases
import effrad_cases as ec
import refl_oracle as ro

pytestmark = pytest.mark.gpu

BOUND_RE = 1e-12
BOUND_DB = 3e-13
NZ_SWEEP = (2, 63, 64, 65, 120, 128, 129, 256)
NAMES = ec.NAMES
REFL_KEYS = ("t", "p", "qv", "qr", "nr", "qs", "qg")


@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = ro.constants(o)
    o.close()
    return c


def _dev(st, dtype=None, keys=NAMES):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(st[k] if dtype is None else st[k].astype(dtype))).to("cuda:0")
            for k in keys if st.get(k) is not None}


def _np(x):
    return None if x is None else x.cpu().numpy()


def _outputs(m, st, dbz=True, radii=True, dtype=None):
    """column_outputs of a numpy state: (dbz, (re_qc, re_qi, re_qs)) as numpy arrays."""
    import torch
    d, r = m.column_outputs(_dev(st, dtype), dbz=dbz, radii=radii)
    torch.cuda.synchronize()
    return _np(d), (None if r is None else tuple(_np(a) for a in r))


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _errors(m, o, c, st):
    """max relative error of the three radii against the oracle started from the presets, max |ddBZ| against refl_oracle"""
    dbz, radii = _outputs(m, st)
    want = o.calc_effectRad(st)
    assert np.all(np.isfinite(dbz)) and all(np.all(np.isfinite(r)) for r in radii)
    e_re = max(float(np.max(np.abs(g - w) / w)) for g, w in zip(radii, want))
    e_db = float(np.max(np.abs(dbz - ro.of_state(c, {k: st[k] for k in REFL_KEYS}))))
    return e_re, e_db


def _dry(nz=120):
    """Levels with qv below the 1e-10 that calc_refl10cm clamps to and calc_effectRad does not (M:4992 / M:4860)."""
    st = ec.random_state(nz, 16, 77)
    st["qv"][:, ::3] = 0.0
    st["qv"][:, 1::7] = 3e-11
    return st


@pytest.mark.parametrize("ctx", ["mixed", "aero"])
def test_all_four_match_the_oracles(request, consts, ctx):
    m = request.getfixturevalue("gpu_mixed" if ctx == "mixed" else "gpu_mixed_aero")
    o = request.getfixturevalue("oracle_mixed" if ctx == "mixed" else "oracle_mixed_aero")
    worst_re = worst_db = 0.0
    for st in (ec.batch(), ec.stack(ec.hand_built()), _dry()):
        e_re, e_db = _errors(m, o, consts, st)
        worst_re, worst_db = max(worst_re, e_re), max(worst_db, e_db)
    print("column outputs (%s; batch, hand-built, dry): max rel |dre| = %.3e, max |ddBZ| = %.3e dB" % (ctx, worst_re, worst_db))
    assert worst_re <= BOUND_RE
    assert worst_db <= BOUND_DB


@pytest.mark.parametrize("nz", NZ_SWEEP)
def test_all_four_nz_sweep(gpu_mixed, gpu_mixed_aero, oracle_mixed, oracle_mixed_aero, consts, nz):
    st = ec.random_state(nz, 96, 200 + nz)
    e_re, e_db = _errors(gpu_mixed, oracle_mixed, consts, st)
    a_re, a_db = _errors(gpu_mixed_aero, oracle_mixed_aero, consts, st)
    print("column outputs nz=%d: max rel |dre| = %.3e (aerosol-aware %.3e), max |ddBZ| = %.3e dB" % (nz, e_re, a_re, max(e_db, a_db)))
    assert max(e_re, a_re) <= BOUND_RE
    assert max(e_db, a_db) <= BOUND_DB


@pytest.mark.parametrize("ctx", ["mixed", "aero"])
def test_bits_against_the_separate_entries(request, ctx):
    import torch
    m = request.getfixturevalue("gpu_mixed" if ctx == "mixed" else "gpu_mixed_aero")
    for st in (ec.random_state(120, 64, 5), ec.random_state(129, 24, 6), ec.stack(ec.hand_built()), _dry(), ec.batch()):
        dev = _dev(st)
        dbz_ref = m.reflectivity(dev).cpu().numpy()
        re_ref = [a.cpu().numpy() for a in m.effective_radii(dev)]
        torch.cuda.synchronize()
        dbz, radii = _outputs(m, st)
        dbz_only, none = _outputs(m, st, radii=False)
        none2, radii_only = _outputs(m, st, dbz=False)
        assert none is None and none2 is None
        assert _same(dbz_only, dbz_ref) and _same(dbz, dbz_ref)
        for a, b, r in zip(radii, radii_only, re_ref):
            assert _same(a, r) and _same(b, r)
        again = _outputs(m, st)
        assert _same(again[0], dbz) and all(_same(a, b) for a, b in zip(again[1], radii))
    st = ec.random_state(120, 64, 5)
    dbz, radii = _outputs(m, st)
    for i in (0, 17, 63):                        # a column alone == the same column in a batch
        d1, r1 = _outputs(m, {k: v[i:i + 1] for k, v in st.items()})
        assert _same(d1[0], dbz[i]) and all(_same(a[0], b[i]) for a, b in zip(r1, radii))


SENTINELS = (-1.0, -2.0, -3.0)


def test_keep_mode_host_entry(gpu_mixed, oracle_mixed):
    """effective_radii_host is the subroutine's INOUT: exactly the levels without the species keep the caller's value."""
    import torch
    L = __import__("kid_amd").load_library()
    st = ec.random_state(65, 100, 31)            # 6 500 elements: four chunks of 16 x 128
    kept = [r == s for r, s in zip(oracle_mixed.calc_effectRad(st, preset=SENTINELS), SENTINELS)]
    gpu_mixed.set_host_chunk(16)
    try:
        for dtype in (np.float64, np.float32):
            s = {k: np.ascontiguousarray(v.astype(dtype)) for k, v in st.items()}
            host = gpu_mixed.effective_radii_host(s, preset=SENTINELS)
            if dtype == np.float64:
                d = gpu_mixed.effective_radii(_dev(s), preset=SENTINELS)
                torch.cuda.synchronize()
                device = [a.cpu().numpy() for a in d]
                for h, k, sv in zip(host, kept, SENTINELS):
                    assert np.array_equal(h == sv, k) and k.any() and (~k).any()
            else:
                dev = _dev(s, keys=ec.RADII_IN)
                out = [torch.full_like(dev["t"], v) for v in SENTINELS]
                rc = L.kidmp32_effective_radii_device(gpu_mixed._h, dev["t"].numel(), *[dev[k].data_ptr() for k in ec.RADII_IN],
                                                      *[a.data_ptr() for a in out], torch.cuda.current_stream().cuda_stream)
                assert rc == 0
                torch.cuda.synchronize()
                device = [a.cpu().numpy() for a in out]
                wide = gpu_mixed.effective_radii_host({k: v.astype(np.float64) for k, v in s.items()}, preset=SENTINELS)
                for h, w in zip(host, wide):     # the fp64 result on the widened inputs, rounded once
                    assert _same(h, w.astype(np.float32))
            for h, g in zip(host, device):
                assert h.dtype == dtype and _same(h, g)
            # seven columns, a chunk setting of 1: 455 elements in chunks of 128, the last one of 71
            gpu_mixed.set_host_chunk(1)
            s7 = {k: np.ascontiguousarray(v[:7]) for k, v in s.items()}
            host7 = gpu_mixed.effective_radii_host(s7, preset=SENTINELS)
            for h, g in zip(host7, device):
                assert h.dtype == dtype and h.shape == (7, 65) and _same(h, g[:7])
            gpu_mixed.set_host_chunk(16)
    finally:
        gpu_mixed.set_host_chunk(0)


def test_float32_entries_are_fp64_kernels_on_widened_inputs(gpu_mixed, gpu_mixed_aero):
    for m in (gpu_mixed, gpu_mixed_aero):
        for st in (ec.random_state(129, 40, 9), ec.stack(ec.hand_built())):
            st32 = {k: v.astype(np.float32) for k, v in st.items()}
            wide_in = {k: v.astype(np.float64) for k, v in st32.items()}
            for dbz, radii in ((True, True), (True, False), (False, True)):
                got = _outputs(m, st32, dbz=dbz, radii=radii)
                wide = _outputs(m, wide_in, dbz=dbz, radii=radii)
                if dbz:
                    assert got[0].dtype == np.float32 and _same(got[0], wide[0].astype(np.float32))
                if radii:
                    for g, w in zip(got[1], wide[1]):
                        assert g.dtype == np.float32 and _same(g, w.astype(np.float32))
            host = m.effective_radii_host({k: st32[k] for k in ec.RADII_IN})
            for h, w in zip(host, _outputs(m, wide_in, dbz=False)[1]):
                assert _same(h, w.astype(np.float32))


def _call_outputs(m, dev, out, nz=None, ncol=None, fn="kidmp_column_outputs_device", names=NAMES):
    """the C entry itself: dev maps names to tensors (missing = NULL), out = four tensors or None"""
    import torch
    from kid_amd.thompson import _Outputs, load_library
    t = next(v for v in dev.values() if v is not None)
    o = _Outputs(*[None if a is None else a.data_ptr() for a in out])
    return getattr(load_library(), fn)(m._h, t.shape[0] if ncol is None else ncol, t.shape[1] if nz is None else nz,
                                       *[dev[k].data_ptr() if dev.get(k) is not None else None for k in names], C.byref(o),
                                       torch.cuda.current_stream().cuda_stream)


def test_warm_context_and_optional_arrays(gpu_warm, gpu_mixed, oracle_warm, consts):
    import torch
    st = ec.random_state(120, 32, 21)
    for k in ("qi", "ni", "qs", "qg"):
        st[k][:] = 0.0
    want_re = oracle_warm.calc_effectRad(st)
    want_db = ro.of_state(consts, {k: st[k] for k in REFL_KEYS})
    few = {k: v for k, v in st.items() if k not in ("qi", "ni", "qs", "qg", "nc")}
    dbz, radii = _outputs(gpu_warm, few)                                       # frozen species and nc left out
    assert np.max(np.abs(dbz - want_db)) <= BOUND_DB
    assert np.max(np.abs(radii[0] - want_re[0]) / want_re[0]) <= BOUND_RE
    assert np.all(radii[1] == 4.99e-6) and np.all(radii[2] == 9.99e-6)         # passed: all preset
    full = _outputs(gpu_warm, st)
    assert _same(full[0], dbz) and all(_same(a, b) for a, b in zip(full[1], radii))
    dev = _dev(few)
    o_dbz, o_qc = torch.empty_like(dev["t"]), torch.empty_like(dev["t"])
    assert _call_outputs(gpu_warm, dev, (o_dbz, o_qc, None, None)) == 0       # re_qi, re_qs left out
    assert _call_outputs(gpu_warm, dev, (None, o_qc, None, None)) == 0
    torch.cuda.synchronize()
    assert _same(o_dbz.cpu().numpy(), dbz) and _same(o_qc.cpu().numpy(), radii[0])
    assert _call_outputs(gpu_warm, dev, (o_dbz, o_qc, o_qc, None)) == -1      # half a pair
    host = gpu_warm.effective_radii_host({k: few[k] for k in ("t", "p", "qv", "qc")})
    assert _same(host[0], radii[0]) and np.all(host[1] == 4.99e-6) and np.all(host[2] == 9.99e-6)
    # a context that is not aerosol-aware never reads nc
    mixed = ec.random_state(120, 32, 22)
    a = _outputs(gpu_mixed, mixed)
    b = _outputs(gpu_mixed, {k: v for k, v in mixed.items() if k != "nc"})
    assert _same(a[0], b[0]) and all(_same(x, y) for x, y in zip(a[1], b[1]))
    c = _outputs(gpu_mixed, {k: v for k, v in mixed.items() if k != "nc"}, dbz=False)
    assert all(_same(x, y) for x, y in zip(a[1], c[1]))


def _host_step(m, st, dt, entry, out=None, want_out=False):
    """kidmp_batch_step_host_{diag,refl,out} itself; st is stepped in place"""
    from kid_amd import STATE_NAMES, FORCING_NAMES, load_library
    from kid_amd.thompson import _Outputs
    L = load_library()
    ncol, nz = st["qv"].shape
    ppt = np.zeros((ncol, 4))
    rates = np.zeros((ncol, 36, nz))
    nstep = np.zeros((ncol, 4), dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    args = [m._h, ncol, nz, dt] + [dp(st[k]) for k in STATE_NAMES + FORCING_NAMES] + [dp(ppt), dp(rates),
                                                                                      nstep.ctypes.data_as(C.POINTER(C.c_int32))]
    if entry == "diag":
        rc = L.kidmp_batch_step_host_diag(*args)
    elif entry == "refl":
        rc = L.kidmp_batch_step_host_refl(*args, dp(out))
    else:
        o = _Outputs(*[None if a is None else a.ctypes.data for a in out]) if out is not None else None
        rc = L.kidmp_batch_step_host_out(*args, C.byref(o) if o is not None else None)
    assert rc == 0
    return ppt, rates, nstep


@pytest.mark.parametrize("chunk", [0, 1000])
def test_host_step_outputs(gpu_mixed, chunk):
    from kid_amd import STATE_NAMES
    ncol = 2500
    st0 = {k: np.ascontiguousarray(v) for k, v in cases.config3(ncol).items()}
    copy = lambda: {k: v.copy() for k, v in st0.items()}   # noqa: E731
    nz = st0["qv"].shape[1]
    gpu_mixed.set_host_chunk(chunk)              # 1000: three chunks through the three-stage pipeline
    try:
        a, b, c, d, e = copy(), copy(), copy(), copy(), copy()
        ra = _host_step(gpu_mixed, a, 10.0, "diag")
        dbz_refl = np.full((ncol, nz), np.nan)
        _host_step(gpu_mixed, b, 10.0, "refl", dbz_refl)
        outs = [np.full((ncol, nz), np.nan) for _ in range(4)]
        rc_ = _host_step(gpu_mixed, c, 10.0, "out", outs)
        rd = _host_step(gpu_mixed, d, 10.0, "out", None)                      # nothing requested
        re_ = _host_step(gpu_mixed, e, 10.0, "out", [None] * 4)
    finally:
        gpu_mixed.set_host_chunk(0)
    for other, res in ((c, rc_), (d, rd), (e, re_)):
        for k in STATE_NAMES:
            assert _same(a[k], other[k]), k
        assert _same(ra[0], res[0]) and _same(ra[1], res[1]) and np.array_equal(ra[2], res[2])
    assert _same(outs[0], dbz_refl)
    dbz, radii = _outputs(gpu_mixed, c)          # column_outputs of the post-step state
    assert _same(outs[0], dbz)
    for got, want in zip(outs[1:], radii):
        assert _same(got, want)


def test_host_step_python_and_binary32(gpu_mixed):
    from kid_amd import STATE_NAMES
    st = {k: np.ascontiguousarray(v) for k, v in cases.config3(300).items()}
    a = {k: v.copy() for k, v in st.items()}
    b = {k: v.copy() for k, v in st.items()}
    plain = gpu_mixed.batch_step_host(b, 10.0, want_rates=True)
    assert len(plain) == 2                       # return shapes unchanged when false
    ppt, rates, dbz, radii = gpu_mixed.batch_step_host(a, 10.0, want_rates=True, want_dbz=True, want_radii=True)
    for k in STATE_NAMES:
        assert _same(a[k], b[k]), k
    assert _same(ppt, plain[0]) and _same(rates, plain[1])
    want = _outputs(gpu_mixed, a)
    assert _same(dbz, want[0]) and all(_same(g, w) for g, w in zip(radii, want[1]))
    a2 = {k: v.copy() for k, v in st.items()}
    ppt2, rates2, radii2 = gpu_mixed.batch_step_host(a2, 10.0, want_radii=True)
    assert rates2 is None and all(_same(g, w) for g, w in zip(radii2, want[1]))
    s32 = {k: v.astype(np.float32) for k, v in st.items()}
    x = {k: v.copy() for k, v in s32.items()}
    y = {k: v.copy() for k, v in s32.items()}
    rx = gpu_mixed.batch_step32_host(x, 10.0, want_rates=True, want_nstep=True)
    assert len(rx) == 3
    py, ry, ny, dbz32, radii32 = gpu_mixed.batch_step32_host(y, 10.0, want_rates=True, want_nstep=True, want_dbz=True,
                                                             want_radii=True)
    for k in STATE_NAMES:
        assert _same(x[k], y[k]), k
    assert _same(rx[0], py) and _same(rx[1], ry) and np.array_equal(rx[2], ny)
    want32 = _outputs(gpu_mixed, y)
    assert dbz32.dtype == np.float32 and _same(dbz32, want32[0])
    for g, w in zip(radii32, want32[1]):
        assert g.dtype == np.float32 and _same(g, w)


def test_bad_arguments_are_refused(gpu_mixed, gpu_mixed_aero):
    import torch
    from kid_amd import load_library
    L = load_library()
    dev = _dev(ec.random_state(64, 4, 3))
    outs = tuple(torch.empty_like(dev["t"]) for _ in range(4))
    assert _call_outputs(gpu_mixed, dev, outs) == 0
    for k in ("t", "p", "qv", "qc", "qr", "nr"):                              # a null required array
        assert _call_outputs(gpu_mixed, {n: (None if n == k else v) for n, v in dev.items()}, outs) == -1, k
    for k in ("qi", "ni", "qs", "qg"):                                        # half a pair
        assert _call_outputs(gpu_mixed, {n: (None if n == k else v) for n, v in dev.items()}, outs) == -1, k
    for pair in (("qi", "ni"), ("qs", "qg")):                                 # a mixed-phase context needs them
        assert _call_outputs(gpu_mixed, {n: (None if n in pair else v) for n, v in dev.items()}, outs) == -1, pair
    assert _call_outputs(gpu_mixed, dev, (outs[0], outs[1], None, None)) == -1   # re_qi, re_qs: iiwarm only
    assert _call_outputs(gpu_mixed, dev, (outs[0], outs[1], outs[2], None)) == -1
    assert _call_outputs(gpu_mixed, dev, (outs[0], None, outs[2], outs[3])) == -1
    for nz in (1, 257):
        assert _call_outputs(gpu_mixed, dev, outs, nz=nz, ncol=1) == -1
    assert _call_outputs(gpu_mixed, dev, outs, ncol=-1) == -1
    host = np.zeros(4 * 64)                                                   # a host pointer on a device entry
    from kid_amd.thompson import _Outputs
    s = torch.cuda.current_stream().cuda_stream
    ptrs = [dev[k].data_ptr() for k in NAMES]
    good = _Outputs(*[a.data_ptr() for a in outs])
    assert L.kidmp_column_outputs_device(gpu_mixed._h, 4, 64, host.ctypes.data, *ptrs[1:], C.byref(good), s) == -1
    bad = _Outputs(outs[0].data_ptr(), host.ctypes.data, outs[2].data_ptr(), outs[3].data_ptr())
    assert L.kidmp_column_outputs_device(gpu_mixed._h, 4, 64, *ptrs, C.byref(bad), s) == -1
    no_nc = {n: (None if n == "nc" else v) for n, v in dev.items()}
    assert _call_outputs(gpu_mixed_aero, no_nc, outs) == -1                   # radii with nc null, aerosol-aware
    assert _call_outputs(gpu_mixed_aero, no_nc, (outs[0], None, None, None)) == 0   # the reflectivity does not read nc
    assert b"nc" in L.kidmp_last_error(gpu_mixed_aero._h)
    # the lenient radii entries
    st = ec.random_state(64, 4, 3)
    h = {k: st[k] for k in ec.RADII_IN}
    re = [np.full(st["t"].shape, v) for v in ec.PRESETS]
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    call = lambda m, hh, rr: L.kidmp_effective_radii_host(m._h, st["t"].size, *[dp(hh.get(k)) for k in ec.RADII_IN], *[dp(a) for a in rr])   # noqa: E731
    assert call(gpu_mixed, h, re) == 0
    assert call(gpu_mixed, {k: v for k, v in h.items() if k != "nc"}, re) == 0
    assert call(gpu_mixed_aero, {k: v for k, v in h.items() if k != "nc"}, re) == -1
    assert call(gpu_mixed, {k: v for k, v in h.items() if k != "qs"}, re) == -1
    assert call(gpu_mixed, {k: v for k, v in h.items() if k != "ni"}, re) == -1
    assert call(gpu_mixed, {k: v for k, v in h.items() if k != "t"}, re) == -1
    assert call(gpu_mixed, h, [re[0], None, None]) == -1
    # empty batches succeed, nothing requested succeeds
    assert _call_outputs(gpu_mixed, dev, outs, ncol=0) == 0
    assert L.kidmp_effective_radii_host(gpu_mixed._h, 0, *([None] * 11)) == 0            # nothing to point at
    assert L.kidmp_effective_radii_host(gpu_mixed._h, 0, *[dp(h[k]) for k in ec.RADII_IN], *[dp(a) for a in re]) == 0
    assert _call_outputs(gpu_mixed, dev, (None, None, None, None)) == 0
    assert L.kidmp_column_outputs_device(gpu_mixed._h, 4, 64, *ptrs, None, s) == 0
    # ... and a good call still works afterwards
    fresh = tuple(torch.full_like(dev["t"], float("nan")) for _ in range(4))
    assert _call_outputs(gpu_mixed, dev, fresh) == 0
    torch.cuda.synchronize()
    for a, b in zip(fresh, outs):
        assert _same(a.cpu().numpy(), b.cpu().numpy())
