"""The spectrum processor on the MI355X (include/kidmp_specproc.h, kidmp::k_spectrum_process) against
tests/specproc_ref.py, the operator restated in numpy.  -m gpu.

Exact, bit for bit: a level without a width returns its input; a spectrum shifted by m bins gives outputs shifted by m
bins; the support, the half-width and the symmetry of the weight row a unit bin returns; every equality between two device
results (batch, column position, request subsets, out=, a repeat, sigma and noise as [nz] and as [ncol, nz], binary32
after one rounding, graph replay, the NaN-filled surroundings, add_noise); nbins, v_lo and v_hi against the restatement.

Against the restatement where exponentials are involved (the kernel's are fastmath.h's, the restatement's numpy's) the
bound is four times the largest difference measured on the MI355X over the cases of this file, MEASURED below, in units
of 2**-52: spec, lost_below and lost_above relative to the level's sum of the input, dbz as the relative difference of the
reflectivity it stands for (|d dB| ln(10)/10), vm and sw relative to max(|ref|, dv), skew and kurt relative to
max(|ref|, 1); `conservation` is |sum_j B_j + lost_below + lost_above - sum_i in[i]| relative to sum_i in[i] and
`variance` |(sw**2 with sigma - sw**2 without) - dv**2 K| relative to dv**2 K, K the discrete kernel's own variance
sum d**2 g_d / G.  The restatement's cases are chosen, and the tests assert on the CPU, so that no bin of the
restatement lies within 1e-9 relative of its detection threshold; no bin is exempted.
    spec 0.15  lost_below 0.50  lost_above 0.50  dbz 14.8  vm 9.2  sw 3.4  skew 168.1  kurt 13.7  conservation 9.3
    variance 1.18e6 (the difference of two variances near 1 m2/s2 against a kernel variance down to 1e-5 m2/s2 at H = 1)
The chain doppler_spectrum(total) -> spectrum_process against doppler_moments on three mixed-phase columns (v0 = -1,
dv = 1/16, 256 bins, the scheme's own diameter bins): the gap is the linear deposit's and the diameter grid's own, the
same on the device and in the numpy restatements of the two operators; measured on the device
    dbz 2.556e-02 dB   vm 1.503e-02 m/s   sw 7.972e-03 m/s   (the restatements: the same three figures)
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import specproc_cases as cases
import specproc_ref as ref

pytestmark = pytest.mark.gpu

ULP = 2.220446049250313e-16
# the largest differences from the restatement measured on the MI355X, in ulp (see the module docstring)
MEASURED = {"spec": 0.15, "lost_below": 0.50, "lost_above": 0.50, "dbz": 14.8, "vm": 9.2, "sw": 3.4, "skew": 168.1, "kurt": 13.7, "conservation": 9.3,
            "variance": 1.18e6}
FLOATS = ref.NAMES[:-1]
MOMENTS = ("dbz", "vm", "sw", "skew", "kurt")
V0, DV = cases.V0, cases.DV
SEEN = {}


def bound(kind):
    return 4.0 * MEASURED[kind] * ULP


def _seen(kind, value, what):
    SEEN[kind] = max(SEEN.get(kind, 0.0), value)
    print("measured %s: %s %.2f ulp (largest so far %.2f, bound %.2f)" % (what, kind, value, SEEN[kind], 4.0 * MEASURED[kind]))


def _sp():
    return importlib.import_module("kid_amd.specproc")


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _proc(m, spec, sigma=None, noise=None, want=ref.NAMES, dtype=None, v0=V0, dv=DV, **cfg):
    """spectrum_process of numpy inputs, back as numpy."""
    import torch
    from kid_amd import SpecCfg
    cast = (lambda a: a) if dtype is None else (lambda a: a.astype(dtype))
    out = m.spectrum_process(_cu(cast(spec)), v0, dv, None if sigma is None else _cu(cast(sigma)), None if noise is None else _cu(cast(noise)),
                             SpecCfg(**cfg), want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    diff = ref.bits(got) != ref.bits(want)
    assert not diff.any(), "%s: %d of %d differ, first at %s: %r vs %r" % (what, int(diff.sum()), diff.size, np.argwhere(diff)[0],
                                                                         got[tuple(np.argwhere(diff)[0])], want[tuple(np.argwhere(diff)[0])])


def _all_same(a, b, what, names=None):
    for n in names or sorted(a):
        _assert_same(a[n], b[n], "%s: %s" % (what, n))


def _noise_for(x, frac=0.03):
    """A noise level per column and level: `frac` of the level's largest bin, so that a peak is detected and its skirts are not."""
    return np.ascontiguousarray(frac * x.max(axis=1))


# ---- 1. levels without a width ----
@pytest.mark.parametrize("nz, nv, ncol", [(2, 1, 1), (65, 25, 3), (120, 64, 5), (256, 2, 3)])
def test_no_width_returns_the_input_bits(gpu_mixed, nz, nv, ncol):
    x = cases.spectrum(ncol, nv, nz, seed=nz + nv)
    x[:, ::3, ::2] = -0.0                                              # a negative zero survives only as bits
    x[0, 0, 0] = 0.0
    got = _proc(gpu_mixed, x)                                          # sigma NULL
    _assert_same(got["spec"], x, "sigma NULL: spec")
    for n in ("lost_below", "lost_above"):
        _assert_same(got[n], np.zeros((ncol, nz)), "sigma NULL: " + n)
    want = ref.process(x, V0, DV)
    _all_same(got, want, "sigma NULL against the restatement", ("nbins", "v_lo", "v_hi", "vm"))
    # zero, negative, NaN at some levels, real widths at the others
    sig = cases.sigma_profile(nz, (8, 0, 1, 33), ncol, seed=3)
    none = np.array([0.0, -0.0, -1.5, float("nan"), float("-inf")])
    flat = sig.reshape(-1)
    idle = np.arange(flat.size) % 2 == 1
    flat[idle] = none[np.arange(idle.sum()) % none.size]
    got = _proc(gpu_mixed, x, sigma=sig)
    at = np.broadcast_to(idle.reshape(ncol, 1, nz), x.shape)
    _assert_same(got["spec"][at], x[at], "levels without a width: spec")
    for n in ("lost_below", "lost_above"):
        _assert_same(got[n][idle.reshape(ncol, nz)], np.zeros(int(idle.sum())), "levels without a width: " + n)
    if nv > 2:
        assert (ref.bits(got["spec"][~at]) != ref.bits(x[~at])).any()


# ---- 2. shift ----
@pytest.mark.parametrize("half, nv, shift", [(1, 25, 3), (8, 64, 7), (9, 64, 11), (16, 64, 9), (17, 64, 5), (33, 256, 5), (70, 256, 30)])
def test_a_shifted_spectrum_gives_shifted_outputs(gpu_mixed, half, nv, shift):
    nz, ncol = 65, 3
    lo, hi = half, nv - 1 - half - shift
    assert lo < hi
    a = cases.inside_spectrum(ncol, nv, nz, lo, hi, seed=half)
    b = np.zeros_like(a)
    b[:, shift:, :] = a[:, :nv - shift, :]
    sig = np.full(nz, cases.RATIOS[half] * DV)
    ga, gb = _proc(gpu_mixed, a, sigma=sig), _proc(gpu_mixed, b, sigma=sig)
    _assert_same(gb["spec"][:, shift:, :], ga["spec"][:, :nv - shift, :], "spec moved by %d bins" % shift)
    assert not gb["spec"][:, :shift, :].any() and not ga["spec"][:, nv - shift:, :].any()
    for n in ("lost_below", "lost_above"):
        assert not ga[n].any() and not gb[n].any(), n
    _assert_same(gb["nbins"], ga["nbins"], "nbins")
    _assert_same(gb["dbz"], ga["dbz"], "dbz")
    _assert_same(gb["v_lo"], ga["v_lo"] + shift * DV, "v_lo")        # the centres are multiples of 1/8: the sums are exact
    _assert_same(gb["v_hi"], ga["v_hi"] + shift * DV, "v_hi")
    assert (ga["nbins"] > 0).all()


# ---- 3. a unit bin returns the weight row ----
@pytest.mark.parametrize("nv, at", [(256, 128), (64, 31), (25, 0), (2, 1), (1, 0)])
def test_a_unit_bin_returns_the_weight_row(gpu_mixed, nv, at):
    halves = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 70, 255, 256, "cap")
    nz = len(halves)
    x = np.zeros((1, nv, nz))
    x[0, at, :] = 1.0
    sig = cases.sigma_profile(nz, halves)
    got = _proc(gpu_mixed, x, sigma=sig, want=("spec", "lost_below", "lost_above"))
    r = ref.process(x, V0, DV, sigma=sig, parts=True)
    H = r["H"][0]
    assert list(H) == [256 if h == "cap" else h for h in halves]
    worst = 0.0
    for k in range(nz):
        row = got["spec"][0, :, k]
        reach = np.abs(np.arange(nv) - at) <= H[k]
        assert not row[~reach].any() and (row[reach] >= 0).all(), (k, "support")
        if H[k] == 0:
            _assert_same(row, x[0, :, k], "H = 0")
        for d in range(1, min(at, nv - 1 - at, H[k]) + 1):
            assert ref.bits(row[at + d])[()] == ref.bits(row[at - d])[()], (k, d, "symmetry")
        worst = max(worst, np.abs(row - r["spec"][0, :, k]).max())       # the level's sum of the input is 1
    _seen("spec", worst / ULP, "unit bin nv %d" % nv)
    assert worst <= bound("spec")
    for n in ("lost_below", "lost_above"):
        e = np.abs(got[n] - r[n]).max()
        _seen(n, e / ULP, "unit bin nv %d" % nv)
        assert e <= bound(n)
    if nv == 256:
        assert not got["lost_below"][0, H <= 128].any() and (got["lost_below"][0, H > 128] > 0).all()


# ---- 4. against the restatement ----
RESTATED = [(65, 25, 3, (0, 1, 7, 8, 9, 33)), (120, 64, 5, (8, 32, 33, 70, 1)), (256, 256, 1, (0, 9, 31, 255, 256, "cap", 70)), (2, 2, 3, (1, 9)),
            (65, 1, 1, (0, 1, 33))]


@pytest.fixture(scope="module")
def restated():
    """name -> (inputs, restatement), computed once on the CPU and left unchanged."""
    out = {}
    for nz, nv, ncol, halves in RESTATED:
        x = cases.spectrum(ncol, nv, nz, seed=nz * nv)
        sig = cases.sigma_profile(nz, halves, ncol, seed=nv)
        noise = _noise_for(x)
        r = ref.process(x, V0, DV, sigma=sig, noise=noise, snr_min=1.5, parts=True)
        q = ref.process(x, V0, DV, sigma=sig, parts=True)
        out[(nz, nv, ncol)] = (x, sig, noise, r, q)
    return out


def _against(got, r, x, what):
    total = x.sum(axis=1)
    assert r["margin"] > 1e-9, (what, "a bin of the restatement sits on its detection threshold", r["margin"])
    for n in ("nbins", "v_lo", "v_hi"):
        _assert_same(got[n], r[n], what + " " + n)
    err = {"spec": (np.abs(got["spec"] - r["spec"]) / total[:, None, :]).max()}
    for n in ("lost_below", "lost_above"):
        err[n] = (np.abs(got[n] - r[n]) / total).max()
    err["dbz"] = np.abs(got["dbz"] - r["dbz"]).max() * np.log(10.0) / 10.0
    for n in ("vm", "sw"):
        err[n] = (np.abs(got[n] - r[n]) / np.maximum(np.abs(r[n]), DV)).max()
    for n in ("skew", "kurt"):
        err[n] = (np.abs(got[n] - r[n]) / np.maximum(np.abs(r[n]), 1.0)).max()
    for n, e in err.items():
        _seen(n, e / ULP, what)
    for n, e in err.items():
        assert e <= bound(n), (what, n, e / ULP)


@pytest.mark.parametrize("nz, nv, ncol", [c[:3] for c in RESTATED])
def test_against_the_restatement(gpu_mixed, restated, nz, nv, ncol):
    x, sig, noise, r, q = restated[(nz, nv, ncol)]
    got = _proc(gpu_mixed, x, sigma=sig, noise=noise, snr_min=1.5)
    _against(got, r, x, "nz %d nv %d noise" % (nz, nv))
    if nv > 2:
        assert (r["nbins"] < nv).any() and (r["nbins"] > 0).any()
    got = _proc(gpu_mixed, x, sigma=sig)
    _against(got, q, x, "nz %d nv %d quiet" % (nz, nv))
    assert (q["nbins"] == nv).all()                                    # the spectra are positive: without noise every bin is detected


# ---- 5. properties ----
@pytest.mark.parametrize("nz, nv, ncol", [c[:3] for c in RESTATED])
def test_conservation(gpu_mixed, restated, nz, nv, ncol):
    x, sig, _, _, _ = restated[(nz, nv, ncol)]
    got = _proc(gpu_mixed, x, sigma=sig, want=("spec", "lost_below", "lost_above"))
    total = x.sum(axis=1)
    e = (np.abs((got["spec"].sum(axis=1) + got["lost_below"] + got["lost_above"]) - total) / total).max()
    _seen("conservation", e / ULP, "nz %d nv %d" % (nz, nv))
    assert e <= bound("conservation")
    if nv >= 25:
        assert (got["lost_below"] > 0).any() and (got["lost_above"] > 0).any()


def test_variances_add(gpu_mixed):
    """A spectrum well inside the grid, no noise: sw**2 with sigma less sw**2 without is dv**2 times the discrete kernel's
    own variance sum d**2 g_d / G, the restatement's."""
    nz, nv, ncol = 65, 256, 3
    halves = (1, 7, 8, 9, 32, 33, 70)
    x = cases.inside_spectrum(ncol, nv, nz, 100, 150, seed=12)
    sig = cases.sigma_profile(nz, halves)
    wide, plain = _proc(gpu_mixed, x, sigma=sig, want=("sw", "lost_below", "lost_above", "nbins")), _proc(gpu_mixed, x, want=("sw", "nbins"))
    assert not wide["lost_below"].any() and not wide["lost_above"].any() and (plain["nbins"] == 51).all()
    s, H = ref.window(sig, 1.0 / DV, 4.0)
    g, G = ref.weights(s, H)
    K = DV * DV * ref.kernel_variance(g, G, H)
    assert np.array_equal(wide["nbins"], np.broadcast_to(51 + 2 * H, (ncol, nz)))
    e = (np.abs((wide["sw"] ** 2 - plain["sw"] ** 2) - K[None, :]) / K[None, :]).max()
    _seen("variance", e / ULP, "variances add")
    assert e <= bound("variance")


def test_noise_properties(gpu_mixed, restated):
    x, sig, noise, _, _ = restated[(120, 64, 5)]
    base = _proc(gpu_mixed, x, sigma=sig, noise=noise, snr_min=1.5)
    added = _proc(gpu_mixed, x, sigma=sig, noise=noise, snr_min=1.5, add_noise=True)
    _assert_same(added["spec"], base["spec"] + noise[:, None, :], "add_noise adds n_k to every bin")
    _all_same(added, base, "add_noise leaves the rest", [n for n in ref.NAMES if n != "spec"])
    last = base
    for snr in (3.0, 10.0, 40.0):
        more = _proc(gpu_mixed, x, sigma=sig, noise=noise, snr_min=snr)
        _assert_same(more["spec"], base["spec"], "snr_min does not touch the spectrum")
        assert (more["nbins"] <= last["nbins"]).all() and (more["nbins"] < last["nbins"]).any()
        assert (more["v_lo"][more["nbins"] > 0] >= last["v_lo"][more["nbins"] > 0]).all()
        assert (more["v_hi"][more["nbins"] > 0] <= last["v_hi"][more["nbins"] > 0]).all()
        last = more
    assert (last["nbins"] == 0).any()
    gone = last["nbins"] == 0
    for n in ("vm", "sw", "skew", "kurt", "v_lo", "v_hi"):
        _assert_same(last[n][gone], np.zeros(int(gone.sum())), "no detected bin: " + n)
    assert (last["dbz"][gone] == -40.0).all()
    for r in (base, last):
        some = r["nbins"] > 0
        assert (r["v_lo"][some] <= r["vm"][some]).all() and (r["vm"][some] <= r["v_hi"][some]).all()
    zero = _proc(gpu_mixed, x, sigma=sig, noise=noise, snr_min=0.0, want=("nbins",))
    assert (zero["nbins"] == 64).all()


def test_chain_with_doppler_spectrum_and_doppler_moments(gpu_mixed):
    """doppler_spectrum(total) -> spectrum_process without broadening and noise against doppler_moments, on three
    mixed-phase columns after one step: the gap is that of the linear deposit and of the diameter bins, and not larger than
    four times what the numpy restatements of the two existing operators give for the same comparison."""
    import torch
    import cases as col
    import doppler_ref as dref
    import doppler_spectrum_ref as sref
    from kid_amd import default_grid
    from oracle.oracle import Oracle
    m = gpu_mixed
    dev = {k: _cu(v) for k, v in col.config3(3).items()}
    ppt = torch.zeros(3, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)
    st = {k: dev[k] for k in sref.INPUTS}
    v0, dv, nv = -1.0, 0.0625, 256
    sp = m.doppler_spectrum(st, v0, dv, nv, want=("total", "below", "above"))
    got = m.spectrum_process(sp["total"], v0, dv, want=("dbz", "vm", "sw", "nbins"))
    mom = m.doppler_moments(st, want=("dbz", "vd", "sw"))
    torch.cuda.synchronize()
    got, mom = {k: v.cpu().numpy() for k, v in got.items()}, {k: v.cpu().numpy() for k, v in mom.items()}
    host = {k: v.cpu().numpy() for k, v in st.items()}
    o = Oracle(iiwarm=True)
    c = dref.constants(o)
    o.close()
    grids = {x: default_grid(m, x) for x in sref.SPECIES}
    rs = sref.doppler_spectrum(c, host, v0, dv, nv, default=grids, want=("total", "below", "above"))
    rp = ref.process(rs["total"], v0, dv)
    rm = dref.doppler_moments(c, host)
    echo = (rp["nbins"] > 0) & (rm["present_r"] | rm["present_s"] | rm["present_g"]) & (rs["below"] == 0) & (rs["above"] <= 1e-12 * rs["total"].sum(axis=1))
    echo = echo & (got["nbins"] > 0)
    assert echo.sum() >= 10
    pairs = (("dbz", "dbz", "dB"), ("vm", "vd", "m/s"), ("sw", "sw", "m/s"))
    for a, b, unit in pairs:
        dev_gap, ref_gap = np.abs(got[a] - mom[b])[echo].max(), np.abs(rp[a] - rm[b])[echo].max()
        print("measured chain: |%s - doppler_moments' %s| at most %.3e %s on the device, %.3e in the restatements" % (a, b, dev_gap, unit, ref_gap))
        assert dev_gap <= 4.0 * ref_gap, (a, dev_gap, ref_gap)


# ---- 6. invariance: every one an equality of bits ----
def test_bits_do_not_depend_on_batch_position_request_repeat_out_or_stride(gpu_mixed, restated):
    import torch
    from kid_amd import SpecCfg
    m = gpu_mixed
    x, sig, noise, _, _ = restated[(120, 64, 5)]
    kw = dict(snr_min=1.5)
    full = _proc(m, x, sigma=sig, noise=noise, **kw)
    _all_same(_proc(m, x, sigma=sig, noise=noise, **kw), full, "repeat")
    for c in (0, 3, 4):
        alone = _proc(m, x[c:c + 1], sigma=sig[c:c + 1], noise=noise[c:c + 1], **kw)
        for n in ref.NAMES:
            _assert_same(alone[n][0], full[n][c], "column %d alone: %s" % (c, n))
    back = _proc(m, x[::-1], sigma=sig[::-1], noise=noise[::-1], **kw)
    for n in ref.NAMES:
        _assert_same(back[n][::-1], full[n], "columns reversed: " + n)
    for sub in [(n,) for n in ref.NAMES] + [("spec", "nbins"), ("lost_above", "sw"), ("vm", "v_hi", "dbz"), ("lost_below", "spec", "kurt")]:
        part = _proc(m, x, sigma=sig, noise=noise, want=sub, **kw)
        assert sorted(part) == sorted(sub)
        _all_same(part, full, "subset %s" % (sub,), sub)
    # [nz] against [ncol, nz]: every column takes column 0's width and noise
    shared = _proc(m, x, sigma=sig[0], noise=noise[0], **kw)
    tiled = _proc(m, x, sigma=np.tile(sig[0], (5, 1)), noise=np.tile(noise[0], (5, 1)), **kw)
    _all_same(shared, tiled, "[nz] against [ncol, nz]")
    mixed = _proc(m, x, sigma=sig[0], noise=np.tile(noise[0], (5, 1)), **kw)
    _all_same(mixed, tiled, "sigma [nz] with noise [ncol, nz]")
    # out= rewrites an earlier result in place
    dx, ds, dn, cfg = _cu(x), _cu(sig), _cu(noise), SpecCfg(**kw)
    first = m.spectrum_process(dx, V0, DV, ds, dn, cfg, ref.NAMES)
    ptrs = {n: t.data_ptr() for n, t in first.items()}
    for t in first.values():
        t.fill_(7)
    before = torch.cuda.memory_allocated()
    second = m.spectrum_process(dx, V0, DV, ds, dn, cfg, ref.NAMES, out=first)
    assert torch.cuda.memory_allocated() == before
    torch.cuda.synchronize()
    assert all(second[n] is first[n] for n in ref.NAMES) and {n: t.data_ptr() for n, t in second.items()} == ptrs
    _all_same({n: t.cpu().numpy() for n, t in second.items()}, full, "out=")


def test_the_middle_of_a_nan_filled_tensor(gpu_mixed, restated):
    """Every output lives in the middle of a NaN-filled (nbins: -7-filled) buffer; the guard zones are intact afterwards."""
    import torch
    from kid_amd import SpecCfg
    x, sig, noise, _, _ = restated[(65, 25, 3)]
    ncol, nv, nz, pad = 3, 25, 65, 4096
    want = _proc(gpu_mixed, x, sigma=sig, noise=noise)
    bufs, out = {}, {}
    for name in ref.NAMES:
        n = ncol * nz * (nv if name == "spec" else 1)
        if name == "nbins":
            bufs[name] = torch.full((n + 2 * pad,), -7, dtype=torch.int32, device="cuda:0")
        else:
            bufs[name] = torch.full((n + 2 * pad,), float("nan"), dtype=torch.float64, device="cuda:0")
        out[name] = bufs[name][pad:pad + n].view((ncol, nv, nz) if name == "spec" else (ncol, nz))
    gpu_mixed.spectrum_process(_cu(x), V0, DV, _cu(sig), _cu(noise), SpecCfg(), ref.NAMES, out=out)
    torch.cuda.synchronize()
    for name in ref.NAMES:
        b = bufs[name].cpu().numpy()
        n = b.size - 2 * pad
        guard = np.concatenate([b[:pad], b[pad + n:]])
        assert (guard == -7).all() if name == "nbins" else (ref.bits(guard) == ref.bits(np.float64("nan"))[()]).all(), name
        _assert_same(b[pad:pad + n].reshape(want[name].shape), want[name], "guarded " + name)


def test_non_finite_values_are_memory_safe(gpu_mixed, restated):
    """NaN and infinite spectrum, sigma and noise values: the call completes, the levels that hold none of them keep their
    bits, and the guard zones around spec stay intact."""
    import torch
    from kid_amd import SpecCfg
    x, sig, noise, _, _ = restated[(65, 25, 3)]
    clean = _proc(gpu_mixed, x, sigma=sig, noise=noise)
    nan, inf = float("nan"), float("inf")
    bx, bs, bn = x.copy(), sig.copy(), noise.copy()
    bx[0, 5, 1], bx[1, 0, 3], bx[2, 24, 5] = nan, inf, -inf
    bs[0, 7], bs[1, 9], bs[2, 11] = inf, nan, 1e300
    bn[0, 13], bn[1, 15] = nan, inf
    dirty = np.zeros((3, 65), dtype=bool)
    for c, k in ((0, 1), (1, 3), (2, 5), (0, 7), (1, 9), (2, 11), (0, 13), (1, 15)):
        dirty[c, k] = True
    pad, n = 4096, x.size
    buf = torch.full((n + 2 * pad,), -7.0, dtype=torch.float64, device="cuda:0")
    out = {"spec": buf[pad:pad + n].view(3, 25, 65)}
    got = gpu_mixed.spectrum_process(_cu(bx), V0, DV, _cu(bs), _cu(bn), SpecCfg(), ref.NAMES, out=out)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    b = buf.cpu().numpy()
    assert (b[:pad] == -7).all() and (b[pad + n:] == -7).all()
    for name in ref.NAMES:
        keep = np.broadcast_to(~dirty[:, None, :], x.shape) if name == "spec" else ~dirty
        _assert_same(got[name][keep], clean[name][keep], "levels without a non-finite value: " + name)
    assert (got["nbins"] >= 0).all() and (got["nbins"] <= 25).all()


@pytest.mark.parametrize("nz, nv, ncol", [(65, 25, 3), (120, 64, 5)])
def test_binary32_entry_rounds_once(gpu_mixed, restated, nz, nv, ncol):
    x, sig, noise, _, _ = restated[(nz, nv, ncol)]
    x32, s32, n32 = x.astype(np.float32), sig.astype(np.float32), noise.astype(np.float32)
    for add in (False, True):
        wide = _proc(gpu_mixed, x32.astype(np.float64), sigma=s32.astype(np.float64), noise=n32.astype(np.float64), snr_min=1.5, add_noise=add)
        narrow = _proc(gpu_mixed, x32, sigma=s32, noise=n32, snr_min=1.5, add_noise=add)
        for n in ref.NAMES:
            _assert_same(narrow[n], wide[n] if n == "nbins" else wide[n].astype(np.float32), "binary32 " + n)
    assert (wide["nbins"] > 0).any()


def test_hip_graph_replay_of_one_captured_launch(gpu_mixed, restated):
    import torch
    sp = _sp()
    m, L = gpu_mixed, sp.library()
    x, sig, noise, _, _ = restated[(120, 64, 5)]
    eager = _proc(m, x, sigma=sig, noise=noise, snr_min=1.5)
    dx, ds, dn = _cu(x), _cu(sig), _cu(noise)
    out = {n: torch.full(eager[n].shape, -7, dtype=torch.int32 if n == "nbins" else torch.float64, device="cuda:0") for n in ref.NAMES}
    o = sp._SpecOut(**{n: t.data_ptr() for n, t in out.items()})
    cfg = sp._SpecCfg(4.0, 1.5, 0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = L.kidmp_spectrum_process_device(m._h, 5, 120, dx.data_ptr(), V0, DV, 64, ds.data_ptr(), 120, dn.data_ptr(), 120, C.byref(cfg), C.byref(o),
                                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    for _ in range(2):
        for t in out.values():
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        _all_same({n: t.cpu().numpy() for n, t in out.items()}, eager, "replay")


# ---- 7. refusals ----
def test_refusals_write_nothing(gpu_mixed):
    import torch
    sp = _sp()
    L = sp.library()
    ncol, nv, nz = 3, 16, 12
    spec = torch.ones(ncol, nv, nz, dtype=torch.float64, device="cuda:0")
    prof = torch.full((ncol, nz), 0.3, dtype=torch.float64, device="cuda:0")
    big = torch.full((ncol, nv, nz), -7.0, dtype=torch.float64, device="cuda:0")
    val = torch.full((ncol, nz), -7.0, dtype=torch.float64, device="cuda:0")
    cnt = torch.full((ncol, nz), -7, dtype=torch.int32, device="cuda:0")
    host = torch.zeros(ncol * nv * nz, dtype=torch.float64)
    nan, inf = float("nan"), float("inf")

    def call(m=gpu_mixed, ncol=ncol, nz=nz, nv=nv, v0=-1.0, dv=0.25, spec=spec.data_ptr(), sigma=prof.data_ptr(), ss=nz, noise=prof.data_ptr(), ns=nz,
             cut=4.0, snr_min=1.0, names=("spec", "vm", "nbins"), cfg=True, outp=True, fn=L.kidmp_spectrum_process_device, **over):
        o = sp._SpecOut(**{n: over.get(n, (big if n == "spec" else cnt if n == "nbins" else val).data_ptr()) for n in names})
        return fn(m._h if m is not None else None, ncol, nz, spec, v0, dv, nv, sigma, ss, noise, ns,
                  C.byref(sp._SpecCfg(cut, snr_min, 0)) if cfg else None, C.byref(o) if outp else None, None)

    refused = [dict(spec=None), dict(nz=1), dict(nz=257), dict(ncol=-1), dict(ncol=2 ** 31), dict(nv=0), dict(nv=257), dict(nv=-1), dict(dv=0.0),
               dict(dv=-0.25), dict(dv=nan), dict(dv=inf), dict(dv=1e-320), dict(v0=nan), dict(v0=inf), dict(cut=0.0), dict(cut=-4.0), dict(cut=nan),
               dict(cut=inf), dict(snr_min=-1.0), dict(snr_min=nan), dict(snr_min=inf), dict(ss=1), dict(ss=-nz), dict(ss=nz + 1), dict(ns=5),
               dict(ns=2 * nz), dict(cfg=False), dict(outp=False), dict(names=()), dict(spec=host.data_ptr()), dict(sigma=host.data_ptr()),
               dict(noise=host.data_ptr()), dict(names=("vm",), vm=host.data_ptr()), dict(names=("nbins",), nbins=host.data_ptr())]
    for kw in refused:
        for fn in (L.kidmp_spectrum_process_device, L.kidmp32_spectrum_process_device):
            assert call(fn=fn, **kw) == -1, kw
            assert L.kidmp_last_error(gpu_mixed._h), kw
    assert call(m=None) == -5 and call(ncol=0) == 0 and call(ncol=0, spec=None) == 0
    torch.cuda.synchronize()
    assert (big.cpu().numpy() == -7).all() and (val.cpu().numpy() == -7).all() and (cnt.cpu().numpy() == -7).all()
    assert call() == 0 and call(sigma=None, ss=0, noise=None, ns=0, names=("dbz",)) == 0 and call(sigma=prof.data_ptr(), ss=0, names=("lost_below",)) == 0
    torch.cuda.synchronize()
    assert np.isfinite(big.cpu().numpy()).all() and (cnt.cpu().numpy() >= 0).all() and np.isfinite(val.cpu().numpy()).all()
    from kid_amd import KidmpError, SpecCfg
    with pytest.raises(KidmpError, match="cut"):
        gpu_mixed.spectrum_process(spec, -1.0, 0.25, cfg=SpecCfg(cut=0.0))
    with pytest.raises(KidmpError, match="sigma"):
        gpu_mixed.spectrum_process(spec, -1.0, 0.25, sigma=prof[:, :5].contiguous())
