"""The KiD adapter on the device (kidmp[32]_kid_interface_*, ThompsonMP.kid_interface / kid_interface_host).  -m gpu.

A bitwise chain reduces the adapter's correctness to the step's, which the rest of the suite holds against the oracle:
  gather    the workspace after the gather alone equals the expressions of W:46-97 formed in numpy, operation by operation
            in the arrays' format, for every profile except p; p is held to an ulp bound (binary64: 4 ulp of
            numpy.longdouble; binary32: 1 ulp of the specified formation in numpy); the default aerosols equal default_aerosols
            on the gathered arrays
  step      batch_step on a copy of the gathered workspace gives the post-step workspace, ppt, rates and nstep of the call
  back-out  every tendency equals the expressions of W:198-245 formed in numpy from the post-step workspace and the inputs
Then: the oracle's adapter (warm, the metric and bound of test_fortran_gpu._check_mphys), parity.assert_parity of the
post-step state (mixed phase), KAT-B over 360 resident calls, a captured hipGraph, the host entry, the refusals."""
import ctypes as C

import numpy as np
import pytest

import cases
import kat_cases as kc
from parity import assert_parity

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
P0, R_ON_CP, DT = 1.0e5, 287.058 / 1005.0, 10.0           # kat_b's Exner recipe
WARM = ("theta", "qv", "qc", "qr", "nr")
FROZEN = ("qi", "ni", "qs", "qg")
FIELDS = WARM + FROZEN
STATE = ("qv", "qc", "qi", "qr", "qs", "qg", "ni", "nr", "nc", "nwfa", "nifa", "t")
HYD = (("qc", 0, 0), ("qr", 1, 0), ("nr", 1, 1), ("qi", 2, 0), ("ni", 2, 1), ("qs", 3, 0), ("qg", 4, 0))   # KiD species, moment
SHAPES = [("warm", 120, 301), ("warm", 37, 203), ("warm", 200, 203), ("mixed", 120, 301), ("mixed", 37, 203), ("mixed", 200, 203)]
IDS = ["%s-nz%d" % (k, nz) for k, nz, _ in SHAPES]


@pytest.fixture
def ctxs(gpu_warm, gpu_mixed):
    yield {"warm": gpu_warm, "mixed": gpu_mixed}
    for m in (gpu_warm, gpu_mixed):
        m.set_column_nc(None)
        m.set_host_chunk(0)


# ---- inputs: columns of tests/cases.py in theta-form, with a smooth forcing ----
def _resample(st, nz):
    ncol, nz0 = st["qv"].shape
    x0, x1 = np.linspace(0.0, 1.0, nz0), np.linspace(0.0, 1.0, nz)
    out = {k: np.stack([np.interp(x1, x0, v[c]) for c in range(ncol)]) for k, v in st.items()}
    out["dz"] = np.full((ncol, nz), float(st["dz"][0].sum()) / nz)
    return out


def _columns(kind, ncol, nz):
    rng = np.random.Generator(np.random.PCG64(cases.SEED + 11))
    if kind == "warm":
        st = cases.config2(ncol)
        for k in ("qc", "qr", "nr"):
            st[k] *= rng.lognormal(0.0, 0.3, size=(ncol, 1))
    else:
        edge = cases.edge_cases()
        n5 = ncol // 4
        parts = [cases.config3(ncol - n5 - edge["qv"].shape[0], seed=cases.SEED + 11), cases.config5(n5, seed=cases.SEED + 12), edge]
        st = {k: np.concatenate([p[k] for p in parts]) for k in cases.KEYS}
    if nz != cases.NZ:
        st = _resample(st, nz)
    return {k: np.ascontiguousarray(v) for k, v in st.items()}


def _inputs(kind, ncol, nz, dtype=f64, forcing=True):
    """KiD's fields of the columns, the forcing dicts, exner and the ONE dz profile, all of `dtype`."""
    st = _columns(kind, ncol, nz)
    exner = (st["p"] / P0) ** R_ON_CP
    F = {k: st[k] for k in FIELDS[1:]}
    F["theta"] = st["t"] / exner
    x = np.linspace(0.0, 1.0, nz)[None, :]
    c = np.arange(ncol)[:, None]
    wave = np.sin(2.0 * np.pi * (1.5 * x + 0.013 * c))
    adv, div = {}, {}
    for k in FIELDS:
        eps = 1e-2 if k in ("nr", "ni") else 1e-9            # a source where the field itself is empty
        adv[k] = 1e-4 * F[k] * wave + eps * (1.0 + wave)
        div[k] = -2e-5 * F[k]                                # a small sink
    adv["theta"] = 2e-3 * wave + 0.0 * F["theta"]
    div["theta"] = -1e-4 * np.cos(2.0 * np.pi * x) + 0.0 * F["theta"]
    cast = lambda d: {k: np.ascontiguousarray(v.astype(dtype)) for k, v in d.items()}   # noqa: E731
    F, adv, div = cast(F), cast(adv), cast(div)
    if not forcing:
        adv, div = None, None
    return F, adv, div, np.ascontiguousarray(exner.astype(dtype)), np.ascontiguousarray(st["dz"][0].astype(dtype))


def _dev(d):
    import torch
    if d is None:
        return None
    if isinstance(d, dict):
        return {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    return torch.from_numpy(d).cuda()


def _views(m, work, ncol, nz, dtype):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in m.kid_workspace_views(work, ncol, nz, dtype).items()}


def _keys(kind):
    return WARM if kind == "warm" else FIELDS


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == f64 else np.uint32 if a.dtype == f32 else a.dtype)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    diff = _bits(a) != _bits(b)
    assert not diff.any(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        what, int(diff.sum()), diff.size, np.argwhere(diff)[0], a[tuple(np.argwhere(diff)[0])], b[tuple(np.argwhere(diff)[0])])


# ---- the expressions of the issue in numpy, every operation rounded in the arrays' format ----
def _np_gather(kind, F, adv, div, exner, dz, dt):
    T = exner.dtype.type
    zero = np.zeros_like(exner)
    g = {}
    for k in _keys(kind):
        a = zero if adv is None or adv.get(k) is None else adv[k]
        d = zero if div is None or div.get(k) is None else div[k]
        g[k] = F[k] + (a + d) * T(dt)
        assert g[k].dtype == exner.dtype
    out = {k: g[k] for k in _keys(kind)[1:]}
    out["t"] = g["theta"] * exner
    for k in FROZEN:
        out.setdefault(k, zero.copy())
    out["w"] = zero.copy()
    out["dz"] = np.ascontiguousarray(np.broadcast_to(dz, exner.shape))
    return out


def _np_aerosols(t, qv, p, nt_c):
    """M:958-964 as k_default_aerosols writes them; nt_c [ncol, 1] or scalar, already in the arrays' format."""
    T = t.dtype.type
    rho = T(0.622) * p / (T(287.04) * t * (qv + T(0.622)))
    return nt_c / rho, T(11.1e6) / rho, T(0.5e6) * T(0.01) / rho


def _np_backout(kind, F, adv, div, exner, post, dt):
    T = exner.dtype.type
    zero = np.zeros_like(exner)
    out = {}
    for k in _keys(kind):
        a = zero if adv is None or adv.get(k) is None else adv[k]
        d = zero if div is None or div.get(k) is None else div[k]
        x1 = post["t"] / exner if k == "theta" else post[k]
        out[k] = (x1 - F[k]) / T(dt) - (a + d)
    return out


def _ulps(a, ref):
    return np.abs(a.astype(np.longdouble) - ref.astype(np.longdouble)) / np.spacing(np.abs(ref).astype(a.dtype)).astype(np.longdouble)


def _p_ulps(p, exner):
    """Distance of p from its reference, in ulps of the arrays' format; the exponent e = 1/r_on_cp is rounded there.
    binary64: p0 * exner**e formed in numpy.longdouble.
    binary32: the formation include/kidmp.h specifies, in numpy operations: the correctly rounded powf (numpy's binary64
    power of the widened operands, rounded once to binary32), then the product with p0 in binary32.  numpy's own float32
    `**` is not that function: on these inputs it is 0.86 ulp from the exact power where the correctly rounded one is
    0.50, and p formed with it lies up to 2.0 ulp from the library's p (measured, MI355X; printed below).  Against the
    exact p0 * exner**e both carry the two roundings of the formation: 1.22 ulp (specified) and 1.47 ulp (numpy's)."""
    T = exner.dtype.type
    e = T(1) / T(R_ON_CP)
    exact = np.longdouble(T(P0)) * np.power(exner.astype(np.longdouble), np.longdouble(e))
    if T is f64:
        return _ulps(p, exact)
    ref = T(P0) * np.power(exner.astype(f64), f64(e)).astype(f32)
    assert ref.dtype == f32
    print("binary32 p: %.3f ulp from numpy's own float32 power and product, %.3f ulp from the exact value"
          % (_ulps(p, T(P0) * np.power(exner, e)).max(), _ulps(p, exact).max()))
    return _ulps(p, ref)


# ---- gather ----
@pytest.mark.parametrize("kind,nz,ncol", SHAPES, ids=IDS)
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
def test_gather_fills_the_workspace_with_the_reference_expressions(ctxs, kind, nz, ncol, dtype):
    m = ctxs[kind]
    F, adv, div, exner, dz = _inputs(kind, ncol, nz, dtype)
    g = m.kid_interface(_dev(F), DT, P0, R_ON_CP, _dev(exner), _dev(dz), adv=_dev(adv), div=_dev(div), gather_only=True)
    ws = _views(m, g["work"], ncol, nz, dtype)
    want = _np_gather(kind, F, adv, div, exner, dz, DT)
    for k in ("qv", "qc", "qr", "nr", "qi", "ni", "qs", "qg", "t", "w", "dz"):
        _same(ws[k], want[k], "gathered " + k)
    if kind == "warm":
        for k in FROZEN:
            assert not _bits(ws[k]).any(), k                  # exact (positive) zeros, W:46-52
    assert not _bits(g["ppt"].cpu().numpy()).any()            # W:55-58
    ulps = _p_ulps(ws["p"], exner)
    print("p: max %.3f ulp of the reference, %d of %d levels differ from it" % (ulps.max(), int((ulps > 0).sum()), ulps.size))
    assert ulps.max() <= (4.0 if dtype == f64 else 1.0)
    nc, nwfa, nifa = _np_aerosols(ws["t"], ws["qv"], ws["p"], dtype(1.0e8))
    for k, w in (("nc", nc), ("nwfa", nwfa), ("nifa", nifa)):
        _same(ws[k], w, "default " + k)
    if dtype == f64:
        import torch
        d = m.default_aerosols(*[torch.from_numpy(ws[k]).cuda() for k in ("qv", "t", "p")])
        for k, w in zip(("nc", "nwfa", "nifa"), d):
            _same(ws[k], w.cpu().numpy(), "default_aerosols " + k)


@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
def test_gather_honours_a_bound_droplet_number(ctxs, dtype):
    import torch
    kind, nz, ncol = "mixed", 120, 301
    m = ctxs[kind]
    values = np.array([(25.0, 100.0, 300.0, 1000.0)[c % 4] for c in range(ncol)])
    m.set_column_nc(values)
    F, adv, div, exner, dz = _inputs(kind, ncol, nz, dtype)
    g = m.kid_interface(_dev(F), DT, P0, R_ON_CP, _dev(exner), _dev(dz), adv=_dev(adv), div=_dev(div), gather_only=True)
    ws = _views(m, g["work"], ncol, nz, dtype)
    nt_c = (values * 1.0e6).astype(dtype)[:, None]
    nc, nwfa, nifa = _np_aerosols(ws["t"], ws["qv"], ws["p"], nt_c)
    for k, w in (("nc", nc), ("nwfa", nwfa), ("nifa", nifa)):
        _same(ws[k], w, "default " + k)
    if dtype == f64:
        d = m.default_aerosols(*[torch.from_numpy(ws[k]).cuda() for k in ("qv", "t", "p")])
        for k, w in zip(("nc", "nwfa", "nifa"), d):
            _same(ws[k], w.cpu().numpy(), "default_aerosols " + k)


# ---- step and back-out ----
def _call(m, F, adv, div, exner, dz, arith=None, **kw):
    """One full call; everything that comes back, as numpy, plus the post-step workspace under 'post'."""
    import torch
    ncol, nz = exner.shape
    rates = torch.zeros(ncol, 36, nz, dtype=torch.float64, device="cuda")
    nstep = torch.zeros(ncol, 4, dtype=torch.int32, device="cuda")
    r = m.kid_interface(_dev(F), DT, P0, R_ON_CP, _dev(exner), _dev(dz), adv=_dev(adv), div=_dev(div), rates=rates, nstep=nstep,
                        arith=arith, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in r.items() if k in FIELDS + ("ppt", "dbz")}
    if "radii" in r:
        out["radii"] = [a.cpu().numpy() for a in r["radii"]]
    out["rates"], out["nstep"] = rates.cpu().numpy(), nstep.cpu().numpy()
    out["post"] = _views(m, r["work"], ncol, nz, exner.dtype)
    out["work"] = r["work"]
    return out


def _chain(m, kind, nz, ncol, dtype, arith):
    import torch
    F, adv, div, exner, dz = _inputs(kind, ncol, nz, dtype)
    g = m.kid_interface(_dev(F), DT, P0, R_ON_CP, _dev(exner), _dev(dz), adv=_dev(adv), div=_dev(div), gather_only=True)
    torch.cuda.synchronize()
    st = {k: v.clone() for k, v in m.kid_workspace_views(g["work"], ncol, nz, dtype).items()}
    ppt = torch.zeros(ncol, 4, dtype=st["qv"].dtype, device="cuda")
    rates = torch.zeros(ncol, 36, nz, dtype=torch.float64, device="cuda")
    nstep = torch.zeros(ncol, 4, dtype=torch.int32, device="cuda")
    if dtype == f64:
        m.batch_step(st, DT, ppt, rates=rates, nstep=nstep)
    else:
        m.batch_step32(st, DT, ppt, arith=arith, rates=rates, nstep=nstep)
    torch.cuda.synchronize()
    got = _call(m, F, adv, div, exner, dz, arith=arith)
    for k in STATE + ("p", "w", "dz"):
        _same(got["post"][k], st[k].cpu().numpy(), "post-step " + k)
    _same(got["ppt"], ppt.cpu().numpy(), "ppt")
    _same(got["rates"], rates.cpu().numpy(), "rates")
    _same(got["nstep"], nstep.cpu().numpy(), "nstep")
    assert got["nstep"].any() and np.abs(got["rates"]).max() > 0       # the step ran
    want = _np_backout(kind, F, adv, div, exner, got["post"], DT)
    for k in _keys(kind):
        _same(got[k], want[k], "tendency of " + k)
    return got


@pytest.mark.parametrize("kind,nz,ncol", SHAPES, ids=IDS)
def test_step_and_back_out_binary64(ctxs, kind, nz, ncol):
    got = _chain(ctxs[kind], kind, nz, ncol, f64, None)
    if kind == "warm":
        assert set(got) & set(FROZEN) == set()               # no frozen tendency out of a warm context


@pytest.mark.parametrize("arith", ["p32n", "f32"])
@pytest.mark.parametrize("kind,nz,ncol", SHAPES, ids=IDS)
def test_step_and_back_out_binary32(ctxs, kind, nz, ncol, arith):
    _chain(ctxs[kind], kind, nz, ncol, f32, arith)


@pytest.mark.parametrize("kind", ["warm", "mixed"])
def test_step_with_a_bound_droplet_number(ctxs, kind):
    m = ctxs[kind]
    ncol = 301
    plain = _chain(m, kind, 120, ncol, f64, None)
    m.set_column_nc(np.array([(25.0, 100.0, 300.0, 1000.0)[c % 4] for c in range(ncol)]))
    bound = _chain(m, kind, 120, ncol, f64, None)
    assert not np.array_equal(plain["qc"], bound["qc"])      # the binding acts (autoconversion depends on Nt_c)
    _same(plain["qc"][1::4], bound["qc"][1::4], "the columns bound to the context's own 100 cm**-3")


# ---- forcing ----
@pytest.mark.parametrize("kind", ["warm", "mixed"])
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
def test_absent_forcing_is_a_zero_operand(ctxs, kind, dtype):
    m = ctxs[kind]
    ncol, nz = 203, 120
    F, adv, div, exner, dz = _inputs(kind, ncol, nz, dtype)
    zeros = {k: np.zeros_like(exner) for k in FIELDS}
    keys = _keys(kind) + ("ppt",)
    full = _call(m, F, adv, div, exner, dz)

    def same(a, b, what):
        for k in keys:
            _same(a[k], b[k], "%s: %s" % (what, k))
        for k in STATE:
            _same(a["post"][k], b["post"][k], "%s: post-step %s" % (what, k))
    same(_call(m, F, None, None, exner, dz), _call(m, F, zeros, zeros, exner, dz), "no forcing")
    same(_call(m, F, adv, None, exner, dz), _call(m, F, adv, zeros, exner, dz), "adv only")
    same(_call(m, F, None, div, exner, dz), _call(m, F, zeros, div, exner, dz), "div only")
    part = {k: v for k, v in adv.items() if k not in ("qv", "nr")}
    same(_call(m, F, part, div, exner, dz), _call(m, F, dict(part, qv=zeros["qv"], nr=zeros["nr"]), div, exner, dz), "members missing")
    same(_call(m, F, {}, {"theta": div["theta"]}, exner, dz),
         _call(m, F, zeros, dict(zeros, theta=div["theta"]), exner, dz), "one member present")
    none = _call(m, F, None, None, exner, dz)
    for k in _keys(kind):                                    # the forcing is not inert
        assert not np.array_equal(full[k], none[k]), k


# ---- outputs ----
@pytest.mark.parametrize("kind", ["warm", "mixed"])
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
def test_outputs_are_those_of_the_post_step_workspace(ctxs, kind, dtype):
    import torch
    m = ctxs[kind]
    ncol, nz = 203, 120
    F, adv, div, exner, dz = _inputs(kind, ncol, nz, dtype)
    plain = _call(m, F, adv, div, exner, dz)
    got = _call(m, F, adv, div, exner, dz, dbz=True, radii=True)
    for k in _keys(kind) + ("ppt",):
        _same(got[k], plain[k], k)                           # asking for outputs changes nothing else
    st = {k: torch.from_numpy(got["post"][k]).cuda() for k in m.OUTPUT_NAMES}
    dbz, radii = m.column_outputs(st)
    _same(got["dbz"], dbz.cpu().numpy(), "dbz")
    for a, b, k in zip(got["radii"], radii, ("re_qc", "re_qi", "re_qs")):
        _same(a, b.cpu().numpy(), k)
    only = _call(m, F, adv, div, exner, dz, dbz=True)
    _same(only["dbz"], got["dbz"], "dbz alone")


# ---- against the oracle ----
def _oracle_adapter(oracle, F, adv, div, exner, dz):
    nx, nz = exner.shape
    z = np.zeros((nx, nz))
    hy, ha, hd = (np.zeros((2, 5, nx, nz)) for _ in range(3))
    for k, ih, im in HYD:
        hy[im, ih], ha[im, ih], hd[im, ih] = F[k], adv.get(k, z), div.get(k, z)
    dth, dqv, dhy, ppt = oracle.kid_interface(nz, nx, DT, P0, R_ON_CP, F["theta"].ravel(), adv["theta"].ravel(), div["theta"].ravel(),
                                              exner.ravel(), dz.copy(), F["qv"].ravel(), adv["qv"].ravel(), div["qv"].ravel(),
                                              hy.ravel(), ha.ravel(), hd.ravel())
    dhy = dhy.reshape(2, 5, nx, nz)
    out = {"theta": dth.reshape(nx, nz), "qv": dqv.reshape(nx, nz)}
    out.update({k: dhy[im, ih] for k, ih, im in HYD})
    return out


def test_warm_tendencies_match_the_oracle_adapter(ctxs, oracle_warm):
    """The metric and bound of tests/test_fortran_gpu.py::_check_mphys: relative error below 1e-9, measured against
    max(|reference|, 1e-5 * max|state| / 10) -- a few ulp of state / dt."""
    ncol, nz = 61, 120
    F, adv, div, exner, dz = _inputs("warm", ncol, nz)
    got = _call(ctxs["warm"], F, adv, div, exner, dz)
    want = _oracle_adapter(oracle_warm, F, adv, div, exner, dz)
    worst = {}
    for k in WARM:
        scale = max(np.abs(F[k]).max() / 10.0, 1e-300)
        err = np.abs(got[k] - want[k]) / np.maximum(np.abs(want[k]), 1e-5 * scale)
        worst[k] = float(err.max())
    print("warm adapter vs oracle, worst relative error per field:", worst)
    assert np.abs(want["qc"]).max() > 0 and np.abs(want["qr"]).max() > 0
    for k in WARM:
        assert worst[k] < 1e-9, (k, worst)


def test_mixed_phase_post_step_state_meets_parity(ctxs, oracle_mixed):
    ncol, nz = 101, 120
    F, adv, div, exner, dz = _inputs("mixed", ncol, nz)
    m = ctxs["mixed"]
    g = m.kid_interface(_dev(F), DT, P0, R_ON_CP, _dev(exner), _dev(dz), adv=_dev(adv), div=_dev(div), gather_only=True)
    st = _views(m, g["work"], ncol, nz, f64)                 # the oracle steps from the gathered inputs
    got = _call(m, F, adv, div, exner, dz)
    v = assert_parity(oracle_mixed, st, DT, got["post"], got["ppt"])
    print("mixed-phase adapter, post-step state vs oracle:", v)


# ---- KAT-B resident on the device ----
def test_kat_b_360_resident_calls(ctxs):
    """SURVEY 9h KAT-B: the reference's recorded end state, to the seven digits tests/test_oracle_kat.py asserts."""
    import torch
    c = kc.kat_b()
    nz = c["nz"]
    F = {"theta": c["theta"], "qv": c["qv"], "qc": c["hydro"][0, 0, 0], "qr": c["hydro"][0, 1, 0], "nr": c["hydro"][1, 1, 0]}
    F = {k: torch.from_numpy(np.ascontiguousarray(v.reshape(1, nz))).cuda() for k, v in F.items()}
    exner, dz = torch.from_numpy(c["exner"].reshape(1, nz).copy()).cuda(), torch.from_numpy(c["dz"].copy()).cuda()
    m = ctxs["warm"]
    work, out = m.kid_workspace(1, nz, f64), None
    for _ in range(360):
        out = m.kid_interface(F, c["dt"], c["p0"], c["r_on_cp"], exner, dz, work=work, out=out)
        for k in WARM:
            F[k] += out[k] * c["dt"]                          # a multiply, then an add
    torch.cuda.synchronize()
    got = [float(F[k].cpu().numpy().sum()) for k in ("qv", "qc", "qr", "nr")]
    print("KAT-B resident:", got)
    for g, r in zip(got, (1.530434, 2.218719e-2, 2.694135e-3, 1.060568e6)):
        assert abs(g / r - 1.0) < 1.0e-6, (got, r)


# ---- hipGraph ----
@pytest.mark.parametrize("kind", ["warm", "mixed"])
def test_hip_graph_capture_of_the_call_and_the_update(ctxs, kind):
    """One call and the update x += tend*dt captured on one stream; three replays equal three eager calls bit for bit."""
    import torch
    m = ctxs[kind]
    ncol, nz = 77, 120
    F, adv, div, exner, dz = _inputs(kind, ncol, nz)
    F = {k: F[k] for k in _keys(kind)}
    d_adv, d_div, d_ex, d_dz = _dev(adv), _dev(div), _dev(exner), _dev(dz)

    def one(Fd, work, out):
        r = m.kid_interface(Fd, DT, P0, R_ON_CP, d_ex, d_dz, adv=d_adv, div=d_div, work=work, out=out)
        for k in _keys(kind):
            Fd[k] += r[k] * DT
        return r

    def fresh():
        Fd, work = _dev(F), m.kid_workspace(ncol, nz, f64)
        out = {k: torch.empty_like(Fd["theta"]) for k in _keys(kind)}
        out["ppt"] = torch.empty(ncol, 4, dtype=torch.float64, device="cuda")
        return Fd, work, out
    Fe, we, oe = fresh()
    for _ in range(3):
        one(Fe, we, oe)
    torch.cuda.synchronize()
    Fg, wg, og = fresh()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        one(Fg, wg, og)
    for k in Fg:                                              # capture does not execute
        assert torch.equal(Fg[k].cpu(), torch.from_numpy(F[k]))
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    for k in _keys(kind):
        _same(Fg[k].cpu().numpy(), Fe[k].cpu().numpy(), "state " + k)
        _same(og[k].cpu().numpy(), oe[k].cpu().numpy(), "tendency " + k)
    _same(og["ppt"].cpu().numpy(), oe["ppt"].cpu().numpy(), "ppt")
    assert not np.array_equal(Fg["qc"].cpu().numpy(), F["qc"])


# ---- host entry ----
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("kind,dtype,arith", [("warm", f64, None), ("mixed", f64, None), ("warm", f32, "p32n"), ("mixed", f32, "p32n"),
                                              ("mixed", f32, "f32")])
def test_host_entry_equals_the_device_entry(ctxs, kind, dtype, arith, chunks, pinned):
    from kid_amd.thompson import host_pinned_copy
    m = ctxs[kind]
    ncol, nz = 301, 120
    F, adv, div, exner, dz = _inputs(kind, ncol, nz, dtype)
    dev = _call(m, F, adv, div, exner, dz, arith=arith, dbz=True, radii=True)
    if pinned:
        pin = lambda d: {k: host_pinned_copy(v) for k, v in d.items()}   # noqa: E731
        F, adv, div, exner, dz = pin(F), pin(adv), pin(div), host_pinned_copy(exner), host_pinned_copy(dz)
    m.set_host_chunk(0 if chunks == 1 else (ncol + chunks - 1) // chunks)
    keep = {k: v.copy() for k, v in F.items()}
    got = m.kid_interface_host(F, DT, P0, R_ON_CP, exner, dz, adv=adv, div=div, want_rates=True, want_nstep=True, dbz=True,
                               radii=True, arith=arith)
    for k in _keys(kind) + ("ppt", "rates", "nstep", "dbz"):
        _same(got[k], dev[k], "host %s" % k)
    for a, b, k in zip(got["radii"], dev["radii"], ("re_qc", "re_qi", "re_qs")):
        _same(a, b, k)
    for k in F:
        _same(F[k], keep[k], "state is IN: " + k)
    # without forcing and without the optional outputs
    dev0 = _call(m, keep, None, None, np.asarray(exner), np.asarray(dz), arith=arith)
    got0 = m.kid_interface_host(F, DT, P0, R_ON_CP, exner, dz, arith=arith)
    for k in _keys(kind) + ("ppt",):
        _same(got0[k], dev0[k], "host, no forcing: %s" % k)


def test_host_entry_with_a_bound_droplet_number_in_three_chunks(ctxs):
    m = ctxs["mixed"]
    ncol, nz = 301, 120
    m.set_column_nc(np.array([(25.0, 100.0, 300.0, 1000.0)[c % 4] for c in range(ncol)]))
    F, adv, div, exner, dz = _inputs("mixed", ncol, nz)
    dev = _call(m, F, adv, div, exner, dz, dbz=True, radii=True)
    m.set_host_chunk(101)
    got = m.kid_interface_host(F, DT, P0, R_ON_CP, exner, dz, adv=adv, div=div, dbz=True, radii=True)
    for k in FIELDS + ("ppt", "dbz"):
        _same(got[k], dev[k], "host %s" % k)
    for a, b in zip(got["radii"], dev["radii"]):
        _same(a, b, "radii")


# ---- refusals ----
def test_refused_calls_write_nothing(ctxs):
    import torch
    from kid_amd.thompson import _KidFields, load_library
    L = load_library()
    ncol, nz = 13, 120
    F, adv, div, exner, dz = _inputs("mixed", ncol, nz)
    Fd, ex, dzd = _dev(F), _dev(exner), _dev(dz)
    SENT = -777.25
    out = {k: torch.full((ncol, nz), SENT, dtype=torch.float64, device="cuda") for k in FIELDS}
    ppt = torch.full((ncol, 4), SENT, dtype=torch.float64, device="cuda")
    need = L.kidmp_kid_workspace_bytes(ncol, nz)
    work = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")

    def fields(d, drop=()):
        return _KidFields(*[None if k in drop or k not in d else d[k].data_ptr() for k in FIELDS])

    def call(m, state, mphys, nz_=nz, dt=DT, wbytes=need, wptr=work.data_ptr(), ppt_=ppt.data_ptr(), exner_=ex.data_ptr()):
        rc = L.kidmp_kid_interface_device(m._h, ncol, nz_, dt, P0, R_ON_CP, C.byref(state), None, None, exner_, dzd.data_ptr(),
                                          C.byref(mphys), ppt_, None, None, None, wptr, wbytes, None)
        torch.cuda.synchronize()
        return rc
    mixed, warm = ctxs["mixed"], ctxs["warm"]
    EINVAL = -1
    assert call(mixed, fields(Fd), fields(out), wbytes=need - 1) == EINVAL                # a workspace that is too small
    assert "workspace" in load_library().kidmp_last_error(mixed._h).decode()
    assert call(mixed, fields(Fd), fields(out), wptr=None) == EINVAL
    assert call(mixed, fields(Fd, drop=("qr",)), fields(out)) == EINVAL                   # a missing required member
    assert call(warm, fields(Fd, drop=("theta",)), fields(out)) == EINVAL
    assert call(mixed, fields(Fd), fields(out, drop=("nr",))) == EINVAL
    assert call(mixed, fields(Fd, drop=("qi",)), fields(out)) == EINVAL                   # mixed phase without state->qi
    assert "mixed-phase" in load_library().kidmp_last_error(mixed._h).decode()
    assert call(mixed, fields(Fd), fields(out, drop=("qg",))) == EINVAL
    assert call(mixed, fields(Fd), fields(out), ppt_=None) == EINVAL
    assert call(mixed, fields(Fd), fields(out), exner_=None) == EINVAL
    assert call(mixed, fields(Fd), fields(out), nz_=1) == EINVAL                          # nz out of range
    assert call(mixed, fields(Fd), fields(out), nz_=257) == EINVAL
    assert call(mixed, fields(Fd), fields(out), dt=0.0) == EINVAL
    assert call(mixed, fields(Fd), fields(out), dt=-1.0) == EINVAL
    mixed.set_column_nc(np.full(ncol + 1, 100.0))                                         # ncol must equal the bound count
    assert call(mixed, fields(Fd), fields(out)) == EINVAL
    mixed.set_column_nc(None)
    for k in FIELDS:                                                                      # every output keeps its sentinel
        assert bool((out[k] == SENT).all()), k
    assert bool((ppt == SENT).all()) and bool((work == 0x5A).all())
    # the warm context takes the same call without any frozen member, and an empty batch is fine
    assert call(warm, fields(Fd, drop=FROZEN), fields(out, drop=FROZEN)) == 0
    assert not bool((out["qc"] == SENT).any()) and bool((out["qi"] == SENT).all())
    assert L.kidmp_kid_interface_device(mixed._h, 0, nz, DT, P0, R_ON_CP, None, None, None, None, None, None, None, None, None, None,
                                        None, 0, None) == 0
    assert call(mixed, fields(Fd), fields(out)) == 0
    assert not bool((out["qi"] == SENT).all())
