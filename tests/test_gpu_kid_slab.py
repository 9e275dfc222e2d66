"""The slab entries on the MI355X (include/kidmp_slab.h, kidmp::k_kid_advect_slab) against tests/kid_slab_ref.py.  -m gpu.

Every comparison with the reference is an equality of bits, binary64 and binary32 alike: the scheme is fixed to the
operation, numpy rounds each of them once, and the binary32 reference is the binary64 reference on the widened inputs,
rounded once.  The shapes are those where the kernel can go wrong: nx around the strip of W cells that a workgroup owns
(a strip shorter than W, a slab shorter than the stencil's reach, two strips and a bit), nz around the hand-over between
level groups, and more than one slab.  Three cross-checks need no reference: a roll of the cells in x, a slab alone and
in a batch, and the 1-D entry where u is zero."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import kid_advect_ref as ref
import kid_slab_ref as sref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = int(re.search(r"SLAB_WAVES\s*=\s*(\d+)", open(os.path.join(ROOT, "kid_amd", "csrc", "kidmp_slab.hip")).read()).group(1))
NX_SWEEP = tuple(sorted({3, 4, W - 1, W, W + 1, 2 * W + 1}))       # the smallest slabs and the strip's edges
NZ_SWEEP = (2, 3, 64, 65, 129, 256)
EINVAL, ESTATE = -1, -5
DT, DX = 4.0, 150.0
CANARY = -777.25
ALL = ("adv", "div", "sum")


def _fields_np(rng, ncol, nz):
    """All nine members: values over many decades, about a third of the cells exactly zero (theta never)."""
    st = {}
    for k in ref.FIELDS:
        hi = 7.0 if k in ("nr", "ni") else -2.0
        st[k] = 10.0 ** rng.uniform(hi - 9.0, hi, (ncol, nz)) * (rng.random((ncol, nz)) < 0.65)
    st["theta"] = 290.0 + 40.0 * np.linspace(0.0, 1.0, nz)[None, :] ** 2 + rng.normal(0.0, 0.5, (ncol, nz))
    return {k: np.ascontiguousarray(v) for k, v in st.items()}


def _flow_np(rng, ncol, nx, nz):
    """u [ncol, nz], w [ncol, nz+1]: random sizes, the signs a chequerboard that changes inside every row (along x) and
    inside every column (along z) for any nx >= 3 and nz >= 2; w = 0 at the ground."""
    i = (np.arange(ncol) % nx)[:, None]
    k, f = np.arange(nz)[None, :], np.arange(nz + 1)[None, :]
    u = rng.uniform(0.2, 3.0, (ncol, nz)) * np.where((i + (k + 1) // 2) % 2 == 0, 1.0, -1.0)
    w = rng.uniform(0.2, 3.0, (ncol, nz + 1)) * np.where((i + f // 2) % 2 == 0, 1.0, -1.0)
    w[:, 0] = 0.0
    return np.ascontiguousarray(u), np.ascontiguousarray(w)


def _changes_sign_everywhere(u, w, nx):
    u3, w3 = u.reshape(-1, nx, u.shape[1]), w.reshape(-1, nx, w.shape[1])[:, :, 1:]
    rows = all(((a > 0).any(axis=1) & (a < 0).any(axis=1)).all() for a in (u3, w3))
    cols = all(((a > 0).any(axis=2) & (a < 0).any(axis=2)).all() for a in (u3, w3))
    return rows and cols


def _profiles_np(rng, nz):
    return (np.ascontiguousarray(1.2 * np.exp(-np.linspace(0.0, 1.1, nz)) * rng.uniform(0.97, 1.03, nz)),
            np.ascontiguousarray(rng.uniform(20.0, 60.0, nz)))


def _case(nslab, nx, nz, seed=0, dtype=f64):
    """(state, u, w, rho, dz) of `dtype` with a flow per slab; a binary32 case is the binary64 one rounded."""
    rng = np.random.Generator(np.random.PCG64(16000 + 1000 * seed + 7 * nx + nz))
    ncol = nslab * nx
    st = _fields_np(rng, ncol, nz)
    u, w = _flow_np(rng, ncol, nx, nz)
    rho, dz = _profiles_np(rng, nz)
    return {k: v.astype(dtype) for k, v in st.items()}, u.astype(dtype), w.astype(dtype), rho.astype(dtype), dz.astype(dtype)


def _reference(st, u, w, rho, dz, nx, dt=DT, dx=DX, keys=None):
    """The reference in the inputs' dtype: binary64 on the widened inputs, rounded once."""
    T = u.dtype.type
    out = sref.advect_slab(st, u, w, rho, dz, dx, dt, nx, keys)
    res = {n: {k: v.astype(T) for k, v in out[n].items()} for n in ALL}
    res["courant"] = out["courant"].astype(T)
    return res


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _dev(d):
    return {k: _cu(v) for k, v in d.items() if v is not None}


def _host(res):
    import torch
    torch.cuda.synchronize()
    return {n: ({k: a.cpu().numpy() for k, a in v.items()} if isinstance(v, dict) else v.cpu().numpy()) for n, v in res.items()}


def _advect(m, st, u, w, rho, dz, nx, dt=DT, dx=DX, want=ALL, courant=True):
    return _host(m.kid_advect_slab(_dev(st), _cu(u), _cu(w), _cu(rho), _cu(dz), dx, dt, nx, want=want, courant=courant))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == f64 else np.uint32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    diff = _bits(a) != _bits(b)
    assert not diff.any(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        what, int(diff.sum()), diff.size, np.argwhere(diff)[0], a[tuple(np.argwhere(diff)[0])], b[tuple(np.argwhere(diff)[0])])


def _same_result(got, want, what, keys=ref.FIELDS, select=lambda a: a):
    for n in ALL:
        if n in want and n in got:
            assert sorted(got[n]) == sorted(keys), (what, n, sorted(got[n]))
            for k in keys:
                _same(got[n][k], select(want[n][k]), "%s %s[%s]" % (what, n, k))
    if "courant" in got:
        _same(got["courant"], select(want["courant"]), what + " courant")


# ---- 1. nx across the strip's edges, nz across the level groups ----
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
@pytest.mark.parametrize("nz", NZ_SWEEP)
@pytest.mark.parametrize("nx", NX_SWEEP)
def test_advect_slab_equals_the_reference_bit_for_bit(gpu_mixed, nx, nz, dtype):
    st, u, w, rho, dz = _case(2, nx, nz, dtype=dtype)
    assert _changes_sign_everywhere(u, w, nx)
    keep = {k: v.copy() for k, v in st.items()}
    got = _advect(gpu_mixed, st, u, w, rho, dz, nx)
    want = _reference(st, u, w, rho, dz, nx)
    _same_result(got, want, "nx=%d nz=%d" % (nx, nz))
    assert all(np.isfinite(want["sum"][k]).all() for k in ref.FIELDS) and np.abs(want["adv"]["qv"]).max() > 0
    for k in st:
        _same(st[k], keep[k], "input " + k)


def test_inputs_are_unchanged_on_the_device(gpu_mixed):
    import torch
    nx = W + 1
    st, u, w, rho, dz = _case(2, nx, 65)
    d, du, dw, drho, ddz = _dev(st), _cu(u), _cu(w), _cu(rho), _cu(dz)
    gpu_mixed.kid_advect_slab(d, du, dw, drho, ddz, DX, DT, nx, want=ALL, courant=True)
    torch.cuda.synchronize()
    for k in st:
        _same(d[k].cpu().numpy(), st[k], "state " + k)
    for name, a, b in (("u", du, u), ("w", dw, w), ("rho", drho, rho), ("dz", ddz, dz)):
        _same(a.cpu().numpy(), b, name)


# ---- 2. the number of slabs; one flow for all against one per slab ----
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
@pytest.mark.parametrize("nslab", [1, 2, 3])
def test_nslab_sweep_shared_against_per_slab_flow(gpu_mixed, nslab, dtype):
    nx, nz = W + 1, 65
    st, u, w, rho, dz = _case(nslab, nx, nz, seed=1, dtype=dtype)
    per_slab = _advect(gpu_mixed, st, u, w, rho, dz, nx)
    _same_result(per_slab, _reference(st, u, w, rho, dz, nx), "nslab=%d, a flow per slab" % nslab)
    u1, w1 = u[:nx].copy(), w[:nx].copy()
    shared = _advect(gpu_mixed, st, u1, w1, rho, dz, nx)                   # [nx, ..]: every slab's
    _same_result(shared, _reference(st, u1, w1, rho, dz, nx), "nslab=%d, one flow" % nslab)
    replicated = _advect(gpu_mixed, st, np.tile(u1, (nslab, 1)), np.tile(w1, (nslab, 1)), rho, dz, nx)
    _same_result(shared, replicated, "nslab=%d, one flow against its copies" % nslab)
    if nslab > 1:
        assert (_bits(shared["sum"]["qv"]) != _bits(per_slab["sum"]["qv"])).any()


@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
def test_zero_flow(gpu_mixed, dtype):
    nx, nz = W + 1, 65
    st, u, w, rho, dz = _case(2, nx, nz, seed=2, dtype=dtype)
    for name, z in (("zero", 0.0), ("minus zero", -0.0)):
        u0, w0 = np.full_like(u, z), np.full_like(w, z)
        got = _advect(gpu_mixed, st, u0, w0, rho, dz, nx)
        _same_result(got, _reference(st, u0, w0, rho, dz, nx), name)
        for n in ALL:
            for k in ref.FIELDS:
                assert not (_bits(got[n][k]) << 1).any(), (name, n, k)       # +0.0 or -0.0, nothing else
        assert not _bits(got["courant"]).any()


# ---- 3. what is asked for ----
def _kid_fields(d):
    from kid_amd.thompson import _KidFields
    return _KidFields(*[d[k].data_ptr() if d.get(k) is not None else None for k in ref.FIELDS])


def _raw(m, nslab, nx, nz, dt, dx, state, u, w, shared, rho, dz, adv, div, sum_, courant, is64=True, ctx=True):
    """The C entry itself: dicts of tensors (or None) for the four structs, tensors (or None, or an address) for the rest."""
    import torch
    from kid_amd.slab import library
    L = library()
    fn = L.kidmp_kid_advect_slab_device if is64 else L.kidmp32_kid_advect_slab_device
    ptr = lambda a: a if a is None or isinstance(a, int) else a.data_ptr()   # noqa: E731
    structs = [None if d is None else _kid_fields(d) for d in (state, adv, div, sum_)]
    refs = [None if s is None else C.byref(s) for s in structs]
    rc = fn(m._h if ctx else None, nslab, nx, nz, dt, dx, refs[0], ptr(u), ptr(w), shared, ptr(rho), ptr(dz), refs[1], refs[2], refs[3],
            ptr(courant), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_every_subset_of_outputs_gives_the_bits_of_all_together(gpu_mixed):
    nx = W + 1
    st, u, w, rho, dz = _case(2, nx, 65, seed=3)
    both = _advect(gpu_mixed, st, u, w, rho, dz, nx)
    for r in (1, 2):
        for names in itertools.combinations(ALL, r):
            for courant in (False, True):
                one = _advect(gpu_mixed, st, u, w, rho, dz, nx, want=names, courant=courant)
                assert sorted(one) == sorted(names + (("courant",) if courant else ()))
                _same_result(one, both, "+".join(names))
    only_c = _advect(gpu_mixed, st, u, w, rho, dz, nx, want=(), courant=True)
    assert sorted(only_c) == ["courant"]
    _same(only_c["courant"], both["courant"], "courant alone")


def test_null_members_are_not_advected_and_their_outputs_stay(gpu_mixed):
    import torch
    nslab, nx, nz = 2, W + 1, 65
    ncol = nslab * nx
    st, u, w, rho, dz = _case(nslab, nx, nz, seed=4)
    want = _reference(st, u, w, rho, dz, nx)
    d = _dev(st)
    d["qi"] = d["qs"] = None                                        # not advected
    canary = lambda: torch.full((ncol, nz), CANARY, dtype=torch.float64, device="cuda:0")   # noqa: E731
    adv = {k: canary() for k in ref.FIELDS}
    sum_ = {k: canary() for k in ref.FIELDS}
    held = {k: sum_[k] for k in ("qv", "nr")}                        # present fields whose sum is not asked for
    for k in held:
        sum_ = dict(sum_, **{k: None})
    assert _raw(gpu_mixed, nslab, nx, nz, DT, DX, d, _cu(u), _cu(w), 0, _cu(rho), _cu(dz), adv, None, sum_, None) == 0
    for k in ref.FIELDS:
        if k in ("qi", "qs"):
            assert (adv[k] == CANARY).all() and (sum_[k] == CANARY).all(), k
        else:
            _same(adv[k].cpu().numpy(), want["adv"][k], "adv " + k)
            if k in held:
                assert (held[k] == CANARY).all(), k
            else:
                _same(sum_[k].cpu().numpy(), want["sum"][k], "sum " + k)


def test_warm_context_ignores_the_frozen_members(gpu_warm):
    import torch
    nslab, nx, nz = 2, W + 1, 65
    ncol = nslab * nx
    st, u, w, rho, dz = _case(nslab, nx, nz, seed=5)
    want = _reference(st, u, w, rho, dz, nx, keys=ref.WARM)
    d = _dev(st)
    garbage = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda:0")   # valid memory, far too small
    for k in ref.FIELDS[5:]:
        d[k] = garbage
    out = {n: {k: torch.full((ncol, nz), CANARY, dtype=torch.float64, device="cuda:0") for k in ref.FIELDS} for n in ALL}
    cour = torch.full((ncol,), CANARY, dtype=torch.float64, device="cuda:0")
    assert _raw(gpu_warm, nslab, nx, nz, DT, DX, d, _cu(u), _cu(w), 0, _cu(rho), _cu(dz), out["adv"], out["div"], out["sum"], cour) == 0
    for n in ALL:
        for k in ref.WARM:
            _same(out[n][k].cpu().numpy(), want[n][k], "warm %s[%s]" % (n, k))
        for k in ref.FIELDS[5:]:
            assert (out[n][k] == CANARY).all(), (n, k)
    _same(cour.cpu().numpy(), want["courant"], "warm courant")
    py = _host(gpu_warm.kid_advect_slab(_dev(st), _cu(u), _cu(w), _cu(rho), _cu(dz), DX, DT, nx))   # the wrapper passes the frozen ones over
    assert sorted(py["sum"]) == sorted(ref.WARM)
    _same_result(py, want, "warm wrapper", ref.WARM)


# ---- 4. cross-checks that need no reference ----
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
@pytest.mark.parametrize("r", [1, W - 1])
def test_rolling_the_cells_in_x_rolls_every_output(gpu_mixed, r, dtype):
    nslab, nx, nz = 2, 2 * W + 1, 65
    st, u, w, rho, dz = _case(nslab, nx, nz, seed=6, dtype=dtype)
    roll = lambda a: np.ascontiguousarray(np.roll(a.reshape(nslab, nx, -1), r, axis=1).reshape(a.shape))   # noqa: E731
    got = _advect(gpu_mixed, st, u, w, rho, dz, nx)
    rolled = _advect(gpu_mixed, {k: roll(v) for k, v in st.items()}, roll(u), roll(w), rho, dz, nx)
    _same_result(rolled, got, "rolled by %d" % r, select=roll)
    assert (_bits(rolled["sum"]["qv"]) != _bits(got["sum"]["qv"])).any()


def test_a_slab_alone_and_at_any_position_of_a_batch(gpu_mixed):
    nslab, nx, nz = 3, W + 1, 65
    st, u, w, rho, dz = _case(nslab, nx, nz, seed=7)
    got = _advect(gpu_mixed, st, u, w, rho, dz, nx)
    again = _advect(gpu_mixed, st, u, w, rho, dz, nx)
    _same_result(again, got, "repeated")
    slab = lambda a, s: np.ascontiguousarray(a.reshape(nslab, nx, -1)[s].reshape((nx,) + a.shape[1:]))   # noqa: E731
    for s in range(nslab):
        alone = _advect(gpu_mixed, {k: slab(v, s) for k, v in st.items()}, slab(u, s), slab(w, s), rho, dz, nx)
        _same_result(alone, got, "slab %d alone" % s, select=lambda a: slab(a, s))
    order = [2, 0, 1]
    perm = lambda a: np.ascontiguousarray(a.reshape(nslab, nx, -1)[order].reshape(a.shape))   # noqa: E731
    moved = _advect(gpu_mixed, {k: perm(v) for k, v in st.items()}, perm(u), perm(w), rho, dz, nx)
    _same_result(moved, got, "slabs in another order", select=perm)


@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
def test_without_u_the_outputs_equal_the_column_entry(gpu_mixed, dtype):
    """u = +0.0 and non-negative fields: equality of numbers with kid_advect (a zero may differ in sign, as the header says)."""
    nslab, nx, nz = 2, W + 1, 129
    st, u, w, rho, dz = _case(nslab, nx, nz, seed=8, dtype=dtype)
    assert all((v >= 0).all() for v in st.values())
    slab = _advect(gpu_mixed, st, np.zeros_like(u), w, rho, dz, nx)
    col = _host(gpu_mixed.kid_advect(_dev(st), _cu(w), _cu(rho), _cu(dz), DT, want=ALL, courant=True))
    for n in ALL:
        for k in ref.FIELDS:
            assert np.array_equal(slab[n][k], col[n][k]), (n, k)
    assert np.array_equal(slab["courant"], col["courant"]) and np.abs(col["sum"]["qv"]).max() > 0


# ---- 5. refusals ----
def test_refusals_write_nothing(gpu_mixed):
    import torch
    from kid_amd.slab import library
    from kid_amd.thompson import _KidFields
    L = library()
    m, nslab, nx, nz = gpu_mixed, 2, W + 1, 65
    ncol = nslab * nx
    st, u, w, rho, dz = _case(nslab, nx, nz, seed=9)
    d, du, dw, drho, ddz = _dev(st), _cu(u), _cu(w), _cu(rho), _cu(dz)
    out = {k: torch.full((ncol, nz), CANARY, dtype=torch.float64, device="cuda:0") for k in ref.FIELDS}
    cour = torch.full((ncol,), CANARY, dtype=torch.float64, device="cuda:0")
    host = np.zeros((ncol, nz + 1))
    big = torch.zeros(ncol, 258, dtype=torch.float64, device="cuda:0")

    def adv(nslab=nslab, nx=nx, nz=nz, dt=DT, dx=DX, state=d, u=du, w=dw, shared=0, rho=drho, dz=ddz, sum_=out, courant=cour, ctx=True):
        return _raw(m, nslab, nx, nz, dt, dx, state, u, w, shared, rho, dz, None, None, sum_, courant, ctx=ctx)

    assert adv(ctx=False) == ESTATE
    refused = {
        "nx = 2": adv(nx=2),
        "nx = 0": adv(nx=0),
        "nx < 0": adv(nx=-3),
        "nz = 1": adv(nz=1),
        "nz = 257": adv(nz=257, state={k: big for k in ref.FIELDS}, u=big, w=big),
        "nslab < 0": adv(nslab=-1),
        "nslab*nx > 2^31 - 1": adv(nslab=(0x7fffffff // nx) + 1),
        "nslab*nx past 2^63": adv(nslab=2 ** 62),
        "dt = 0": adv(dt=0.0),
        "dt < 0": adv(dt=-1.0),
        "dt NaN": adv(dt=float("nan")),
        "dx = 0": adv(dx=0.0),
        "dx < 0": adv(dx=-DX),
        "dx NaN": adv(dx=float("nan")),
        "state NULL": adv(state=None),
        "theta NULL": adv(state=dict(d, theta=None)),
        "nr NULL": adv(state=dict(d, nr=None)),
        "u NULL": adv(u=None),
        "w NULL": adv(w=None),
        "rho NULL": adv(rho=None),
        "dz NULL": adv(dz=None),
        "nothing requested": adv(sum_=None, courant=None),
        "only outputs of absent fields": adv(state=dict(d, qi=None), sum_={"qi": out["qi"]}, courant=None),
        "u on the host": adv(u=host.ctypes.data),
        "w on the host": adv(w=host.ctypes.data),
        "rho on the host": adv(rho=host.ctypes.data),
        "courant on the host": adv(courant=host.ctypes.data),
    }
    hf = _KidFields(*[d[k].data_ptr() for k in ref.FIELDS])
    hf.qc = host.ctypes.data
    refused["qc on the host"] = L.kidmp_kid_advect_slab_device(m._h, nslab, nx, nz, DT, DX, C.byref(hf), du.data_ptr(), dw.data_ptr(), 0,
                                                               drho.data_ptr(), ddz.data_ptr(), None, None, C.byref(_kid_fields(out)), None,
                                                               torch.cuda.current_stream().cuda_stream)
    ho = _kid_fields(out)
    ho.qr = host.ctypes.data
    refused["an output on the host"] = L.kidmp_kid_advect_slab_device(m._h, nslab, nx, nz, DT, DX, C.byref(_kid_fields(d)), du.data_ptr(),
                                                                      dw.data_ptr(), 0, drho.data_ptr(), ddz.data_ptr(), None, None, C.byref(ho),
                                                                      None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert {k: v for k, v in refused.items() if v != EINVAL} == {}
    assert all((a == CANARY).all() for a in out.values()) and (cour == CANARY).all()
    assert adv(nslab=0) == 0 and (cour == CANARY).all()                # an empty batch: nothing to do
    assert adv(dx=0.0) == EINVAL and b"kidmp_kid_advect_slab_device" in L.kidmp_last_error(m._h)
    assert adv() == 0 and (cour != CANARY).all() and all((a != CANARY).any() for a in out.values())   # and a good call does write


# ---- 6. graph capture ----
def test_hip_graph_capture_replayed_twice(gpu_mixed):
    """advect_slab + update captured once on one stream, out= reused: two replays equal two eager calls and the reference."""
    import torch
    m, nslab, nx, nz = gpu_mixed, 2, W + 1, 65
    ncol = nslab * nx
    st, u, w, rho, dz = _case(nslab, nx, nz, seed=10)
    du, dw, drho, ddz = _cu(u), _cu(0.5 * w), _cu(rho), _cu(dz)

    def step(state, out):
        out = m.kid_advect_slab(state, du, dw, drho, ddz, DX, DT, nx, want="sum", courant=True, out=out)
        m.kid_update(state, DT, out["sum"])
        return out

    graphed = _dev(st)
    out_g = {"sum": {k: torch.zeros_like(graphed[k]) for k in ref.FIELDS}, "courant": torch.zeros(ncol, dtype=torch.float64, device="cuda:0")}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert step(graphed, out_g) is out_g
    for k, v in _dev(st).items():                                    # whatever the capture did to the state: start over
        graphed[k].copy_(v)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    eager, out_e = _dev(st), None
    for _ in range(2):
        out_e = step(eager, out_e)
    torch.cuda.synchronize()
    for k in ref.FIELDS:
        assert torch.equal(graphed[k], eager[k]), k
        assert torch.equal(out_g["sum"][k], out_e["sum"][k]), k
    assert torch.equal(out_g["courant"], out_e["courant"])
    x = {k: v.copy() for k, v in st.items()}
    for _ in range(2):
        x = ref.update(x, DT, sref.advect_slab(x, u, 0.5 * w, rho, dz, DX, DT, nx)["sum"])
    for k in ref.FIELDS:
        _same(eager[k].cpu().numpy(), x[k], "two steps: " + k)
