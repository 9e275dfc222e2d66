"""The kinematic entries on the MI355X (include/kidmp_kinematic.h, kidmp::k_kid_advect / k_kid_update) against
tests/kid_advect_ref.py.  -m gpu.

Every comparison with the reference is an equality of bits, binary64 and binary32 alike: the scheme is fixed to the
operation, numpy rounds each of them once, and the binary32 reference is the binary64 reference on the widened inputs,
rounded once.  The shapes are those where the hand-over between level groups (lane 63 -> lane 0), the faces without a
second upwind cell and the top face can go wrong."""
import ctypes as C

import numpy as np
import pytest

import kid_advect_ref as ref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NZ_SWEEP = (2, 3, 4, 63, 64, 65, 127, 128, 129, 192, 193, 256)
NCOL_SWEEP = (1, 3, 4, 5, 9)
EINVAL, ESTATE = -1, -5
DT = 4.0
CANARY = -777.25


def _fields_np(rng, ncol, nz):
    """All nine members: values over many decades, about a third of the cells exactly zero (theta never)."""
    st = {}
    for k in ref.FIELDS:
        hi = 7.0 if k in ("nr", "ni") else -2.0
        st[k] = 10.0 ** rng.uniform(hi - 9.0, hi, (ncol, nz)) * (rng.random((ncol, nz)) < 0.65)
    st["theta"] = 290.0 + 40.0 * np.linspace(0.0, 1.0, nz)[None, :] ** 2 + rng.normal(0.0, 0.5, (ncol, nz))
    return {k: np.ascontiguousarray(v) for k, v in st.items()}


def _w_np(rng, ncol, nz):
    """[ncol, nz+1], both signs and a sign change inside every column (nz = 2: between the one interior face and the top)."""
    f = np.linspace(0.0, 1.0, nz + 1)[None, :]
    w = rng.uniform(0.5, 3.0, (ncol, 1)) * np.sin(2.0 * np.pi * rng.integers(1, 3, (ncol, 1)) * f + rng.uniform(0.1, 3.0, (ncol, 1)))
    w += rng.normal(0.0, 0.2, w.shape)
    w[:, 0] = 0.0
    flip = nz // 2 + 1
    w[:, flip] = -np.abs(w[:, flip]) - 0.1
    w[:, flip - 1] = np.abs(w[:, flip - 1]) + 0.1
    return np.ascontiguousarray(w)


def _profiles_np(rng, nz):
    return (np.ascontiguousarray(1.2 * np.exp(-np.linspace(0.0, 1.1, nz)) * rng.uniform(0.97, 1.03, nz)),
            np.ascontiguousarray(rng.uniform(20.0, 60.0, nz)))


def _case(ncol, nz, seed=0, dtype=f64):
    """(state, w, rho, dz) of `dtype`; a binary32 case is the binary64 one rounded."""
    rng = np.random.Generator(np.random.PCG64(9000 + 1000 * seed + nz))
    st, w = _fields_np(rng, ncol, nz), _w_np(rng, ncol, nz)
    rho, dz = _profiles_np(rng, nz)
    return {k: v.astype(dtype) for k, v in st.items()}, w.astype(dtype), rho.astype(dtype), dz.astype(dtype)


def _reference(st, w, rho, dz, dt=DT, keys=None):
    """The reference in the inputs' dtype: binary64 on the widened inputs, rounded once."""
    T = w.dtype.type
    out = ref.advect(st, w, rho, dz, dt, keys)
    res = {n: {k: v.astype(T) for k, v in out[n].items()} for n in ("adv", "div", "sum")}
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


def _advect(m, st, w, rho, dz, dt=DT, want=("adv", "div", "sum"), courant=True):
    return _host(m.kid_advect(_dev(st), _cu(w), _cu(rho), _cu(dz), dt, want=want, courant=courant))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == f64 else np.uint32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    diff = _bits(a) != _bits(b)
    assert not diff.any(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        what, int(diff.sum()), diff.size, np.argwhere(diff)[0], a[tuple(np.argwhere(diff)[0])], b[tuple(np.argwhere(diff)[0])])


def _same_result(got, want, what, keys=ref.FIELDS):
    for n in ("adv", "div", "sum"):
        if n in want and n in got:
            assert sorted(got[n]) == sorted(keys), (what, n, sorted(got[n]))
            for k in keys:
                _same(got[n][k], want[n][k], "%s %s[%s]" % (what, n, k))
    if "courant" in got:
        _same(got["courant"], want["courant"], what + " courant")


# ---- 1. the nz sweep ----
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
@pytest.mark.parametrize("nz", NZ_SWEEP)
def test_advect_equals_the_reference_bit_for_bit(gpu_mixed, nz, dtype):
    st, w, rho, dz = _case(5, nz, dtype=dtype)
    keep = {k: v.copy() for k, v in st.items()}
    got = _advect(gpu_mixed, st, w, rho, dz)
    want = _reference(st, w, rho, dz)
    _same_result(got, want, "nz=%d" % nz)
    assert all(np.isfinite(want["sum"][k]).all() for k in ref.FIELDS) and np.abs(want["adv"]["qv"]).max() > 0
    assert ((w[:, 1:] < 0) != (w[:, :-1] < 0)).any(axis=1).all()
    for k in st:
        _same(st[k], keep[k], "input " + k)


def test_inputs_are_unchanged_on_the_device(gpu_mixed):
    import torch
    st, w, rho, dz = _case(5, 65)
    d, dw, drho, ddz = _dev(st), _cu(w), _cu(rho), _cu(dz)
    gpu_mixed.kid_advect(d, dw, drho, ddz, DT, want=("adv", "div", "sum"), courant=True)
    torch.cuda.synchronize()
    for k in st:
        _same(d[k].cpu().numpy(), st[k], "state " + k)
    _same(dw.cpu().numpy(), w, "w")
    _same(drho.cpu().numpy(), rho, "rho")
    _same(ddz.cpu().numpy(), dz, "dz")


# ---- 2. the ncol sweep: partial workgroups; a column alone, at any position, repeated ----
@pytest.mark.parametrize("ncol", NCOL_SWEEP)
def test_ncol_sweep_and_column_independence(gpu_mixed, ncol):
    st, w, rho, dz = _case(9, 65, seed=1)
    sub = {k: v[:ncol].copy() for k, v in st.items()}
    got = _advect(gpu_mixed, sub, w[:ncol].copy(), rho, dz)
    _same_result(got, _reference(sub, w[:ncol].copy(), rho, dz), "ncol=%d" % ncol)
    again = _advect(gpu_mixed, sub, w[:ncol].copy(), rho, dz)
    _same_result(again, got, "repeated ncol=%d" % ncol)
    c = ncol - 1                                              # the last column alone, and moved to the front of a batch
    alone = _advect(gpu_mixed, {k: v[c:c + 1].copy() for k, v in st.items()}, w[c:c + 1].copy(), rho, dz)
    order = [c] + [i for i in range(9) if i != c]
    moved = _advect(gpu_mixed, {k: v[order].copy() for k, v in st.items()}, w[order].copy(), rho, dz)
    for n in ("adv", "div", "sum"):
        for k in ref.FIELDS:
            _same(alone[n][k][0], got[n][k][c], "alone %s[%s]" % (n, k))
            _same(moved[n][k][0], got[n][k][c], "moved %s[%s]" % (n, k))
    _same(alone["courant"][0], got["courant"][c], "alone courant")
    _same(moved["courant"][0], got["courant"][c], "moved courant")


# ---- 3. the forms of w ----
def _w_patterns(nz):
    f = np.linspace(0.0, 1.0, nz + 1)
    bump = np.sin(np.pi * f)
    return {
        "all up": 2.0 * bump + 0.25,
        "all down": -2.0 * bump - 0.25,
        "convergent": 2.5 * np.where(f < 0.5, f, f - 1.0) * 2.0,     # up below the middle, down above it
        "divergent": -2.5 * np.where(f < 0.5, f, f - 1.0) * 2.0,
        "zero": np.zeros(nz + 1),
        "minus zero": -np.zeros(nz + 1),
    }


@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [65, 130])
def test_w_variants(gpu_mixed, nz, dtype):
    st, _, rho, dz = _case(5, nz, seed=2, dtype=dtype)
    for name, prof in _w_patterns(nz).items():
        w1 = np.ascontiguousarray(prof.astype(dtype))
        wn = np.ascontiguousarray(np.broadcast_to(w1, (5, nz + 1)))
        shared = _advect(gpu_mixed, st, w1, rho, dz)                 # stride 0
        per_col = _advect(gpu_mixed, st, wn, rho, dz)
        _same_result(shared, per_col, name + ": shared against replicated")
        _same_result(shared, _reference(st, wn, rho, dz), name)
        if "zero" in name:
            for n in ("adv", "div", "sum"):
                for k in ref.FIELDS:
                    assert not (_bits(shared[n][k]) << 1).any(), (name, n, k)      # +0.0 or -0.0, nothing else
            assert not _bits(shared["courant"]).any()
        else:
            assert shared["courant"].min() > 0 and np.abs(shared["sum"]["qv"]).max() > 0


# ---- 4. what is asked for ----
def _kid_fields(d):
    from kid_amd.thompson import _KidFields
    return _KidFields(*[d[k].data_ptr() if d.get(k) is not None else None for k in ref.FIELDS])


def _raw_advect(m, ncol, nz, dt, state, w, stride, rho, dz, adv, div, sum_, courant, is64=True, ctx=True):
    """The C entry itself: dicts of tensors (or None) for the four structs, tensors (or None, or an address) for the rest."""
    import torch
    from kid_amd.kinematic import library
    L = library()
    fn = L.kidmp_kid_advect_device if is64 else L.kidmp32_kid_advect_device
    ptr = lambda a: a if a is None or isinstance(a, int) else a.data_ptr()   # noqa: E731
    structs = [None if d is None else _kid_fields(d) for d in (state, adv, div, sum_)]
    refs = [None if s is None else C.byref(s) for s in structs]
    rc = fn(m._h if ctx else None, ncol, nz, dt, refs[0], ptr(w), stride, ptr(rho), ptr(dz), refs[1], refs[2], refs[3], ptr(courant),
            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def test_each_output_alone_gives_the_bits_of_all_together(gpu_mixed):
    st, w, rho, dz = _case(5, 65, seed=3)
    both = _advect(gpu_mixed, st, w, rho, dz)
    for n in ("adv", "div", "sum"):
        one = _advect(gpu_mixed, st, w, rho, dz, want=n, courant=False)
        assert sorted(one) == [n]
        _same_result(one, both, n + " alone")
    only_c = _advect(gpu_mixed, st, w, rho, dz, want=(), courant=True)
    assert sorted(only_c) == ["courant"]
    _same(only_c["courant"], both["courant"], "courant alone")


def test_null_members_are_not_advected_and_their_outputs_stay(gpu_mixed):
    import torch
    ncol, nz = 5, 65
    st, w, rho, dz = _case(ncol, nz, seed=4)
    want = _reference(st, w, rho, dz)
    d = _dev(st)
    d["qi"] = d["qs"] = None                                        # not advected
    canary = lambda: torch.full((ncol, nz), CANARY, dtype=torch.float64, device="cuda:0")   # noqa: E731
    adv = {k: canary() for k in ref.FIELDS}
    sum_ = {k: canary() for k in ref.FIELDS}
    held = {k: sum_[k] for k in ("qv", "nr")}                        # present fields whose sum is not asked for
    for k in held:
        sum_ = dict(sum_, **{k: None})
    assert _raw_advect(gpu_mixed, ncol, nz, DT, d, _cu(w), nz + 1, _cu(rho), _cu(dz), adv, None, sum_, None) == 0
    for k in ref.FIELDS:
        if k in ("qi", "qs"):
            assert (adv[k] == CANARY).all() and (sum_[k] == CANARY).all(), k
        else:
            _same(adv[k].cpu().numpy(), want["adv"][k], "adv " + k)
            if k in held:
                assert (held[k] == CANARY).all(), k
            else:
                _same(sum_[k].cpu().numpy(), want["sum"][k], "sum " + k)


# ---- 5. a warm context ----
def test_warm_context_ignores_the_frozen_members(gpu_warm):
    import torch
    ncol, nz = 5, 65
    st, w, rho, dz = _case(ncol, nz, seed=5)
    want = _reference(st, w, rho, dz, keys=ref.WARM)
    d = _dev(st)
    garbage = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda:0")   # valid memory, far too small
    for k in ref.FIELDS[5:]:
        d[k] = garbage
    out = {n: {k: torch.full((ncol, nz), CANARY, dtype=torch.float64, device="cuda:0") for k in ref.FIELDS} for n in ("adv", "div", "sum")}
    cour = torch.full((ncol,), CANARY, dtype=torch.float64, device="cuda:0")
    assert _raw_advect(gpu_warm, ncol, nz, DT, d, _cu(w), nz + 1, _cu(rho), _cu(dz), out["adv"], out["div"], out["sum"], cour) == 0
    for n in ("adv", "div", "sum"):
        for k in ref.WARM:
            _same(out[n][k].cpu().numpy(), want[n][k], "warm %s[%s]" % (n, k))
        for k in ref.FIELDS[5:]:
            assert (out[n][k] == CANARY).all(), (n, k)
    _same(cour.cpu().numpy(), want["courant"], "warm courant")
    py = _host(gpu_warm.kid_advect(_dev(st), _cu(w), _cu(rho), _cu(dz), DT))          # the wrapper passes the frozen ones over
    assert sorted(py["sum"]) == sorted(ref.WARM)
    _same_result(py, want, "warm wrapper", ref.WARM)


# ---- 6. the update ----
def _update_case(ncol, nz, dtype, seed):
    rng = np.random.Generator(np.random.PCG64(7000 + seed + nz))
    st = {k: v.astype(dtype) for k, v in _fields_np(rng, ncol, nz).items()}
    tend = [{k: (rng.normal(0.0, 1.0, (ncol, nz)) * np.abs(st[k]).max() / DT).astype(dtype) for k in ref.FIELDS} for _ in range(3)]
    return st, tend


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [2, 3, 64, 65])
def test_update_equals_the_reference_bit_for_bit(gpu_mixed, nz, dtype, clip):
    import torch
    ncol = 7
    st, t = _update_case(ncol, nz, dtype, 0)
    cases = {
        "three tendencies": (st, t),
        "two": (st, t[:2]),
        "none": (st, []),
        "a missing struct": (st, [t[0], None, t[2]]),
        "missing members": (st, [t[0], {k: v for k, v in t[1].items() if k not in ("qv", "qg")}, {"theta": t[2]["theta"]}]),
        "state without theta and qs": ({k: v for k, v in st.items() if k not in ("theta", "qs")}, t),
    }
    for name, (s, tt) in cases.items():
        d = _dev(s)
        back = gpu_mixed.kid_update(d, DT, *[None if x is None else _dev(x) for x in tt], clip=clip)
        torch.cuda.synchronize()
        assert back is d
        want = ref.update(s, DT, *tt, clip=clip)
        for k in s:
            _same(d[k].cpu().numpy(), want[k], "%s: %s" % (name, k))
    want = ref.update(st, DT, *t, clip=clip)
    assert (want["qv"] == 0).any() if clip else (want["qv"] < 0).any()
    assert (want["theta"] < 0).any()                                 # theta is never clipped


@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
def test_update_of_a_misaligned_view(gpu_mixed, dtype):
    """nz = 64 allows the 16-byte form; a state member one element off a 16-byte boundary must take the scalar one."""
    import torch
    ncol, nz = 7, 64
    st, t = _update_case(ncol, nz, dtype, 1)
    d = _dev(st)
    flat = torch.zeros(ncol * nz + 1, dtype=d["qc"].dtype, device="cuda:0")
    flat[1:] = d["qc"].reshape(-1)
    d["qc"] = flat[1:].view(ncol, nz)
    assert d["qc"].data_ptr() % 16 != 0 and d["qc"].is_contiguous()
    tt = [_dev(x) for x in t]
    tflat = torch.zeros(ncol * nz + 1, dtype=d["qc"].dtype, device="cuda:0")
    tflat[1:] = tt[1]["nr"].reshape(-1)
    tt[1]["nr"] = tflat[1:].view(ncol, nz)
    gpu_mixed.kid_update(d, DT, *tt)
    torch.cuda.synchronize()
    want = ref.update(st, DT, *t)
    for k in st:
        _same(d[k].cpu().numpy(), want[k], k)
    assert float(flat[0]) == 0.0


# ---- 7. refusals ----
def test_refusals_write_nothing(gpu_mixed):
    import torch
    from kid_amd.kinematic import library
    from kid_amd.thompson import _KidFields
    L = library()
    m, ncol, nz = gpu_mixed, 5, 65
    st, w, rho, dz = _case(ncol, nz, seed=6)
    d, dw, drho, ddz = _dev(st), _cu(w), _cu(rho), _cu(dz)
    out = {k: torch.full((ncol, nz), CANARY, dtype=torch.float64, device="cuda:0") for k in ref.FIELDS}
    cour = torch.full((ncol,), CANARY, dtype=torch.float64, device="cuda:0")
    host = np.zeros((ncol, nz + 1))
    big = torch.zeros(ncol, 258, dtype=torch.float64, device="cuda:0")

    def adv(ncol=ncol, nz=nz, dt=DT, state=d, w=dw, stride=nz + 1, rho=drho, dz=ddz, sum_=out, courant=cour, ctx=True):
        return _raw_advect(m, ncol, nz, dt, state, w, stride, rho, dz, None, None, sum_, courant, ctx=ctx)

    assert adv(ctx=False) == ESTATE
    refused = {
        "state NULL": adv(state=None),
        "theta NULL": adv(state=dict(d, theta=None)),
        "nr NULL": adv(state=dict(d, nr=None)),
        "w NULL": adv(w=None),
        "rho NULL": adv(rho=None),
        "dz NULL": adv(dz=None),
        "nz = 1": adv(nz=1),
        "nz = 257": adv(nz=257, state={k: big for k in ref.FIELDS}, stride=258),
        "ncol < 0": adv(ncol=-1),
        "dt = 0": adv(dt=0.0),
        "dt < 0": adv(dt=-1.0),
        "dt NaN": adv(dt=float("nan")),
        "stride = nz": adv(stride=nz),
        "stride < 0": adv(stride=-1),
        "nothing requested": adv(sum_=None, courant=None),
        "only outputs of absent fields": adv(state=dict(d, qi=None), sum_={"qi": out["qi"]}, courant=None),
        "w on the host": adv(w=host.ctypes.data),
        "courant on the host": adv(courant=host.ctypes.data),
    }
    hf = _KidFields(*[d[k].data_ptr() for k in ref.FIELDS])
    hf.qc = host.ctypes.data
    refused["qc on the host"] = L.kidmp_kid_advect_device(m._h, ncol, nz, DT, C.byref(hf), dw.data_ptr(), nz + 1, drho.data_ptr(), ddz.data_ptr(),
                                                          None, None, C.byref(_kid_fields(out)), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert {k: v for k, v in refused.items() if v != EINVAL} == {}
    assert all((a == CANARY).all() for a in out.values()) and (cour == CANARY).all()
    assert adv(ncol=0) == 0 and (cour == CANARY).all()                # an empty batch: nothing to do
    assert adv(dt=0.0) == EINVAL and b"kidmp_kid_advect_device" in L.kidmp_last_error(m._h)

    # the update
    x = {k: torch.full((ncol, nz), CANARY, dtype=torch.float64, device="cuda:0") for k in ref.FIELDS}
    t = {k: torch.ones((ncol, nz), dtype=torch.float64, device="cuda:0") for k in ref.FIELDS}
    s = torch.cuda.current_stream().cuda_stream

    def upd(ncol=ncol, nz=nz, dt=DT, state=x, t1=t, ctx=True):
        fs, ft = (None if state is None else _kid_fields(state)), _kid_fields(t1)
        rc = L.kidmp_kid_update_device(m._h if ctx else None, ncol, nz, dt, None if fs is None else C.byref(fs), C.byref(ft), None, None, 1, s)
        torch.cuda.synchronize()
        return rc

    assert upd(ctx=False) == ESTATE
    ht = dict(t)
    refused = {"state NULL": upd(state=None), "no member": upd(state={}), "nz = 1": upd(nz=1), "nz = 257": upd(nz=257), "ncol < 0": upd(ncol=-1),
               "dt = 0": upd(dt=0.0), "dt < 0": upd(dt=-2.0)}
    hf = _kid_fields(ht)
    hf.qv = np.zeros((ncol, nz)).ctypes.data
    refused["a tendency on the host"] = L.kidmp_kid_update_device(m._h, ncol, nz, DT, C.byref(_kid_fields(x)), C.byref(hf), None, None, 1, s)
    torch.cuda.synchronize()
    assert {k: v for k, v in refused.items() if v != EINVAL} == {}
    assert all((a == CANARY).all() for a in x.values())
    assert upd(ncol=0) == 0 and all((a == CANARY).all() for a in x.values())
    assert upd() == 0 and all((a == CANARY + DT).all() for k, a in x.items() if k == "theta")   # and a good call does write


# ---- 8. graph capture ----
def test_hip_graph_capture_advect_update(gpu_mixed):
    """advect + update captured once: three replays equal three eager calls."""
    import torch
    m, ncol, nz = gpu_mixed, 9, 65
    st, w, rho, dz = _case(ncol, nz, seed=7)
    dw, drho, ddz = _cu(0.5 * w), _cu(rho), _cu(dz)

    def step(state, out):
        out = m.kid_advect(state, dw, drho, ddz, DT, want="sum", courant=True, out=out)
        m.kid_update(state, DT, out["sum"])
        return out

    graphed = _dev(st)
    out_g = {"sum": {k: torch.zeros_like(graphed[k]) for k in ref.FIELDS}, "courant": torch.zeros(ncol, dtype=torch.float64, device="cuda:0")}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(graphed, out_g)
    for k, v in _dev(st).items():                                    # whatever the capture did to the state: start over
        graphed[k].copy_(v)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    eager, out_e = _dev(st), None
    for _ in range(3):
        out_e = step(eager, out_e)
    torch.cuda.synchronize()
    for k in ref.FIELDS:
        assert torch.equal(graphed[k], eager[k]), k
        assert torch.equal(out_g["sum"][k], out_e["sum"][k]), k
    assert torch.equal(out_g["courant"], out_e["courant"])
    # and the three eager steps are the reference's
    x = {k: v.copy() for k, v in st.items()}
    for _ in range(3):
        x = ref.update(x, DT, ref.advect(x, 0.5 * w, rho, dz, DT)["sum"])
    for k in ref.FIELDS:
        _same(eager[k].cpu().numpy(), x[k], "three steps: " + k)
