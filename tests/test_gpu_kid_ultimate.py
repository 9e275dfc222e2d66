"""ULTIMATE QUICKEST on the MI355X (include/kidmp_advection.h; the ULTIMATE instantiations of kidmp::k_kid_advect and
kidmp::k_kid_advect_slab) against tests/kid_ultimate_ref.py.  -m gpu.

Every comparison with the reference is an equality of bits, binary64 and binary32 alike: the scheme is fixed to the
operation, numpy rounds each of them once, and the binary32 reference is the binary64 reference on the widened inputs,
rounded once.  The inputs (tests/kid_ultimate_cases.py) are those of the van Leer tests -- fields over many decades with a
third exact zeros, w of both signs with a sign change in every column -- with interior faces of w = +0.0, w = -0.0, c = 1
and c = 1.5 planted; tests/test_kid_ultimate_abi.py asserts on the reference's masks that they reach every branch of the
limiter, and the first test here asserts it again on what it runs.  The shapes are those where the kernels can go wrong: nz
at the edges of the `uu inside` test and at every hand-over between level groups, whole and partial workgroups of four
waves, nx around the strip of four cells, one and two slabs.  Every test leaves the shared contexts at "vanleer"."""
import numpy as np
import pytest

import kid_advect_ref as ref
import kid_ultimate_cases as cases
import kid_ultimate_ref as uref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NZ_SWEEP = (2, 3, 4, 63, 64, 65, 128, 129, 256)
NCOL_SWEEP = (1, 3, 4, 5, 9)
NX_SWEEP = (3, 4, 5, 9)
DT, DX = cases.DT, cases.DX
ALL = ("adv", "div", "sum")
AER = ("nc", "nwfa", "nifa")


@pytest.fixture
def ult(gpu_mixed):
    gpu_mixed.set_advection("ultimate")
    yield gpu_mixed
    gpu_mixed.set_advection("vanleer")


@pytest.fixture
def ult_aero(gpu_mixed_aero):
    gpu_mixed_aero.set_advection("ultimate")
    yield gpu_mixed_aero
    gpu_mixed_aero.set_advection("vanleer")


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _dev(d):
    return {k: _cu(v) for k, v in d.items() if v is not None}


def _host(res):
    import torch
    torch.cuda.synchronize()
    return {n: ({k: a.cpu().numpy() for k, a in v.items()} if isinstance(v, dict) else v.cpu().numpy()) for n, v in res.items()}


def _advect(m, st, w, rho, dz, dt=DT, want=ALL, courant=True):
    return _host(m.kid_advect(_dev(st), _cu(w), _cu(rho), _cu(dz), dt, want=want, courant=courant))


def _advect_slab(m, st, u, w, rho, dz, nx, dt=DT, dx=DX, want=ALL, courant=True):
    return _host(m.kid_advect_slab(_dev(st), _cu(u), _cu(w), _cu(rho), _cu(dz), dx, dt, nx, want=want, courant=courant))


def _rounded(out, T):
    """The reference in the inputs' dtype: binary64 on the widened inputs, rounded once."""
    res = {n: {k: v.astype(T) for k, v in out[n].items()} for n in ALL}
    res["courant"] = out["courant"].astype(T)
    return res


def _reference(st, w, rho, dz, dt=DT, keys=None):
    return _rounded(uref.advect(st, w, rho, dz, dt, keys), w.dtype.type)


def _reference_slab(st, u, w, rho, dz, nx, dt=DT, dx=DX, keys=None):
    return _rounded(uref.advect_slab(st, u, w, rho, dz, dx, dt, nx, keys), u.dtype.type)


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
    for n in ALL:
        if n in want and n in got:
            assert sorted(got[n]) == sorted(keys), (what, n, sorted(got[n]))
            for k in keys:
                _same(got[n][k], want[n][k], "%s %s[%s]" % (what, n, k))
    if "courant" in got and "courant" in want:
        _same(got["courant"], want["courant"], what + " courant")


def _reached(masks_by_member):
    return {n for m in masks_by_member.values() for n, a in m.items() if a.any()}


EVERY_BRANCH = set(uref.BRANCHES) | {"rising_quickest", "falling_quickest"}


# ---- 1. 1-D parity: the nz sweep ----
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
@pytest.mark.parametrize("nz", NZ_SWEEP)
def test_advect_equals_the_reference_bit_for_bit(ult, nz, dtype):
    st, w, rho, dz = cases.case(5, nz, dtype=dtype)
    full = uref.advect(st, w, rho, dz, DT)
    got = _advect(ult, st, w, rho, dz)
    want = _rounded(full, dtype)
    _same_result(got, want, "nz=%d" % nz)
    assert all(np.isfinite(want["sum"][k]).all() for k in ref.FIELDS) and np.abs(want["adv"]["qv"]).max() > 0
    wi = w[:, 1:nz]
    for what, there in (("+0", (wi == 0) & ~np.signbit(wi)), ("-0", (wi == 0) & np.signbit(wi)), ("c > 1", full["c"][:, 1:nz] > 1.0)):
        assert there.any(), what                                     # the planted faces are what they claim in this dtype
    if nz >= 8:
        assert ((wi[:, 1:] < 0) != (wi[:, :-1] < 0)).any(axis=1).all()
    if nz >= 63:
        assert EVERY_BRANCH <= _reached(full["branch"]), sorted(EVERY_BRANCH - _reached(full["branch"]))
        vl = ref.advect(st, w, rho, dz, DT)                          # and it is not the van Leer scheme that was run
        assert (_bits(want["adv"]["qv"]) != _bits(vl["adv"]["qv"].astype(dtype))).any()


# ---- 2. the ncol sweep: whole and partial workgroups; a column alone and inside a batch ----
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
@pytest.mark.parametrize("ncol", NCOL_SWEEP)
def test_ncol_sweep_and_column_independence(ult, ncol, dtype):
    st, w, rho, dz = cases.case(9, 65, seed=1, dtype=dtype)
    sub = {k: v[:ncol].copy() for k, v in st.items()}
    got = _advect(ult, sub, w[:ncol].copy(), rho, dz)
    _same_result(got, _reference(sub, w[:ncol].copy(), rho, dz), "ncol=%d" % ncol)
    c = ncol - 1                                                     # the last column alone, and moved to the front of a batch
    alone = _advect(ult, {k: v[c:c + 1].copy() for k, v in st.items()}, w[c:c + 1].copy(), rho, dz)
    order = [c] + [i for i in range(9) if i != c]
    moved = _advect(ult, {k: v[order].copy() for k, v in st.items()}, w[order].copy(), rho, dz)
    for n in ALL:
        for k in ref.FIELDS:
            _same(alone[n][k][0], got[n][k][c], "alone %s[%s]" % (n, k))
            _same(moved[n][k][0], got[n][k][c], "moved %s[%s]" % (n, k))
    _same(alone["courant"][0], got["courant"][c], "alone courant")
    _same(moved["courant"][0], got["courant"][c], "moved courant")


# ---- 3. slab parity ----
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
@pytest.mark.parametrize("nz", [2, 65, 129])
@pytest.mark.parametrize("nx", NX_SWEEP)
def test_advect_slab_equals_the_reference_bit_for_bit(ult, nx, nz, dtype):
    for nslab in (1, 2):
        st, u, w, rho, dz = cases.slab_case(nslab, nx, nz, dtype=dtype)
        assert (u > 0).any() and (u < 0).any() and (w > 0).any() and (w < 0).any()
        full = uref.advect_slab(st, u, w, rho, dz, DX, DT, nx)
        got = _advect_slab(ult, st, u, w, rho, dz, nx)
        _same_result(got, _rounded(full, dtype), "nx=%d nz=%d nslab=%d, a flow per slab" % (nx, nz, nslab))
        assert all(np.isfinite(full["sum"][k]).all() for k in ref.FIELDS)
        if nz >= 65 and nslab == 2:
            assert EVERY_BRANCH <= _reached(full["branch_x"]), sorted(EVERY_BRANCH - _reached(full["branch_x"]))
            assert (full["cx"] > 1.0).any() and ((u == 0) & np.signbit(u)).any() and ((u == 0) & ~np.signbit(u)).any()
        u1, w1 = u[:nx].copy(), w[:nx].copy()                        # [nx, ..]: one flow for every slab
        shared = _advect_slab(ult, st, u1, w1, rho, dz, nx)
        _same_result(shared, _reference_slab(st, u1, w1, rho, dz, nx), "nx=%d nz=%d nslab=%d, one flow" % (nx, nz, nslab))


@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
def test_slab_with_zero_u_is_the_1d_entry_as_a_number(ult, dtype):
    nx, nz = 5, 65
    st, u, w, rho, dz = cases.slab_case(2, nx, nz, seed=2, dtype=dtype)
    u0 = np.zeros_like(u)                                            # +0.0: rc = +inf in x, every x flux 0
    slab = _advect_slab(ult, st, u0, w, rho, dz, nx)
    one = _advect(ult, st, w, rho, dz)
    _same_result(slab, _reference_slab(st, u0, w, rho, dz, nx), "u = +0.0")
    for n in ALL:
        for k in ref.FIELDS:
            assert np.array_equal(slab[n][k], one[n][k]), (n, k)     # as numbers: a zero may differ in sign
    assert np.array_equal(slab["courant"], one["courant"])


# ---- 4. the aerosol entries ----
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
def test_aerosol_entries_equal_the_reference_on_the_three_members(ult_aero, dtype):
    m, nx, nz = ult_aero, 5, 65
    st, u, w, rho, dz = cases.slab_case(2, nx, nz, seed=3, dtype=dtype)
    aer = {"nc": st["nr"], "nwfa": st["ni"], "nifa": st["qv"]}      # sparse, many decades; qv holds the planted ramps
    got = _host(m.kid_advect_aero(_dev(aer), _cu(w), _cu(rho), _cu(dz), DT, want=ALL))
    want = _reference(aer, w, rho, dz, keys=AER)
    _same_result(got, want, "advect_aero", AER)
    got = _host(m.kid_advect_slab_aero(_dev(aer), _cu(u), _cu(w), _cu(rho), _cu(dz), DX, DT, nx, want=ALL))
    _same_result(got, _reference_slab(aer, u, w, rho, dz, nx, keys=AER), "advect_slab_aero", AER)
    vl = ref.advect(aer, w, rho, dz, DT, AER)
    assert (_bits(want["adv"]["nc"]) != _bits(vl["adv"]["nc"].astype(dtype))).any()


# ---- 5. the setting itself ----
def test_the_setting(gpu_mixed):
    from kid_amd import KidmpError, ThompsonMP
    from kid_amd.advection import library
    m, other = gpu_mixed, ThompsonMP(iiwarm=True)                    # a shared context that every test leaves at van Leer, and a new one
    L = library()
    st, w, rho, dz = cases.case(5, 65, seed=4)
    su, uu, wu, _, _ = cases.slab_case(1, 5, 65, seed=4)
    try:
        assert m.advection == "vanleer" and other.advection == "vanleer" and L.kidmp_advection(m._h) == 0
        before = _advect(m, st, w, rho, dz)
        before_slab = _advect_slab(m, su, uu, wu, rho, dz, 5)
        _same_result(before, ref.advect(st, w, rho, dz, DT), "a context that was never set is van Leer")
        assert m.set_advection("ultimate") == "ultimate" and m.advection == "ultimate" and L.kidmp_advection(m._h) == 1
        assert other.advection == "vanleer"                          # two contexts hold their settings independently
        ultimate = _advect(m, st, w, rho, dz)
        _same_result(ultimate, _reference(st, w, rho, dz), "after set_advection('ultimate')")
        warm = _advect(other, st, w, rho, dz)
        _same_result(warm, before, "the other context meanwhile", ref.WARM)
        other.set_advection("ultimate")
        m.set_advection("vanleer")
        assert m.advection == "vanleer" and other.advection == "ultimate"
        _same_result(_advect(other, st, w, rho, dz), ultimate, "the other context set to ultimate", ref.WARM)
        _same_result(_advect(m, st, w, rho, dz), before, "back to van Leer")
        _same_result(_advect_slab(m, su, uu, wu, rho, dz, 5), before_slab, "back to van Leer, slab")
        # a refused value changes nothing
        for bad in (2, -1, 7):
            assert L.kidmp_set_advection(other._h, bad) == -1        # KIDMP_EINVAL
            assert L.kidmp_advection(other._h) == 1 and b"kidmp_set_advection" in L.kidmp_last_error(other._h)
        with pytest.raises(KidmpError, match="unknown scheme"):
            other.set_advection("quickest")
        assert other.advection == "ultimate"
        _same_result(_advect(other, st, w, rho, dz), ultimate, "after the refusals", ref.WARM)
    finally:
        m.set_advection("vanleer")
        other.close()


# ---- 6. a chain ----
@pytest.mark.parametrize("dtype", [f64, f32], ids=["f64", "f32"])
def test_forty_steps_equal_the_reference_chain(ult, dtype):
    import torch
    ncol, nz, courant, dzv, dt = 3, 80, 0.4, 25.0, 10.0
    rng = np.random.Generator(np.random.PCG64(19900))
    st = {k: v.astype(dtype) for k, v in cases.fields(rng, ncol, nz).items()}
    st["qv"][:] = (np.exp(-0.5 * ((np.arange(nz)[None, :] - 20.0) / np.array([[2.0], [4.0], [8.0]])) ** 2) * 1.0e-2).astype(dtype)
    w = np.full(nz + 1, courant * dzv / dt).astype(dtype)
    w[0] = 0.0
    rho, dz = np.full(nz, 1.1).astype(dtype), np.full(nz, dzv).astype(dtype)
    d, dw, drho, ddz = _dev(st), _cu(w), _cu(rho), _cu(dz)
    out = None
    for _ in range(40):
        out = ult.kid_advect(d, dw, drho, ddz, dt, want="sum", courant=True, out=out)
        ult.kid_update(d, dt, out["sum"])
    torch.cuda.synchronize()
    x = {k: v.copy() for k, v in st.items()}
    for _ in range(40):
        r = uref.advect(x, w, rho, dz, dt)
        x = ref.update(x, dt, {k: v.astype(dtype) for k, v in r["sum"].items()})
    for k in ref.FIELDS:
        _same(d[k].cpu().numpy(), x[k], "forty steps: " + k)
    _same(out["courant"].cpu().numpy(), r["courant"].astype(dtype), "forty steps: courant")
    assert abs(float(r["courant"][0]) - courant) < 1e-6 and np.abs(x["qv"] - st["qv"]).max() > 1e-3
