"""The device-resident x-z KiD loop (kid_amd.slab.run_slab, ThompsonMP.kid_run_slab) on the MI355X.  -m gpu.

In binary64 `run_slab` must equal, bit for bit, a step-by-step loop on numpy arrays: the reference advection
(tests/kid_slab_ref.py), the adapter's host entry (documented bit-equal to the device entry), the reference update
(tests/kid_advect_ref.py).  Nothing here is a tolerance.  The flow is a stream function's, scaled per step, at a
reported courant of at most 0.5."""
import numpy as np
import pytest

import cases
import kid_advect_ref as ref
import kid_slab_ref as sref

pytestmark = pytest.mark.gpu
P0, R_ON_CP, DT = 1.0e5, 287.058 / 1005.0, 10.0


def _kid_case(st):
    """KiD's theta-form fields of a batch of tests/cases.py, exner, and the profiles of dz and rho (column 0)."""
    exner = (st["p"] / P0) ** R_ON_CP
    F = {k: np.ascontiguousarray(st[k]) for k in ref.FIELDS[1:]}
    F["theta"] = np.ascontiguousarray(st["t"] / exner)
    rho = 0.622 * st["p"][0] / (287.04 * st["t"][0] * (st["qv"][0] + 0.622))
    return F, np.ascontiguousarray(exner), np.ascontiguousarray(st["dz"][0]), np.ascontiguousarray(rho)


def _psi(nslab, nx, nz, amp):
    """[nslab*nx, nz+1]: one overturning cell pair per slab, a little stronger from slab to slab; zero at the ground."""
    x = (np.arange(nx) / float(nx))[None, :, None]
    f = (np.arange(nz + 1) / float(nz))[None, None, :]
    a = amp * np.linspace(1.0, 0.7, nslab)[:, None, None]
    return np.ascontiguousarray((a * np.sin(2.0 * np.pi * x + 0.4) * np.sin(np.pi * f)).reshape(nslab * nx, nz + 1))


def _setup(kind):
    if kind == "warm":
        nslab, nx, nsteps = 2, 5, 6
        F, exner, dz, rho = _kid_case(cases.config2(nslab * nx))
        F = {k: F[k] for k in ref.WARM}
        scale = np.array([0.4, 0.7, 1.0, 1.0, 0.8, 0.5])
    else:
        nslab, nx, nsteps = 1, 4, 3
        F, exner, dz, rho = _kid_case(cases.config3(nslab * nx))
        scale = np.array([0.5, 1.0, 0.75])
    dx = 4.0 * float(dz.mean())
    nz = dz.shape[0]
    # the stream function's size: the unsplit courant number of the strongest step comes out at 0.45
    u, w = sref.streamfunction_flow(_psi(nslab, nx, nz, 1.0), rho, dz, dx, nx)
    one = sref.advect_slab({"qv": F["qv"]}, u, w, rho, dz, dx, DT, nx)["courant"].max()
    psi = _psi(nslab, nx, nz, 0.45 / one)
    return F, exner, dz, rho, dx, nx, psi, scale, nsteps


def _reference_loop(m, F, exner, dz, rho, dx, nx, u, w, scale, nsteps, fix_theta=False):
    """advect_slab (numpy) -> kid_interface_host -> update (numpy); returns the states, ppt and courant of every step."""
    x = {k: v.copy() for k, v in F.items()}
    keys = list(F)
    states, ppts, cours = [], [], []
    for step in range(nsteps):
        a = sref.advect_slab(x, u * scale[step], w * scale[step], rho, dz, dx, DT, nx, keys)
        res = m.kid_interface_host(x, DT, P0, R_ON_CP, exner, dz, adv=a["sum"])
        moved = [k for k in keys if not (fix_theta and k == "theta")]
        new = ref.update(x, DT, a["sum"], res, keys=moved)
        x = dict(x, **new)
        states.append({k: v.copy() for k, v in x.items()})
        ppts.append(res["ppt"].copy())
        cours.append(a["courant"])
    return states, ppts, cours


def _cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    diff = _bits(a) != _bits(b)
    assert not diff.any(), "%s: %d of %d elements differ, first at %s: %r vs %r" % (
        what, int(diff.sum()), diff.size, np.argwhere(diff)[0], a[tuple(np.argwhere(diff)[0])], b[tuple(np.argwhere(diff)[0])])


@pytest.fixture
def ctxs(gpu_warm, gpu_mixed):
    yield {"warm": gpu_warm, "mixed": gpu_mixed}
    for m in (gpu_warm, gpu_mixed):
        m.set_host_chunk(0)


@pytest.mark.parametrize("kind", ["warm", "mixed"])
def test_run_slab_equals_the_step_by_step_reference(ctxs, kind):
    import torch
    from kid_amd import streamfunction_flow
    m = ctxs[kind]
    F, exner, dz, rho, dx, nx, psi, scale, nsteps = _setup(kind)
    drho, ddz = _cu(rho), _cu(dz)
    du, dw = streamfunction_flow(_cu(psi), drho, ddz, dx, nx=nx)
    torch.cuda.synchronize()
    u, w = sref.streamfunction_flow(psi, rho, dz, dx, nx)
    _same(du.cpu().numpy(), u, "streamfunction_flow u")              # division for division the restatement's
    _same(dw.cpu().numpy(), w, "streamfunction_flow w")
    assert (u > 0).any() and (u < 0).any() and (w > 0).any() and (w < 0).any()
    states, ppts, cours = _reference_loop(m, F, exner, dz, rho, dx, nx, u, w, scale, nsteps)
    top = max(c.max() for c in cours)
    assert 0.4 < top <= 0.5, top

    state = {k: _cu(v) for k, v in F.items()}
    seen = []

    def on_step(step, st, res):
        assert st is state and sorted(k for k in res if k in ref.FIELDS) == sorted(F)
        seen.append((step, st["qr"].clone(), st["theta"].clone(), res["ppt"].clone()))

    out, ppt, courant = m.kid_run_slab(state, nsteps, DT, P0, R_ON_CP, _cu(exner), ddz, drho, dx, nx,
                                       lambda step: du * float(scale[step]), lambda step: dw * float(scale[step]), on_step=on_step)
    torch.cuda.synchronize()
    assert out is state
    for k in F:
        _same(state[k].cpu().numpy(), states[-1][k], "%s after %d steps: %s" % (kind, nsteps, k))
    assert (states[-1]["theta"] != F["theta"]).any()
    assert [s[0] for s in seen] == list(range(nsteps))               # on_step sees every step, with the live state of its step
    for step, qr, theta, p in seen:
        _same(qr.cpu().numpy(), states[step]["qr"], "qr at step %d" % step)
        _same(theta.cpu().numpy(), states[step]["theta"], "theta at step %d" % step)
        _same(p.cpu().numpy(), ppts[step], "ppt of step %d" % step)
    acc = np.zeros_like(ppts[0])
    for p in ppts:
        acc = acc + p
    _same(ppt.cpu().numpy(), acc, "accumulated ppt")
    _same(courant.cpu().numpy(), cours[-1], "courant of the last step")
    assert float(courant.max()) <= 0.5 and np.isfinite(acc).all()
    assert any((states[i]["qr"] != states[i + 1]["qr"]).any() for i in range(nsteps - 1))
    # the x direction took part: the columns of a slab no longer move alike
    nocross = sref.advect_slab(F, np.zeros_like(u), w * scale[0], rho, dz, dx, DT, nx, list(F))["sum"]["qv"]
    cross = sref.advect_slab(F, u * scale[0], w * scale[0], rho, dz, dx, DT, nx, list(F))["sum"]["qv"]
    assert (nocross != cross).any()


def test_run_slab_with_fixed_tensors_shared_flow_and_fix_theta(ctxs):
    """u and w as tensors [nx, ..] shared by both slabs instead of callables; kid_amd.run_slab itself; theta held."""
    import torch
    from kid_amd import run_slab
    m = ctxs["warm"]
    F, exner, dz, rho, dx, nx, psi, _, _ = _setup("warm")
    u, w = sref.streamfunction_flow(psi[:nx], rho, dz, dx)
    states, ppts, cours = _reference_loop(m, F, exner, dz, rho, dx, nx, u, w, np.ones(2), 2, fix_theta=True)
    state = {k: _cu(v) for k, v in F.items()}
    _, ppt, courant = run_slab(m, state, 2, DT, P0, R_ON_CP, _cu(exner), _cu(dz), _cu(rho), dx, nx, _cu(u), _cu(w), fix_theta=True)
    torch.cuda.synchronize()
    for k in F:
        _same(state[k].cpu().numpy(), states[-1][k], k)
    _same(state["theta"].cpu().numpy(), F["theta"], "theta stays")
    _same(ppt.cpu().numpy(), ppts[0] + ppts[1], "ppt")
    _same(courant.cpu().numpy(), cours[-1], "courant")
    with pytest.raises(Exception, match="kid_run_slab"):
        run_slab(m, state, 2, DT, P0, R_ON_CP, _cu(exner), _cu(dz), _cu(rho), dx, nx, _cu(u), _cu(w), work=None)


@pytest.mark.parametrize("kind", ["warm", "mixed"])
def test_float32_run_slab_equals_its_own_composition(ctxs, kind):
    """binary32 fields step in the native arithmetic (arith="p32n"): run_slab is the three calls, step by step, bit for bit."""
    import torch
    m = ctxs[kind]
    F, exner, dz, rho, dx, nx, psi, scale, nsteps = _setup(kind)
    nsteps = min(nsteps, 3)
    u, w = sref.streamfunction_flow(psi, rho, dz, dx, nx)
    c32 = lambda a: _cu(a.astype(np.float32))   # noqa: E731
    dex, ddz, drho, du, dw = c32(exner), c32(dz), c32(rho), c32(u), c32(w)
    ut = lambda step: du * float(scale[step])   # noqa: E731
    wt = lambda step: dw * float(scale[step])   # noqa: E731
    ncol = du.shape[0]

    state = {k: c32(v) for k, v in F.items()}
    _, ppt, courant = m.kid_run_slab(state, nsteps, DT, P0, R_ON_CP, dex, ddz, drho, dx, nx, ut, wt, arith="p32n")
    torch.cuda.synchronize()

    x = {k: c32(v) for k, v in F.items()}
    acc = torch.zeros(ncol, 4, dtype=torch.float32, device="cuda:0")
    for step in range(nsteps):
        a = m.kid_advect_slab(x, ut(step), wt(step), drho, ddz, dx, DT, nx, want="sum", courant=True)
        res = m.kid_interface(x, DT, P0, R_ON_CP, dex, ddz, adv=a["sum"], arith="p32n")
        m.kid_update(x, DT, a["sum"], {k: res[k] for k in F})
        acc = acc + res["ppt"]
    torch.cuda.synchronize()
    for k in F:
        assert state[k].dtype == torch.float32
        _same(state[k].cpu().numpy(), x[k].cpu().numpy(), "%s float32: %s" % (kind, k))
    assert all((state[k].cpu().numpy() != F[k].astype(np.float32)).any() for k in ("theta", "qv", "qr"))
    _same(ppt.cpu().numpy(), acc.cpu().numpy(), "ppt")
    _same(courant.cpu().numpy(), a["courant"].cpu().numpy(), "courant")
    assert np.isfinite(ppt.cpu().numpy()).all() and 0 < float(courant.max()) <= 0.5
