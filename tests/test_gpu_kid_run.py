"""The device-resident 1-D KiD loop (kid_amd.kinematic.run, ThompsonMP.kid_run) on the MI355X.  -m gpu.

In binary64 `run` must equal, bit for bit, a step-by-step loop on numpy arrays: the reference advection
(tests/kid_advect_ref.py), the adapter's host entry (documented bit-equal to the device entry), the reference update.
Nothing here is a tolerance: the advection is pinned to the reference, and the update is plain arithmetic."""
import numpy as np
import pytest

import cases
import kid_advect_ref as ref

pytestmark = pytest.mark.gpu
P0, R_ON_CP, DT = 1.0e5, 287.058 / 1005.0, 10.0
NCOL = 5


def _kid_case(st):
    """KiD's theta-form fields of a batch of tests/cases.py, exner, and the profiles of dz and rho (column 0)."""
    exner = (st["p"] / P0) ** R_ON_CP
    F = {k: np.ascontiguousarray(st[k]) for k in ref.FIELDS[1:]}
    F["theta"] = np.ascontiguousarray(st["t"] / exner)
    rho = 0.622 * st["p"][0] / (287.04 * st["t"][0] * (st["qv"][0] + 0.622))
    return F, np.ascontiguousarray(exner), np.ascontiguousarray(st["dz"][0]), np.ascontiguousarray(rho)


def _w_base(nz, wmax, amps):
    """[ncol, nz+1]: wmax sin(pi z/z_top) on the faces, scaled per column."""
    f = np.arange(nz + 1) / float(nz)
    return np.ascontiguousarray(np.asarray(amps)[:, None] * (wmax * np.sin(np.pi * f))[None, :])


def _setup(kind):
    if kind == "warm":
        F, exner, dz, rho = _kid_case(cases.config2(NCOL))
        F = {k: F[k] for k in ref.WARM}
        nsteps, wmax = 12, 2.0
        scale = np.sin(np.pi * (np.arange(nsteps) + 0.5) / nsteps)
        scale[nsteps // 2] = 1.0                                     # Courant 2 * 10 / 25 = 0.8 at its largest
    else:
        F, exner, dz, rho = _kid_case(cases.config3(NCOL))
        nsteps, wmax = 6, 8.0
        scale = np.array([0.25, 0.5, 1.0, 1.0, 0.75, 0.5])            # Courant 8 * 10 / 125 = 0.64 at its largest
    w = _w_base(dz.shape[0], wmax, np.linspace(0.6, 1.0, NCOL))
    return F, exner, dz, rho, w, scale, nsteps


def _reference_loop(m, F, exner, dz, rho, w, scale, nsteps, fix_theta=False):
    """advect (numpy) -> kid_interface_host -> update (numpy); returns the states, ppt and courant of every step."""
    x = {k: v.copy() for k, v in F.items()}
    keys = list(F)
    states, ppts, cours = [], [], []
    for step in range(nsteps):
        a = ref.advect(x, w * scale[step], rho, dz, DT, keys)
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


@pytest.mark.parametrize("fix_theta", [False, True], ids=["theta-moves", "fix-theta"])
@pytest.mark.parametrize("kind", ["warm", "mixed"])
def test_run_equals_the_step_by_step_reference(ctxs, kind, fix_theta):
    import torch
    m = ctxs[kind]
    F, exner, dz, rho, w, scale, nsteps = _setup(kind)
    states, ppts, cours = _reference_loop(m, F, exner, dz, rho, w, scale, nsteps, fix_theta)
    assert max(c.max() for c in cours) == pytest.approx(0.8 if kind == "warm" else 0.64, rel=1e-12)

    state = {k: _cu(v) for k, v in F.items()}
    dw = _cu(w)
    seen = []

    def on_step(step, st, res):
        assert st is state and sorted(k for k in res if k in ref.FIELDS) == sorted(F)
        seen.append((step, st["qr"].clone(), st["theta"].clone(), res["ppt"].clone()))

    out, ppt, courant = m.kid_run(state, nsteps, DT, P0, R_ON_CP, _cu(exner), _cu(dz), _cu(rho), lambda step: dw * float(scale[step]),
                                  fix_theta=fix_theta, on_step=on_step)
    torch.cuda.synchronize()
    assert out is state
    for k in F:
        _same(state[k].cpu().numpy(), states[-1][k], "%s after %d steps: %s" % (kind, nsteps, k))
    if fix_theta:
        _same(state["theta"].cpu().numpy(), F["theta"], "theta stays")
    else:
        assert (states[-1]["theta"] != F["theta"]).any()
    # on_step: nsteps calls, each with the live state of its step
    assert [s[0] for s in seen] == list(range(nsteps))
    for step, qr, theta, p in seen:
        _same(qr.cpu().numpy(), states[step]["qr"], "qr at step %d" % step)
        _same(theta.cpu().numpy(), states[step]["theta"], "theta at step %d" % step)
        _same(p.cpu().numpy(), ppts[step], "ppt of step %d" % step)
    # the accumulated precipitation: the per-step ppt summed in the order of the steps
    acc = np.zeros_like(ppts[0])
    for p in ppts:
        acc = acc + p
    _same(ppt.cpu().numpy(), acc, "accumulated ppt")
    assert np.isfinite(acc).all() and (kind != "warm" or acc[:, 0].max() > 0)    # the warm column rains at the surface
    _same(courant.cpu().numpy(), cours[-1], "courant of the last step")
    assert any((states[i]["qr"] != states[i + 1]["qr"]).any() for i in range(nsteps - 1))


def test_run_with_a_fixed_w_tensor_and_shared_profile(ctxs):
    """w as a tensor [nz+1] (one profile for every column) instead of a callable; kid_amd.run itself."""
    import torch
    from kid_amd import run
    m = ctxs["warm"]
    F, exner, dz, rho, w, _, _ = _setup("warm")
    w1 = np.ascontiguousarray(w[-1])
    states, ppts, cours = _reference_loop(m, F, exner, dz, rho, w1, np.ones(3), 3)
    state = {k: _cu(v) for k, v in F.items()}
    _, ppt, courant = run(m, state, 3, DT, P0, R_ON_CP, _cu(exner), _cu(dz), _cu(rho), _cu(w1))
    torch.cuda.synchronize()
    for k in F:
        _same(state[k].cpu().numpy(), states[-1][k], k)
    _same(ppt.cpu().numpy(), (ppts[0] + ppts[1]) + ppts[2], "ppt")
    _same(courant.cpu().numpy(), cours[-1], "courant")
    with pytest.raises(Exception, match="kid_run"):
        run(m, state, 3, DT, P0, R_ON_CP, _cu(exner), _cu(dz), _cu(rho), _cu(w1), work=None)


@pytest.mark.parametrize("kind", ["warm", "mixed"])
def test_float32_run_equals_its_own_composition(ctxs, kind):
    """binary32 fields step in the native arithmetic (arith="p32n"): run is the three calls, step by step, bit for bit."""
    import torch
    m = ctxs[kind]
    F, exner, dz, rho, w, scale, nsteps = _setup(kind)
    nsteps = min(nsteps, 4)
    c32 = lambda a: _cu(a.astype(np.float32))   # noqa: E731
    dex, ddz, drho, dw = c32(exner), c32(dz), c32(rho), c32(w)
    wt = lambda step: dw * float(scale[step])   # noqa: E731

    state = {k: c32(v) for k, v in F.items()}
    _, ppt, courant = m.kid_run(state, nsteps, DT, P0, R_ON_CP, dex, ddz, drho, wt, arith="p32n")
    torch.cuda.synchronize()

    x = {k: c32(v) for k, v in F.items()}
    acc = torch.zeros(NCOL, 4, dtype=torch.float32, device="cuda:0")
    for step in range(nsteps):
        a = m.kid_advect(x, wt(step), drho, ddz, DT, want="sum", courant=True)
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
    assert np.isfinite(ppt.cpu().numpy()).all() and float(courant.max()) > 0
