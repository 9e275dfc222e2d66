"""The advection setting (include/kidmp_advection.h, kid_amd/advection.py) without a GPU: the two symbols exist in the built
library and in the new header only, kid_amd/advection.py declares them as the header has them and no other mirror does, the
header compiles as C99 and C++11, a missing context is refused, an unknown scheme is refused before the library is reached,
and the numpy reference of the GPU tests (tests/kid_ultimate_ref.py) has the scheme's properties:

  telescoping      SUM_k den[k]*adv[k] = F[0] - F[nz] within 8 nz eps max|F|: the flux form is the van Leer scheme's, so the
                   bound is that of tests/test_kid_advect_abi.py (four roundings per term of a quantity bounded by 2 max|F|)
  constant fields  |adv + div| <= 4 eps max|M| |q| / min(den), as there: every face value of a constant field is q exactly
                   (b*dq = 0: the first-order fallback)
  finite           exact +0.0 and -0.0 faces (rc = +inf) and faces with c > 1 give finite outputs
  bounded          uniform one-signed flow at Courant 0.1, 0.5, 0.9: over 20 steps of q + dt*sum every cell stays inside the
                   range of its three-cell neighbourhood of the step before -- both the upwind one (the cell and its two
                   upwind neighbours) and the centred one -- up to 4 ulp of the field's maximum.  The universal limiter puts a
                   face value between its upwind and downwind cells and below ref, which bounds the updated cell by its
                   upwind neighbour and itself in exact arithmetic; the allowance is for the roundings of flux and update
  zero             a zero field stays zero
  accuracy         a Gaussian of width 0.08 advected 0.3 domain lengths on a uniform grid with uniform w, L1 error against
                   the exact solution (the translate, and the constant inflow below it), at Courant 0.1, 0.4, 0.8: the
                   observed order between n = 40 and n = 160 is >= 2.5, and the error at n = 160 is at most a quarter of
                   the van Leer scheme's (tests/kid_advect_ref.py)
  branches         the inputs of the GPU tests (tests/kid_ultimate_cases.py) reach the first-order fallback, both downwind
                   clamps (the reference value and the downwind cell) of the rising and of the falling case, and QUICKEST
                   itself, in z and in x: the bit tests of tests/test_gpu_kid_ultimate.py cannot miss a branch
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kid_advect_ref as ref
import kid_ultimate_cases as cases
import kid_ultimate_ref as uref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_advection.h")
SYMBOLS = ("kidmp_set_advection", "kidmp_advection")
EPS = np.finfo(np.float64).eps
ESTATE = -5

SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "size_t": (C.c_size_t,), "double": (C.c_double,),
           "float": (C.c_float,), "int": (C.c_int, C.c_int32)}


def _code(path=HEADER):
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes(path=HEADER):
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of a header (the method of
    test_kid_advect_abi.py)."""
    text = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", " ", _code(path), flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([\w \t\n\*]+?)\b(kidmp(?:32)?_\w+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        out[name] = (" ".join(ret.split()), [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    return out


class _Entry:
    restype = "never set"
    argtypes = None


class _Stub:
    def __init__(self):
        self.entries = {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self.entries.setdefault(name, _Entry())


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_symbols_are_exported_and_prototyped_in_the_new_header_only():
    lib = os.path.join(ROOT, "kid_amd", "libkidmp.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(lib)
    protos = _prototypes()
    assert sorted(protos) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    text = open(HEADER).read()
    assert '#include "kidmp.h"' in text
    values = dict(re.findall(r"#define\s+(KIDMP_ADVECT_\w+)\s+(\d+)", text))
    assert values == {"KIDMP_ADVECT_VANLEER": "0", "KIDMP_ADVECT_ULTIMATE": "1"}
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):
        if other.endswith(".h") and other != "kidmp_advection.h":
            assert not set(SYMBOLS) & set(_prototypes(os.path.join(inc, other))), other
            assert "KIDMP_ADVECT_" not in _code(os.path.join(inc, other)), other


def test_the_python_declarations_match_the_header():
    import kid_amd
    import kid_amd.advection as ka
    declared = ka.declare(_Stub()).entries
    protos = _prototypes()
    assert sorted(declared) == sorted(protos)
    wrong = []
    for name, (ret, params) in sorted(protos.items()):
        e = declared[name]
        if len(e.argtypes) != len(params):
            wrong.append("%s: %d arguments declared, the header has %d" % (name, len(e.argtypes), len(params)))
            continue
        for i, (p, t) in enumerate(zip(params, e.argtypes)):
            ok = _is_pointer(t) if "*" in p else t in SCALARS[re.sub(r"\bconst\b", "", p).split()[0]]
            if not ok:
                wrong.append("%s: argument %d is `%s`, declared %s" % (name, i, p, getattr(t, "__name__", t)))
        if e.restype not in SCALARS[ret]:
            wrong.append("%s: returns `%s`, declared %s" % (name, ret, getattr(e.restype, "__name__", e.restype)))
    assert not wrong, "\n".join(wrong)
    assert ka.SCHEMES == ("vanleer", "ultimate") and kid_amd.ADVECTION_SCHEMES is ka.SCHEMES
    assert callable(kid_amd.ThompsonMP.set_advection) and isinstance(kid_amd.ThompsonMP.advection, property)


def test_the_other_mirrors_do_not_declare_them():
    import kid_amd.aerosol as ae
    import kid_amd.doppler as dp
    import kid_amd.fall as fl
    import kid_amd.kinematic as kk
    import kid_amd.slab as ks
    import kid_amd.spectra as sp
    import kid_amd.stats as st
    import kid_amd.summary as sm
    import kid_amd.thompson as th
    for other in (th, st, sm, fl, dp, kk, ks, sp, ae):
        assert not set(SYMBOLS) & set(other._declarations()), other.__name__


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_advection.h"\n'
                   "int use(kidmp_ctx *c)\n"
                   "{ return kidmp_set_advection(c, KIDMP_ADVECT_ULTIMATE) + kidmp_set_advection(c, KIDMP_ADVECT_VANLEER) + kidmp_advection(c); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.advection import library
    L = library()
    assert L.kidmp_set_advection(None, 0) == ESTATE
    assert L.kidmp_set_advection(None, 1) == ESTATE
    assert L.kidmp_set_advection(None, 7) == ESTATE
    assert L.kidmp_advection(None) == ESTATE
    assert b"kidmp_advection" in L.kidmp_last_error(None)


# ---- an unknown scheme is refused before the library is reached ----
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called")


def _bare():
    from kid_amd import ThompsonMP
    m = ThompsonMP.__new__(ThompsonMP)                      # no kidmp_init: there is no device here
    m._h = None
    m.device = 0
    m.iiwarm = False
    return m


@pytest.mark.parametrize("name", ["quickest", "ULTIMATE", "", None, 1, 0, ("ultimate",), b"ultimate"], ids=repr)
def test_unknown_schemes_are_refused_before_the_library(name, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd.advection import set_scheme
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="set_advection: unknown scheme"):
        set_scheme(_bare(), name)
    with pytest.raises(th.KidmpError, match="vanleer, ultimate"):
        _bare().set_advection(name)


def test_a_missing_context_is_an_error_in_python_too():
    from kid_amd import KidmpError
    with pytest.raises(KidmpError, match="kidmp error -5"):
        _bare().set_advection("ultimate")
    with pytest.raises(KidmpError, match="kidmp error -5"):
        _bare().advection


# ---- the properties of the reference ----
def _profiles(rng, nz):
    rho = 1.2 * np.exp(-np.linspace(0.0, 1.1, nz)) * rng.uniform(0.97, 1.03, nz)
    dz = rng.uniform(20.0, 60.0, nz)
    return rho, dz


def _w_with_sign_change(rng, ncol, nz):
    """[ncol, nz+1]: both signs, a sign change inside every column, w[0] = 0 (tests/test_kid_advect_abi.py's)."""
    f = np.linspace(0.0, 1.0, nz + 1)[None, :]
    w = rng.uniform(0.5, 3.0, (ncol, 1)) * np.sin(np.pi * rng.integers(1, 4, (ncol, 1)) * 2.0 * f + rng.uniform(0.1, 3.0, (ncol, 1)))
    w += rng.normal(0.0, 0.2, w.shape)
    w[:, 0] = 0.0
    flip = nz // 2 + 1
    w[:, flip] = -np.abs(w[:, flip]) - 0.1
    w[:, flip - 1] = np.abs(w[:, flip - 1]) + 0.1
    return w


@pytest.mark.parametrize("nz", [3, 65, 129])
def test_reference_flux_form_telescopes(nz):
    rng = np.random.Generator(np.random.PCG64(19100 + nz))
    ncol = 200
    q = 10.0 ** rng.uniform(-12.0, 9.0, (ncol, nz)) * (rng.random((ncol, nz)) < 0.5)
    rho, dz = _profiles(rng, nz)
    w = _w_with_sign_change(rng, ncol, nz)
    assert ((w[:, 1:] < 0) != (w[:, :-1] < 0)).any(axis=1).all() and (q == 0).mean() > 0.3
    out = uref.advect({"qv": q}, w, rho, dz, 2.0)
    F, adv = out["F"]["qv"], out["adv"]["qv"]
    total = np.sum(out["den"][None, :] * adv, axis=1)
    resid = np.abs(total - (F[:, 0] - F[:, nz]))
    bound = 8 * nz * EPS * np.abs(F).max(axis=1)
    print("telescoping nz=%d: worst residual / bound = %.3g" % (nz, float(np.max(resid / np.maximum(bound, 1e-300)))))
    assert np.isfinite(adv).all() and (np.abs(F).max(axis=1) > 0).mean() > 0.5
    assert (resid <= bound).all()


@pytest.mark.parametrize("nz", [3, 65, 129])
def test_reference_leaves_a_constant_field_constant(nz):
    rng = np.random.Generator(np.random.PCG64(19200 + nz))
    ncol = 200
    qc = 10.0 ** rng.uniform(-12.0, 9.0, (ncol, 1))
    q = np.ascontiguousarray(np.broadcast_to(qc, (ncol, nz)))
    rho, dz = _profiles(rng, nz)
    w = _w_with_sign_change(rng, ncol, nz)
    out = uref.advect({"qv": q}, w, rho, dz, 2.0)
    assert out["branch"]["qv"]["upwind"].all()
    bound = 4 * EPS * np.abs(out["M"]).max(axis=1, keepdims=True) * np.abs(qc) / out["den"].min()
    resid = np.abs(out["sum"]["qv"])
    print("constant field nz=%d: worst residual / bound = %.3g" % (nz, float(np.max(resid / bound))))
    assert (np.abs(out["adv"]["qv"]) > 0).any()                                  # the flux form alone does move it
    assert (resid <= bound).all()


@pytest.mark.parametrize("nz", [3, 65, 129])
def test_reference_is_finite_at_zero_faces_and_beyond_courant_one(nz):
    rng = np.random.Generator(np.random.PCG64(19300 + nz))
    ncol, dt = 402, 2.0                                                          # many: at nz = 3 few faces have a second upwind cell
    q = 10.0 ** rng.uniform(-12.0, 9.0, (ncol, nz)) * (rng.random((ncol, nz)) < 0.6)
    q[::2] = np.cumsum(10.0 ** rng.uniform(-3.0, 3.0, q[::2].shape), axis=1)     # strictly monotone columns: the limiter acts
    q[::4] = q[::4, ::-1]
    rho, dz = _profiles(rng, nz)
    w = _w_with_sign_change(rng, ncol, nz)
    kind = rng.integers(0, 4, w.shape)
    w[kind == 0] = 0.0
    w[kind == 1] = -0.0
    w[kind == 2] *= 40.0 * rng.choice([-1.0, 1.0], w.shape)[kind == 2]           # c up to 40 * 3.5 * 2 / 20, either way
    out = uref.advect({"qv": q}, w, rho, dz, dt)
    c = out["c"][:, 1:nz]
    zero = w[:, 1:nz] == 0.0
    assert (zero & ~np.signbit(w[:, 1:nz])).any() and (zero & np.signbit(w[:, 1:nz])).any() and (c > 1.0).any() and (c == 0.0).any()
    limited = ~out["branch"]["qv"]["upwind"]
    assert (limited & zero).any() and (limited & (c > 1.0)).any()                # not only through the fallback
    for n in ("adv", "div", "sum", "F"):
        assert np.isfinite(out[n]["qv"]).all(), n
    assert not out["F"]["qv"][:, 1:nz][zero].any()                               # and a zero face carries nothing
    # the same in x
    nx = 6
    u = rng.uniform(-3.0, 3.0, (ncol // nx * nx, nz))
    kind = rng.integers(0, 4, u.shape)
    u[kind == 0] = 0.0
    u[kind == 1] = -0.0
    u[kind == 2] *= 400.0
    sl = uref.advect_slab({"qv": q[:u.shape[0]]}, u, w[:u.shape[0]], rho, dz, 150.0, dt, nx)
    assert (sl["cx"] > 1.0).any() and (~sl["branch_x"]["qv"]["upwind"] & (sl["cx"] == 0.0)).any()
    for n in ("adv", "div", "sum", "Fx"):
        assert np.isfinite(sl[n]["qv"]).all(), n


def _bounded_fields(rng, ncol, nz):
    """Random sparse fields <= 1, steps and peaks."""
    q = 10.0 ** rng.uniform(-6.0, 0.0, (ncol, nz)) * (rng.random((ncol, nz)) < 0.6)
    q[:10] = (np.arange(nz)[None, :] > np.linspace(3, nz - 4, 10).astype(int)[:, None]) * 1.0      # steps
    q[10:20] = np.exp(-0.5 * ((np.arange(nz)[None, :] - nz / 2.0) / np.arange(1, 11)[:, None]) ** 2)   # peaks of every width
    return q


@pytest.mark.parametrize("nz", [3, 65, 129])
@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["up", "down"])
@pytest.mark.parametrize("courant", [0.1, 0.5, 0.9])
def test_reference_stays_inside_the_three_cell_range_over_20_steps(courant, sign, nz):
    rng = np.random.Generator(np.random.PCG64(19400 + nz))
    ncol, dzv, dt = 60, 25.0, 10.0
    q = _bounded_fields(rng, ncol, nz)
    w = np.full(nz + 1, sign * courant * dzv / dt)
    rho, dz = np.full(nz, 1.1), np.full(nz, dzv)
    tol = 4 * EPS * q.max()
    worst = 0.0
    for step in range(20):
        out = uref.advect({"qv": q}, w, rho, dz, dt)
        assert not out["div"]["qv"].any()                                        # uniform M: no divergence at all
        new = q + dt * out["sum"]["qv"]
        if nz >= 4:
            k = np.arange(2, nz - 2)                                             # cells whose neighbours k-2 .. k+2 all exist
            s = -1 if sign > 0 else 1                                            # towards the upwind side
            for hood in ((k + 2 * s, k + s, k), (k - 1, k, k + 1)):
                lo = np.minimum.reduce([q[:, i] for i in hood])
                hi = np.maximum.reduce([q[:, i] for i in hood])
                worst = max(worst, float(np.max(lo - new[:, k], initial=0.0)), float(np.max(new[:, k] - hi, initial=0.0)))
        worst = max(worst, float(np.max(q.min(axis=1) - new.min(axis=1))), float(np.max(new.max(axis=1) - q.max(axis=1))))
        q = new
    print("bounded c=%g sign=%+g nz=%d: worst excursion %.3g = %.2f ulp of the maximum (allowed 4)" % (courant, sign, nz, worst, worst / (tol / 4)))
    assert np.all(np.abs(out["courant"] - courant) <= 4 * EPS)
    assert worst <= tol


@pytest.mark.parametrize("nz", [3, 65, 129])
def test_reference_keeps_a_zero_field_zero(nz):
    rng = np.random.Generator(np.random.PCG64(19500 + nz))
    rho, dz = _profiles(rng, nz)
    w = _w_with_sign_change(rng, 20, nz)
    w[:, 1] = 0.0
    out = uref.advect({"qv": np.zeros((20, nz))}, w, rho, dz, 2.0)
    for n in ("adv", "div", "sum"):
        assert not out[n]["qv"].any(), n


# ---- accuracy ----
def _l1_after_translation(advect, n, courant, width=0.08, distance=0.3, x0=0.35):
    """L1 error of a Gaussian advected `distance` domain lengths upwards on n uniform cells of a unit domain, against the
    exact solution of the problem the entry solves: the lower boundary face carries q[0] (zero gradient), and q[0] never
    changes under upward flow, so what has entered by the end is the constant g(x[0]) and the rest is the translate.
    (Against the translate on an infinite line the inflow's error, the size of the tail g(0) = 7e-5, would sit in the L1
    norm beside a scheme error of 4e-5 .. 1e-4 at n = 160 and be mistaken for it.)"""
    dzv, wv = 1.0 / n, 1.0
    dt = courant * dzv / wv
    nsteps = int(round(distance / (wv * dt)))
    assert abs(nsteps * wv * dt - distance) < 1e-12
    x = (np.arange(n) + 0.5) * dzv
    q = np.exp(-0.5 * ((x - x0) / width) ** 2)[None, :]
    w, rho, dz = np.full(n + 1, wv), np.ones(n), np.full(n, dzv)
    for _ in range(nsteps):
        q = q + dt * advect({"qv": q}, w, rho, dz, dt)["sum"]["qv"]
    origin = np.maximum(x - distance, x[0])                                      # where the cell's content started
    exact = np.exp(-0.5 * ((origin - x0) / width) ** 2)
    return float(np.abs(q[0] - exact).sum() * dzv)


@pytest.mark.parametrize("courant", [0.1, 0.4, 0.8])
def test_ultimate_is_third_order_on_a_uniform_grid_and_beats_van_leer(courant):
    eu = {n: _l1_after_translation(uref.advect, n, courant) for n in (40, 160)}
    ev = {n: _l1_after_translation(ref.advect, n, courant) for n in (40, 160)}
    order_u = np.log(eu[40] / eu[160]) / np.log(4.0)
    order_v = np.log(ev[40] / ev[160]) / np.log(4.0)
    print("accuracy c=%g: ULTIMATE L1 %.3e -> %.3e (order %.2f), van Leer %.3e -> %.3e (order %.2f), van Leer / ULTIMATE at 160: %.2f"
          % (courant, eu[40], eu[160], order_u, ev[40], ev[160], order_v, ev[160] / eu[160]))
    assert order_u >= 2.5
    assert eu[160] <= 0.25 * ev[160]


# ---- the inputs of the GPU tests reach every branch ----
def _reached(masks_by_member):
    return {n for m in masks_by_member.values() for n, a in m.items() if a.any()}


@pytest.mark.parametrize("dtype", [cases.f64, cases.f32], ids=["f64", "f32"])
def test_the_gpu_cases_reach_every_branch(dtype):
    want = set(uref.BRANCHES) | {"rising_quickest", "falling_quickest"}
    st, w, rho, dz = cases.case(5, 65, dtype=dtype)
    out = uref.advect(st, w, rho, dz, cases.DT)
    assert want <= _reached(out["branch"]), sorted(want - _reached(out["branch"]))
    c = out["c"][:, 1:65]
    wi = w[:, 1:65]
    assert ((wi == 0) & ~np.signbit(wi)).any(axis=1).all() and ((wi == 0) & np.signbit(wi)).any(axis=1).all()
    assert (c > 1.0).any(axis=1).all() and (c == 1.0).any(axis=1).all()
    assert ((wi[:, 1:] < 0) != (wi[:, :-1] < 0)).any(axis=1).all()
    limited = ~out["branch"]["qv"]["upwind"]
    assert (limited & (c > 1.0)).any() and (limited & (c == 1.0)).any()           # the planted faces meet the limiter
    assert all((v == 0).mean() > 0.25 for k, v in st.items() if k != "theta")
    st, u, w, rho, dz = cases.slab_case(2, 5, 65, dtype=dtype)
    sl = uref.advect_slab(st, u, w, rho, dz, cases.DX, cases.DT, 5)
    assert want <= _reached(sl["branch"]) and want <= _reached(sl["branch_x"]), sorted(want - _reached(sl["branch_x"]))
    assert ((u == 0) & ~np.signbit(u)).any() and ((u == 0) & np.signbit(u)).any() and (sl["cx"] == 1.5).any()
    assert (u > 0).any() and (u < 0).any()
