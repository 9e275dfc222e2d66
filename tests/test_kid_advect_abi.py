"""The kinematic entries (include/kidmp_kinematic.h, kid_amd/kinematic.py) without a GPU: the four symbols exist in the
built library and in the new header, kid_amd/kinematic.py declares them as the header has them, the header compiles as C99
and C++11, a missing context is refused, the Python wrappers turn wrong arguments away before the library is called, and
the numpy reference of the GPU tests (tests/kid_advect_ref.py) has the scheme's three properties, each within a bound
derived from the number of roundings involved (none is a measured number):

  telescoping      SUM_k den[k]*adv[k] = F[0] - F[nz] within 8 nz eps max|F|: each term is recovered through at most four
                   roundings (the difference, the division, the product, the running sum) of a quantity bounded by 2 max|F|
  constant fields  |adv + div| <= 4 eps max|M| |q| / min(den): F = M q exactly rounded once per face, two faces per cell,
                   one rounding in each of the two quotients
  monotonicity     for uniform w, rho, dz at Courant <= 0.9: q + dt*sum stays within the minimum and maximum of the cell
                   and its two neighbours (interior cells, up to 4 eps max|q|) and q + dt*adv >= 0
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kid_advect_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_kinematic.h")
SYMBOLS = ("kidmp_kid_advect_device", "kidmp32_kid_advect_device", "kidmp_kid_update_device", "kidmp32_kid_update_device")
EPS = np.finfo(np.float64).eps

SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "size_t": (C.c_size_t,), "double": (C.c_double,),
           "float": (C.c_float,), "int": (C.c_int, C.c_int32)}


def _code():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes():
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of the header (the method of
    test_column_summary_abi.py)."""
    text = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", " ", _code(), flags=re.M)
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


def test_symbols_are_exported_and_prototyped():
    lib = os.path.join(ROOT, "kid_amd", "libkidmp.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(lib)
    protos = _prototypes()
    assert sorted(protos) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert '#include "kidmp.h"' in open(HEADER).read()
    assert "_host" not in " ".join(protos)                                   # no host-array entries: the header says why


def test_the_python_declarations_match_the_header():
    import kid_amd
    import kid_amd.kinematic as kk
    declared = kk.declare(_Stub()).entries
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
            if "kid_fields" in p and t is not C.POINTER(kid_amd.thompson._KidFields):
                wrong.append("%s: argument %d is `%s`, declared %s" % (name, i, p, getattr(t, "__name__", t)))
        if e.restype not in SCALARS[ret]:
            wrong.append("%s: returns `%s`, declared %s" % (name, ret, getattr(e.restype, "__name__", e.restype)))
    assert not wrong, "\n".join(wrong)
    assert kid_amd.KID_FIELDS == ref.FIELDS and kid_amd.ADVECT_OUTPUTS == ("adv", "div", "sum")
    assert kid_amd.advect is kk.advect and kid_amd.update is kk.update and kid_amd.run is kk.run
    for name in ("kid_advect", "kid_update", "kid_run"):
        assert callable(getattr(kid_amd.ThompsonMP, name))


def test_the_other_mirrors_do_not_declare_them():
    import kid_amd.doppler as dp
    import kid_amd.fall as fl
    import kid_amd.stats as st
    import kid_amd.summary as sm
    import kid_amd.thompson as th
    for other in (th, st, sm, fl, dp):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_kinematic.h"\n'
                   "int use(kidmp_ctx *c, const double *a, double *o, const kidmp_kid_fields *f)\n"
                   "{ return kidmp_kid_advect_device(c, 1, 2, 1.0, f, a, 0, a, a, f, f, f, o, 0)\n"
                   "       + kidmp_kid_update_device(c, 1, 2, 1.0, f, f, f, f, 1, 0); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.kinematic import library
    from kid_amd.thompson import _KidFields
    L = library()
    f = C.byref(_KidFields())
    advect = [None, 4, 120, 10.0, f, None, 0, None, None, f, f, f, None, None]
    update = [None, 4, 120, 10.0, f, f, f, f, 1, None]
    assert L.kidmp_kid_advect_device(*advect) == -5                              # KIDMP_ESTATE
    assert L.kidmp32_kid_advect_device(*advect) == -5
    assert L.kidmp_kid_update_device(*update) == -5
    assert L.kidmp32_kid_update_device(*update) == -5


# ---- the wrappers refuse wrong input before the library is reached ----
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


N, NZ = 6, 40


def _good(dt=None, nz=NZ, n=N):
    import torch
    dt = dt or torch.float64
    st = {k: torch.zeros(n, nz, dtype=dt) for k in ref.FIELDS}
    return st, dict(w=torch.zeros(nz + 1, dtype=dt), rho=torch.ones(nz, dtype=dt), dz=torch.ones(nz, dtype=dt), dt=1.0)


def _advect_cases():
    """Host tensors throughout: each case is wrong in one way and, being host memory, on the wrong device as well."""
    import torch
    st, kw = _good()
    f16 = _good(torch.float16)
    return [
        ("host memory", st, kw),
        ("not a dict", [torch.zeros(N, NZ, dtype=torch.float64)], kw),
        ("numpy for torch", {k: np.zeros((N, NZ)) for k in ref.FIELDS}, kw),
        ("float16", f16[0], f16[1]),
        ("one-dimensional", {k: torch.zeros(NZ, dtype=torch.float64) for k in ref.FIELDS}, kw),
        ("nz = 1", _good(nz=1)[0], _good(nz=1)[1]),
        ("nz = 257", _good(nz=257)[0], _good(nz=257)[1]),
        ("qr missing", {k: v for k, v in st.items() if k != "qr"}, kw),
        ("unknown member", dict(st, qh=st["qg"]), kw),
        ("mixed dtypes", dict(st, qs=torch.zeros(N, NZ, dtype=torch.float32)), kw),
        ("shapes differ", dict(st, nr=torch.zeros(N, NZ + 1, dtype=torch.float64)), kw),
        ("not contiguous", dict(st, qv=torch.zeros(NZ, N, dtype=torch.float64).T), kw),
        ("unknown want", st, dict(kw, want=("sum", "flux"))),
        ("a name twice", st, dict(kw, want=("adv", "adv"))),
        ("want a number", st, dict(kw, want=3)),
        ("nothing wanted", st, dict(kw, want=())),
        ("w numpy", st, dict(kw, w=np.zeros(NZ + 1))),
        ("w of nz values", st, dict(kw, w=torch.zeros(NZ, dtype=torch.float64))),
        ("w [ncol, nz]", st, dict(kw, w=torch.zeros(N, NZ, dtype=torch.float64))),
        ("w [nz+1, ncol]", st, dict(kw, w=torch.zeros(NZ + 1, N, dtype=torch.float64))),
        ("w dtype", st, dict(kw, w=torch.zeros(NZ + 1, dtype=torch.float32))),
        ("rho shape", st, dict(kw, rho=torch.ones(N, NZ, dtype=torch.float64))),
        ("dz dtype", st, dict(kw, dz=torch.ones(NZ, dtype=torch.float32))),
        ("dt = 0", st, dict(kw, dt=0.0)),
        ("dt a string", st, dict(kw, dt="fast")),
        ("out of another call", st, dict(kw, out={"adv": {}})),
    ]


@pytest.mark.parametrize("case", _advect_cases(), ids=lambda c: c[0])
def test_advect_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import advect
    _, st, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="kid_advect"):
        advect(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="kid_advect"):
        _bare().kid_advect(st, **kw)


def _update_cases():
    import torch
    st, _ = _good()
    t = {k: torch.zeros(N, NZ, dtype=torch.float64) for k in ref.FIELDS}
    return [
        ("host memory", st, (t,), {}),
        ("not a dict", [st["qv"]], (t,), {}),
        ("no member", {}, (t,), {}),
        ("float16", _good(torch.float16)[0], (), {}),
        ("unknown member", dict(st, qh=st["qg"]), (), {}),
        ("four tendencies", st, (t, t, t, t), {}),
        ("a tendency that is a tensor", st, (t["qv"],), {}),
        ("tendency dtype", st, (dict(t, qc=torch.zeros(N, NZ, dtype=torch.float32)),), {}),
        ("tendency shape", st, (t, dict(t, nr=torch.zeros(N, NZ - 1, dtype=torch.float64))), {}),
        ("dt < 0", st, (t,), dict(dt=-1.0)),
    ]


@pytest.mark.parametrize("case", _update_cases(), ids=lambda c: c[0])
def test_update_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import update
    _, st, tend, kw = case
    dt = kw.pop("dt", 1.0) if "dt" in kw else 1.0
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="kid_update"):
        update(_bare(), st, dt, *tend)
    with pytest.raises(th.KidmpError, match="kid_update"):
        _bare().kid_update(st, dt, *tend)


def test_run_rejects_bad_arguments_before_the_library(monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import run
    st, kw = _good()
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    args = (1.0, 1.0e5, 0.286, st["qv"], kw["dz"], kw["rho"], kw["w"])
    with pytest.raises(th.KidmpError, match="kid_run"):
        run(_bare(), st, 3, *args, work=None)                                    # the workspace is run's own
    with pytest.raises(th.KidmpError, match="kid_run"):
        _bare().kid_run(st, -1, *args)
    with pytest.raises(th.KidmpError, match="kid_run"):
        run(_bare(), [st["qv"]], 3, *args)


# ---- the three properties of the reference ----
def _profiles(rng, nz):
    rho = 1.2 * np.exp(-np.linspace(0.0, 1.1, nz)) * rng.uniform(0.97, 1.03, nz)
    dz = rng.uniform(20.0, 60.0, nz)
    return rho, dz


def _w_with_sign_change(rng, ncol, nz):
    """[ncol, nz+1]: both signs, a sign change inside every column, w[0] = 0."""
    f = np.linspace(0.0, 1.0, nz + 1)[None, :]
    w = rng.uniform(0.5, 3.0, (ncol, 1)) * np.sin(np.pi * rng.integers(1, 4, (ncol, 1)) * 2.0 * f + rng.uniform(0.1, 3.0, (ncol, 1)))
    w += rng.normal(0.0, 0.2, w.shape)
    w[:, 0] = 0.0
    flip = nz // 2 + 1
    w[:, flip] = -np.abs(w[:, flip]) - 0.1                                       # whatever the sine did: one change for sure
    w[:, flip - 1] = np.abs(w[:, flip - 1]) + 0.1
    return w


@pytest.mark.parametrize("nz", [3, 65, 129])
def test_reference_flux_form_telescopes(nz):
    rng = np.random.Generator(np.random.PCG64(1500 + nz))
    ncol = 200
    q = 10.0 ** rng.uniform(-12.0, 9.0, (ncol, nz)) * (rng.random((ncol, nz)) < 0.5)
    rho, dz = _profiles(rng, nz)
    w = _w_with_sign_change(rng, ncol, nz)
    assert ((w[:, 1:] < 0) != (w[:, :-1] < 0)).any(axis=1).all() and (q == 0).mean() > 0.3
    out = ref.advect({"qv": q}, w, rho, dz, 2.0)
    F, adv = out["F"]["qv"], out["adv"]["qv"]
    total = np.sum(out["den"][None, :] * adv, axis=1)
    resid = np.abs(total - (F[:, 0] - F[:, nz]))
    bound = 8 * nz * EPS * np.abs(F).max(axis=1)
    print("telescoping nz=%d: worst residual / bound = %.3g" % (nz, float(np.max(resid / np.maximum(bound, 1e-300)))))
    assert np.isfinite(adv).all() and (np.abs(F).max(axis=1) > 0).mean() > 0.5
    assert (resid <= bound).all()


@pytest.mark.parametrize("nz", [3, 65, 129])
def test_reference_leaves_a_constant_field_constant(nz):
    rng = np.random.Generator(np.random.PCG64(1600 + nz))
    ncol = 200
    qc = 10.0 ** rng.uniform(-12.0, 9.0, (ncol, 1))
    q = np.ascontiguousarray(np.broadcast_to(qc, (ncol, nz)))
    rho, dz = _profiles(rng, nz)
    w = _w_with_sign_change(rng, ncol, nz)
    out = ref.advect({"qv": q}, w, rho, dz, 2.0)
    bound = 4 * EPS * np.abs(out["M"]).max(axis=1, keepdims=True) * np.abs(qc) / out["den"].min()
    resid = np.abs(out["sum"]["qv"])
    print("constant field nz=%d: worst residual / bound = %.3g" % (nz, float(np.max(resid / bound))))
    assert (np.abs(out["adv"]["qv"]) > 0).any()                                  # the flux form alone does move it
    assert (resid <= bound).all()


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("courant", [0.1, 0.5, 0.9])
def test_reference_is_monotone_and_positive(courant, sign):
    rng = np.random.Generator(np.random.PCG64(1700))
    ncol, nz, dzv, dt = 60, 40, 25.0, 10.0
    q = 10.0 ** rng.uniform(-6.0, 0.0, (ncol, nz)) * (rng.random((ncol, nz)) < 0.6)
    q[:10] = (np.arange(nz)[None, :] > np.arange(5, 35, 3)[:, None]) * 3.0e-3     # steps
    q[10:20] = np.exp(-0.5 * ((np.arange(nz)[None, :] - 20.0) / np.arange(1, 11)[:, None]) ** 2)   # peaks of every width
    w = np.full(nz + 1, sign * courant * dzv / dt)
    out = ref.advect({"qv": q}, w, np.full(nz, 1.1), np.full(nz, dzv), dt)
    assert out["courant"].shape == (ncol,) and np.all(np.abs(out["courant"] - courant) <= 4 * EPS)
    assert not out["div"]["qv"].any()                                            # uniform M: no divergence at all
    new = q + dt * out["sum"]["qv"]
    lo = np.minimum(np.minimum(q[:, :-2], q[:, 1:-1]), q[:, 2:])
    hi = np.maximum(np.maximum(q[:, :-2], q[:, 1:-1]), q[:, 2:])
    tol = 4 * EPS * q.max()
    under, over = float(np.max(lo - new[:, 1:-1])), float(np.max(new[:, 1:-1] - hi))
    print("monotone c=%g sign=%+g: worst undershoot %.3g, overshoot %.3g (tolerance %.3g)" % (courant, sign, under, over, tol))
    assert under <= tol and over <= tol
    assert (q + dt * out["adv"]["qv"] >= 0).all()


def test_reference_update_is_plain_arithmetic():
    rng = np.random.Generator(np.random.PCG64(1800))
    for T in (np.float64, np.float32):
        x = {k: rng.normal(0.0, 1.0, (3, 5)).astype(T) for k in ("theta", "qv")}
        t1 = {k: rng.normal(0.0, 1.0, (3, 5)).astype(T) for k in ("theta", "qv")}
        t2 = {"qv": rng.normal(0.0, 1.0, (3, 5)).astype(T)}
        y = ref.update(x, 0.1, t1, t2)
        assert y["qv"].dtype == T and (y["qv"] >= 0).all() and (y["theta"] < 0).any()
        want = x["qv"] + ((t1["qv"] + t2["qv"]) + np.zeros((3, 5), T)) * T(0.1)
        assert np.array_equal(y["qv"], np.where(want < 0, T(0), want))
        assert np.array_equal(ref.update(x, 0.1, t1, t2, clip=False)["qv"], want) and (want < 0).any()
        assert np.array_equal(ref.update(x, 0.1)["theta"], x["theta"] + T(0) * T(0.1))
