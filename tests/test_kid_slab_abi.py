"""The slab entries (include/kidmp_slab.h, kid_amd/slab.py) without a GPU: the two symbols exist in the built library and
in the new header only, kid_amd/slab.py declares them as the header has them and no other mirror does, the header compiles
as C99 and C++11, a missing context is refused, the Python wrappers turn wrong arguments away before the library is called,
and the numpy reference of the GPU tests (tests/kid_slab_ref.py) has the scheme's three properties, each within a bound
derived from the number of roundings involved (none is a measured number):

  conservation     over a periodic slab SUM_{i,k} rho dz adv = SUM_i (Fz[i,0] - Fz[i,nz]) within 16 nx nz eps Fmax, Fmax =
                   max(|Fz|, |Fx| dz/dx): a cell's term is recovered through at most eight roundings (two differences, two
                   quotients, the add, the product with rho dz, the running sum twice over) of quantities bounded by 2 Fmax
  constant fields  |adv + div| <= 8 eps scale, scale = q max(max|Mz|/min(rho dz), max|Mx|/min(rho dx)): the 1-D bound of
                   four roundings in either direction; for a stream-function flow also |adv| <= 16 eps scale (each of the
                   four face fluxes carries the four roundings of its velocity)
  positivity       uniform one-signed u and w, non-negative q: a limited face value is at most (2 - c) times its upwind
                   cell, so q + dt adv >= q (1 - cx(2 - cx) - cz(2 - cz)) >= 0 while cx(2 - cx) + cz(2 - cz) <= 1, up to
                   4 eps max q; the condition is sharp: (0.45, 0.45) goes negative
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import kid_slab_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_slab.h")
SYMBOLS = ("kidmp_kid_advect_slab_device", "kidmp32_kid_advect_slab_device")
EPS = np.finfo(np.float64).eps

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
    assert '#include "kidmp.h"' in open(HEADER).read()
    assert "_host" not in " ".join(protos)                                   # no host-array entries: the header says why
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):
        if other.endswith(".h") and other != "kidmp_slab.h":
            assert not set(SYMBOLS) & set(_prototypes(os.path.join(inc, other))), other


def test_the_python_declarations_match_the_header():
    import kid_amd
    import kid_amd.slab as ks
    declared = ks.declare(_Stub()).entries
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
    assert kid_amd.advect_slab is ks.advect_slab and kid_amd.run_slab is ks.run_slab
    assert kid_amd.streamfunction_flow is ks.streamfunction_flow
    for name in ("kid_advect_slab", "kid_run_slab"):
        assert callable(getattr(kid_amd.ThompsonMP, name))


def test_the_other_mirrors_do_not_declare_them():
    import kid_amd.doppler as dp
    import kid_amd.fall as fl
    import kid_amd.kinematic as kk
    import kid_amd.stats as st
    import kid_amd.summary as sm
    import kid_amd.thompson as th
    for other in (th, st, sm, fl, dp, kk):
        assert not set(SYMBOLS) & set(other._declarations()), other.__name__


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_slab.h"\n'
                   "int use(kidmp_ctx *c, const double *a, double *o, const kidmp_kid_fields *f,\n"
                   "        const float *a32, float *o32, const kidmp32_kid_fields *f32)\n"
                   "{ return kidmp_kid_advect_slab_device(c, 1, 3, 2, 1.0, 1.0, f, a, a, 1, a, a, f, f, f, o, 0)\n"
                   "       + kidmp32_kid_advect_slab_device(c, 1, 3, 2, 1.0, 1.0, f32, a32, a32, 0, a32, a32, f32, f32, f32, o32, 0); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.slab import library
    from kid_amd.thompson import _KidFields
    L = library()
    f = C.byref(_KidFields())
    args = [None, 2, 5, 120, 10.0, 100.0, f, None, None, 1, None, None, f, f, f, None, None]
    assert L.kidmp_kid_advect_slab_device(*args) == -5                           # KIDMP_ESTATE
    assert L.kidmp32_kid_advect_slab_device(*args) == -5


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


NX, NSLAB, NZ = 5, 2, 40
N = NX * NSLAB


def _good(dt=None, nz=NZ, n=N, nx=NX):
    import torch
    dt = dt or torch.float64
    st = {k: torch.zeros(n, nz, dtype=dt) for k in sref.FIELDS}
    return st, dict(u=torch.zeros(nx, nz, dtype=dt), w=torch.zeros(nx, nz + 1, dtype=dt), rho=torch.ones(nz, dtype=dt),
                    dz=torch.ones(nz, dtype=dt), dx=100.0, dt=1.0, nx=nx)


def _advect_cases():
    """(name, state, arguments, what the message must say).  Host tensors throughout: each case is wrong in one way and,
    being host memory, on the wrong device as well; the message of the last resort is the one about CUDA tensors."""
    import torch
    st, kw = _good()
    f16 = _good(torch.float16)
    z = lambda *s, **k: torch.zeros(*s, dtype=k.get("dtype", torch.float64))   # noqa: E731
    host = "CUDA tensor"
    return [
        ("host memory", st, kw, host),
        ("not a dict", [z(N, NZ)], kw, "state must be a dict"),
        ("float16", f16[0], f16[1], "float64 or float32"),
        ("nz = 257", _good(nz=257)[0], _good(nz=257)[1], "nz in"),
        ("nx = 2", st, dict(kw, nx=2, u=z(2, NZ), w=z(2, NZ + 1)), "nx must be >= 3"),
        ("nx = 0", st, dict(kw, nx=0), "nx must be >= 3"),
        ("nx a float", st, dict(kw, nx=5.0), "nx must be a whole number"),
        ("ncol % nx != 0", st, dict(kw, nx=4, u=z(4, NZ), w=z(4, NZ + 1)), "not a multiple of nx"),
        ("qr missing", {k: v for k, v in st.items() if k != "qr"}, kw, host),
        ("unknown member", dict(st, qh=st["qg"]), kw, "unknown members"),
        ("mixed dtypes", dict(st, qs=z(N, NZ, dtype=torch.float32)), kw, host),
        ("unknown want", st, dict(kw, want=("sum", "flux")), "unknown output"),
        ("nothing wanted", st, dict(kw, want=()), "nothing requested"),
        ("u shared, w per slab", st, dict(kw, w=z(N, NZ + 1)), "both be shared"),
        ("u per slab, w shared", st, dict(kw, u=z(N, NZ)), "both be shared"),
        ("u numpy", st, dict(kw, u=np.zeros((NX, NZ))), "u must be a torch tensor"),
        ("u of nz+1 values", st, dict(kw, u=z(NX, NZ + 1)), "u must be"),
        ("w of nz values", st, dict(kw, w=z(NX, NZ)), "w must be"),
        ("w one profile", st, dict(kw, w=z(NZ + 1)), "w must be"),
        ("u [nz, nx]", st, dict(kw, u=z(NZ, NX)), "u must be"),
        ("u dtype", st, dict(kw, u=z(NX, NZ, dtype=torch.float32)), host),
        ("w dtype", st, dict(kw, u=z(N, NZ), w=z(N, NZ + 1, dtype=torch.float32)), host),
        ("rho shape", st, dict(kw, rho=torch.ones(N, NZ, dtype=torch.float64)), host),
        ("dz dtype", st, dict(kw, dz=torch.ones(NZ, dtype=torch.float32)), host),
        ("dx = 0", st, dict(kw, dx=0.0), "dx must be > 0"),
        ("dx < 0", st, dict(kw, dx=-100.0), "dx must be > 0"),
        ("dx a string", st, dict(kw, dx="wide"), "dx must be a number"),
        ("dt = 0", st, dict(kw, dt=0.0), "dt must be > 0"),
        ("out of another call", st, dict(kw, out={"adv": {}}), host),
    ]


@pytest.mark.parametrize("case", _advect_cases(), ids=lambda c: c[0])
def test_advect_slab_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import advect_slab
    _, st, kw, says = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="kid_advect_slab") as e:
        advect_slab(_bare(), st, **kw)
    assert says in str(e.value), str(e.value)
    with pytest.raises(th.KidmpError, match="kid_advect_slab"):
        _bare().kid_advect_slab(st, **kw)


def test_run_slab_rejects_bad_arguments_before_the_library(monkeypatch):
    import torch
    import kid_amd.thompson as th
    from kid_amd import run_slab
    st, kw = _good()
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    args = (1.0, 1.0e5, 0.286, st["qv"], kw["dz"], kw["rho"], 100.0)             # dt, p0, r_on_cp, exner, dz, rho, dx
    flow = (kw["u"], kw["w"])
    for bad in (lambda: run_slab(_bare(), st, 3, *args, NX, *flow, work=None),   # the workspace is run_slab's own
                lambda: _bare().kid_run_slab(st, -1, *args, NX, *flow),
                lambda: run_slab(_bare(), [st["qv"]], 3, *args, NX, *flow),
                lambda: run_slab(_bare(), st, 3, *args, 2, *flow),               # nx < 3
                lambda: run_slab(_bare(), st, 3, *args, 4, *flow),               # ncol % nx
                lambda: run_slab(_bare(), st, 3, *args, NX, kw["u"], torch.zeros(N, NZ + 1, dtype=torch.float64)),
                lambda: run_slab(_bare(), st, 3, *args[:-1], 0.0, NX, *flow),    # dx
                lambda: run_slab(_bare(), st, 3, *args, NX, *flow)):             # host tensors
        with pytest.raises(th.KidmpError, match="kid_run_slab"):
            bad()


def test_streamfunction_flow_is_the_restatement_and_refuses_bad_shapes():
    import torch
    from kid_amd import KidmpError, streamfunction_flow
    rng = np.random.Generator(np.random.PCG64(2100))
    nx, nz, nslab = 7, 9, 3
    rho, dz = _profiles(rng, nz)
    psi = rng.normal(0.0, 50.0, (nslab * nx, nz + 1))
    t = lambda a: torch.from_numpy(a)   # noqa: E731
    for p, n in ((psi[:nx], None), (psi, nx)):
        u, w = streamfunction_flow(t(np.ascontiguousarray(p)), t(rho), t(dz), 150.0, **({} if n is None else {"nx": n}))
        ru, rw = sref.streamfunction_flow(p, rho, dz, 150.0, n)
        assert u.shape == (p.shape[0], nz) and w.shape == (p.shape[0], nz + 1) and u.is_contiguous() and w.is_contiguous()
        assert np.array_equal(u.numpy(), ru) and np.array_equal(w.numpy(), rw)
    u1, w1 = sref.streamfunction_flow(psi[nx:2 * nx], rho, dz, 150.0)            # each slab is periodic on its own
    assert np.array_equal(ru[nx:2 * nx], u1) and np.array_equal(rw[nx:2 * nx], w1)
    for bad in (lambda: streamfunction_flow(t(psi[:, :-1].copy()), t(rho), t(dz), 150.0),
                lambda: streamfunction_flow(psi, t(rho), t(dz), 150.0),
                lambda: streamfunction_flow(t(psi), t(rho), t(dz), 0.0),
                lambda: streamfunction_flow(t(psi), t(rho), t(dz), 150.0, nx=4)):
        with pytest.raises(KidmpError, match="streamfunction_flow"):
            bad()


# ---- the three properties of the reference ----
def _profiles(rng, nz):
    rho = 1.2 * np.exp(-np.linspace(0.0, 1.1, nz)) * rng.uniform(0.97, 1.03, nz)
    dz = rng.uniform(20.0, 60.0, nz)
    return rho, dz


def _psi(rng, nx, nz, amp=400.0):
    """[nx, nz+1]: cells that turn over plus noise, so that u and w change sign inside every row and column; psi = 0 at
    the ground, so w[:, 0] = 0."""
    x = (np.arange(nx) / float(nx))[:, None]
    f = np.linspace(0.0, 1.0, nz + 1)[None, :]
    psi = amp * np.sin(2.0 * np.pi * x + 0.3) * np.sin(np.pi * f) + rng.normal(0.0, 0.05 * amp, (nx, nz + 1))
    psi[:, 0] = 0.0
    return psi


@pytest.mark.parametrize("nz", [3, 65, 129])
def test_reference_conserves_mass_over_a_periodic_slab(nz):
    rng = np.random.Generator(np.random.PCG64(2200 + nz))
    nx, dx, dt = 7, 150.0, 2.0
    rho, dz = _profiles(rng, nz)
    u, w = sref.streamfunction_flow(_psi(rng, nx, nz), rho, dz, dx)
    q = 10.0 ** rng.uniform(-12.0, 9.0, (nx, nz)) * (rng.random((nx, nz)) < 0.67)
    assert (u > 0).any() and (u < 0).any() and (w > 0).any() and (w < 0).any() and (q == 0).mean() > 0.2
    out = sref.advect_slab({"qv": q}, u, w, rho, dz, dx, dt, nx)
    Fz, Fx, adv = out["Fz"]["qv"], out["Fx"]["qv"], out["adv"]["qv"]
    total = np.sum(out["den"][None, :] * adv)
    through = np.sum(Fz[:, 0] - Fz[:, nz])
    Fmax = max(np.abs(Fz).max(), (np.abs(Fx) * dz[None, :] / dx).max())
    bound = 16 * nx * nz * EPS * Fmax
    print("conservation nz=%d: residual %.3g = %.3g of nx nz eps Fmax" % (nz, abs(total - through), abs(total - through) / (nx * nz * EPS * Fmax)))
    assert np.isfinite(adv).all() and Fmax > 0 and np.abs(Fx).max() > 0
    assert abs(total - through) <= bound


@pytest.mark.parametrize("nz", [3, 65, 129])
def test_reference_leaves_a_constant_field_constant(nz):
    rng = np.random.Generator(np.random.PCG64(2300 + nz))
    nx, dx, dt = 7, 150.0, 2.0
    rho, dz = _profiles(rng, nz)
    qc = 10.0 ** rng.uniform(-12.0, 9.0)
    q = np.full((nx, nz), qc)
    flows = {"stream function": sref.streamfunction_flow(_psi(rng, nx, nz), rho, dz, dx),
             "divergent": (rng.normal(0.0, 3.0, (nx, nz)), np.concatenate([np.zeros((nx, 1)), rng.normal(0.0, 1.0, (nx, nz))], axis=1))}
    for name, (u, w) in flows.items():
        out = sref.advect_slab({"qv": q}, u, w, rho, dz, dx, dt, nx)
        scale = qc * max(np.abs(out["Mz"]).max() / out["den"].min(), np.abs(out["Mx"]).max() / out["denx"].min())
        worst = np.abs(out["sum"]["qv"]).max() / (EPS * scale)
        print("constant field nz=%d, %s: |sum| <= %.3g eps scale" % (nz, name, worst))
        assert worst <= 8
        if name == "stream function":
            worst = np.abs(out["adv"]["qv"]).max() / (EPS * scale)
            print("constant field nz=%d, %s: |adv| <= %.3g eps scale" % (nz, name, worst))
            assert worst <= 16
        else:
            assert np.abs(out["adv"]["qv"]).max() > 1e6 * EPS * scale            # the flux form alone does move it


def _positivity_field(rng, nx, nz, su, sw):
    """Non-negative, a third zeros, with the worst case planted: a cell of 1 whose upwind neighbours are 0 and whose
    downwind neighbours are large, in x and in z at once (both outflow faces then carry (2 - c) times the cell)."""
    q = 10.0 ** rng.uniform(-6.0, 0.0, (nx, nz)) * (rng.random((nx, nz)) < 0.67)
    i, k = nx // 2, nz // 2
    q[i - 2:i + 3, k - 2:k + 3] = 0.0
    q[i, k] = 1.0
    q[i + su, k] = q[i, k + sw] = 1.0e3
    return q


@pytest.mark.parametrize("su, sw", [(1, 1), (1, -1), (-1, 1), (-1, -1)], ids=["u+w+", "u+w-", "u-w+", "u-w-"])
@pytest.mark.parametrize("cx, cz", [(0.29, 0.29), (0.1, 0.45), (0.45, 0.1), (0.2, 0.36), (0.5, 0.0), (0.45, 0.45)])
def test_reference_is_positive_under_the_unsplit_condition(cx, cz, su, sw):
    rng = np.random.Generator(np.random.PCG64(2400))
    nx, nz, dx, dzv, dt = 9, 12, 100.0, 25.0, 10.0
    q = _positivity_field(rng, nx, nz, su, sw)
    u = np.full((nx, nz), su * cx * dx / dt)
    w = np.full((nx, nz + 1), sw * cz * dzv / dt)
    out = sref.advect_slab({"qv": q}, u, w, np.full(nz, 1.1), np.full(nz, dzv), dx, dt, nx)
    assert np.all(np.abs(out["courant"] - (cx + cz)) <= 8 * EPS)
    new = q + dt * out["adv"]["qv"]
    tol = 4 * EPS * q.max()
    # a limited face value is at most (2 - c) times its upwind cell
    qf_x = out["Fx"]["qv"] / out["Mx"] if cx else None
    up_x = np.roll(q, 1, axis=0) if su > 0 else q
    if qf_x is not None:
        assert (qf_x <= (2.0 - cx) * up_x + tol).all() and (qf_x >= -tol).all()
    if cz:
        qf_z = out["Fz"]["qv"][:, 1:nz] / out["Mz"][:, 1:nz]
        up_z = q[:, :nz - 1] if sw > 0 else q[:, 1:]
        assert (qf_z <= (2.0 - cz) * up_z + tol).all() and (qf_z >= -tol).all()
    print("positivity cx=%g cz=%g: min(q + dt adv) = %.3g (tolerance %.3g)" % (cx, cz, new.min(), -tol))
    if cx * (2.0 - cx) + cz * (2.0 - cz) <= 1.0:
        assert (new >= -tol).all()
    else:
        assert new.min() < 0.0                                       # (0.45, 0.45): the condition is sharp
