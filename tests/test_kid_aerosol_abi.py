"""The aerosol entries (include/kidmp_aerosol.h, kid_amd/aerosol.py) without a GPU: the ten symbols exist in the built
library and in the new header only, kid_amd/aerosol.py declares them as the header has them and no other mirror does, the
header compiles as C99 and C++11, a missing context is refused by every entry, and the Python wrappers turn wrong arguments
away before the library is called."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_aerosol.h")
STEMS = ("kid_interface_aero_device", "kid_gather_aero_device", "kid_advect_aero_device", "kid_advect_slab_aero_device",
         "kid_update_aero_device")
SYMBOLS = tuple(pre + "_" + s for s in STEMS for pre in ("kidmp", "kidmp32"))

SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "size_t": (C.c_size_t,), "double": (C.c_double,),
           "float": (C.c_float,), "int": (C.c_int, C.c_int32)}


def _code(path=HEADER):
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes(path=HEADER):
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of a header (the method of
    test_kid_slab_abi.py)."""
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
    assert len(SYMBOLS) == 10 and sorted(protos) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    text = open(HEADER).read()
    for inc in ("kidmp.h", "kidmp_kinematic.h", "kidmp_slab.h"):
        assert '#include "%s"' % inc in text, inc
    assert "_host" not in " ".join(protos)                                   # no host-array entries: the header says why
    assert "W:36" in text and "tnccn_act" in text and "unpinned" in text     # ... and states the two facts of this branch
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):
        if other.endswith(".h") and other != "kidmp_aerosol.h":
            assert not set(SYMBOLS) & set(_prototypes(os.path.join(inc, other))), other
    assert len(_prototypes(os.path.join(inc, "kidmp.h"))) == 67              # kidmp.h keeps exactly its prototypes


def test_the_python_declarations_match_the_header():
    import kid_amd
    import kid_amd.aerosol as ka
    declared = ka.declare(_Stub()).entries
    protos = _prototypes()
    assert sorted(declared) == sorted(protos)
    structs = {"kid_fields": kid_amd.thompson._KidFields, "kid_aerosols": ka._KidAerosols, "outputs": kid_amd.thompson._Outputs}
    assert [n for n, _ in ka._KidAerosols._fields_] == ["nc", "nwfa", "nifa"] and C.sizeof(ka._KidAerosols) == 3 * C.sizeof(C.c_void_p)
    assert re.search(r"struct kidmp_kid_aerosols\s*\{\s*double \*nc, \*nwfa, \*nifa;\s*\}", _code())
    assert re.search(r"struct kidmp32_kid_aerosols\s*\{\s*float\s+\*nc, \*nwfa, \*nifa;\s*\}", _code())
    wrong = []
    for name, (ret, params) in sorted(protos.items()):
        e = declared[name]
        if len(e.argtypes) != len(params):
            wrong.append("%s: %d arguments declared, the header has %d" % (name, len(e.argtypes), len(params)))
            continue
        for i, (p, t) in enumerate(zip(params, e.argtypes)):
            ok = _is_pointer(t) if "*" in p else t in SCALARS[re.sub(r"\bconst\b", "", p).split()[0]]
            for word, struct in structs.items():
                if re.search(r"kidmp(32)?_%s\b" % word, p):
                    ok = ok and t is C.POINTER(struct)
            if not ok:
                wrong.append("%s: argument %d is `%s`, declared %s" % (name, i, p, getattr(t, "__name__", t)))
        if e.restype not in SCALARS[ret]:
            wrong.append("%s: returns `%s`, declared %s" % (name, ret, getattr(e.restype, "__name__", e.restype)))
    assert not wrong, "\n".join(wrong)
    assert ka.AEROSOL_FIELDS == ("nc", "nwfa", "nifa") and kid_amd.AEROSOL_FIELDS is ka.AEROSOL_FIELDS
    for name in ("kid_interface_aero", "advect_aero", "advect_slab_aero", "update_aero", "run_aero", "run_slab_aero"):
        assert getattr(kid_amd, name) is getattr(ka, name), name
    for name in ("kid_interface_aero", "kid_advect_aero", "kid_advect_slab_aero", "kid_update_aero", "kid_run_aero", "kid_run_slab_aero"):
        assert callable(getattr(kid_amd.ThompsonMP, name)), name


def test_the_other_mirrors_do_not_declare_them():
    import kid_amd.doppler as dp
    import kid_amd.fall as fl
    import kid_amd.kinematic as kk
    import kid_amd.slab as ks
    import kid_amd.spectra as sp
    import kid_amd.stats as st
    import kid_amd.summary as sm
    import kid_amd.thompson as th
    for other in (th, st, sm, fl, dp, kk, ks, sp):
        assert not set(SYMBOLS) & set(other._declarations()), other.__name__


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text(
        '#include "kidmp_aerosol.h"\n'
        "int use(kidmp_ctx *c, const double *a, double *o, const kidmp_kid_fields *f, const kidmp_kid_aerosols *n,\n"
        "        const float *a32, float *o32, const kidmp32_kid_fields *f32, const kidmp32_kid_aerosols *n32, void *wk)\n"
        "{ return kidmp_kid_interface_aero_device(c, 1, 2, 1.0, 1.0, 1.0, f, f, f, a, a, f, o, o, 0, 0, n, n, n, n, a, 0, a, wk, 0, 0)\n"
        "       + kidmp32_kid_interface_aero_device(c, 1, 2, 1.0f, 1.0f, 1.0f, f32, f32, f32, a32, a32, f32, o32, o, 0, 0, 1, n32, n32, n32,\n"
        "                                           n32, a32, 0, a32, wk, 0, 0)\n"
        "       + kidmp_kid_gather_aero_device(c, 1, 2, 1.0, 1.0, 1.0, f, f, f, a, a, o, n, n, n, a, 0, wk, 0, 0)\n"
        "       + kidmp32_kid_gather_aero_device(c, 1, 2, 1.0f, 1.0f, 1.0f, f32, f32, f32, a32, a32, o32, n32, n32, n32, a32, 0, wk, 0, 0)\n"
        "       + kidmp_kid_advect_aero_device(c, 1, 2, 1.0, n, a, 0, a, a, n, n, n, 0)\n"
        "       + kidmp32_kid_advect_aero_device(c, 1, 2, 1.0, n32, a32, 0, a32, a32, n32, n32, n32, 0)\n"
        "       + kidmp_kid_advect_slab_aero_device(c, 1, 3, 2, 1.0, 1.0, n, a, a, 1, a, a, n, n, n, 0)\n"
        "       + kidmp32_kid_advect_slab_aero_device(c, 1, 3, 2, 1.0, 1.0, n32, a32, a32, 0, a32, a32, n32, n32, n32, 0)\n"
        "       + kidmp_kid_update_aero_device(c, 1, 2, 1.0, n, n, n, n, 1, 0)\n"
        "       + kidmp32_kid_update_aero_device(c, 1, 2, 1.0f, n32, n32, n32, n32, 1, 0); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.aerosol import _KidAerosols, library
    from kid_amd.thompson import _KidFields
    L = library()
    f, a = C.byref(_KidFields()), C.byref(_KidAerosols())
    ESTATE = -5
    head = [None, 4, 120, 10.0, 1.0e5, 0.286, f, None, None, None, None]
    assert L.kidmp_kid_interface_aero_device(*head, f, None, None, None, None, a, None, None, a, None, 0, None, None, 0, None) == ESTATE
    assert L.kidmp32_kid_interface_aero_device(*head, f, None, None, None, None, 0, a, None, None, a, None, 0, None, None, 0, None) == ESTATE
    assert L.kidmp_kid_gather_aero_device(*head, None, a, None, None, None, 0, None, 0, None) == ESTATE
    assert L.kidmp32_kid_gather_aero_device(*head, None, a, None, None, None, 0, None, 0, None) == ESTATE
    for fn in (L.kidmp_kid_advect_aero_device, L.kidmp32_kid_advect_aero_device):
        assert fn(None, 4, 120, 10.0, a, None, 0, None, None, a, a, a, None) == ESTATE
    for fn in (L.kidmp_kid_advect_slab_aero_device, L.kidmp32_kid_advect_slab_aero_device):
        assert fn(None, 2, 5, 120, 10.0, 100.0, a, None, None, 1, None, None, a, a, a, None) == ESTATE
    for fn in (L.kidmp_kid_update_aero_device, L.kidmp32_kid_update_aero_device):
        assert fn(None, 4, 120, 10.0, a, a, None, None, 1, None) == ESTATE


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
    m.aerosol_aware = True
    return m


NX, NSLAB, NZ = 5, 2, 40
N = NX * NSLAB
HOST = "CUDA tensor"                                        # the message of the last resort: every tensor here is host memory


def _z(*shape, dtype=None):
    import torch
    return torch.zeros(*shape, dtype=dtype or torch.float64)


def _state(dtype=None, nz=NZ, n=N):
    from kid_amd import AEROSOL_FIELDS, KID_FIELDS
    return {k: _z(n, nz, dtype=dtype) for k in KID_FIELDS + AEROSOL_FIELDS}


def _interface_cases():
    import torch
    st = _state()
    kw = dict(dt=1.0, p0=1.0e5, r_on_cp=0.286, exner=_z(N, NZ), dz=_z(NZ))
    f16 = _state(torch.float16)
    return [
        ("host memory", st, kw, HOST),
        ("nwfa missing", {k: v for k, v in st.items() if k != "nwfa"}, kw, "state['nwfa'] is required"),
        ("nc None", dict(st, nc=None), kw, "state['nc'] is required"),
        ("float16", f16, dict(kw, exner=f16["qv"]), "float64 or float32"),
        ("w of nz+1 values", st, dict(kw, w=_z(NZ + 1)), "cell-centre updraft"),
        ("w [ncol, nz+1]", st, dict(kw, w=_z(N, NZ + 1)), "cell-centre updraft"),
        ("w numpy", st, dict(kw, w=np.zeros(NZ)), "w must be a torch tensor"),
        ("nwfa_source [ncol, 1]", st, dict(kw, nwfa_source=_z(N, 1)), "nwfa_source must be a tensor [ncol]"),
        ("nwfa_source [nz]", st, dict(kw, nwfa_source=_z(NZ)), "nwfa_source must be a tensor [ncol]"),
        ("unknown member", dict(st, nh=st["nc"]), kw, "unknown members"),
        ("unknown member of adv", st, dict(kw, adv={"ccn": st["nc"]}), "adv has unknown members"),
        ("arith on float64", st, dict(kw, arith="f32"), "arith applies to float32"),
        ("arith f32", _state(torch.float32), dict(kw, arith="f32", exner=_z(N, NZ, dtype=torch.float32)), "'p32n' only"),
        ("dt = 0", st, dict(kw, dt=0.0), "dt must be > 0"),
    ]


@pytest.mark.parametrize("case", _interface_cases(), ids=lambda c: c[0])
def test_kid_interface_aero_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import kid_interface_aero
    _, st, kw, says = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="kid_interface_aero") as e:
        kid_interface_aero(_bare(), st, **kw)
    assert says in str(e.value), str(e.value)
    with pytest.raises(th.KidmpError, match="kid_interface_aero"):
        _bare().kid_interface_aero(st, **kw)


def test_a_context_that_is_not_aerosol_aware_is_refused_by_name(monkeypatch):
    import kid_amd.thompson as th
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    m = _bare()
    m.aerosol_aware = False
    st = _state()
    with pytest.raises(th.KidmpError, match="kid_interface_aero: the context is not aerosol-aware"):
        m.kid_interface_aero(st, 1.0, 1.0e5, 0.286, _z(N, NZ), _z(NZ))
    with pytest.raises(th.KidmpError, match="kid_run_aero: the context is not aerosol-aware"):
        m.kid_run_aero(st, 1, 1.0, 1.0e5, 0.286, _z(N, NZ), _z(NZ), _z(NZ), _z(NZ + 1))


def _advect_cases():
    import torch
    aer = {k: _z(N, NZ) for k in ("nc", "nwfa", "nifa")}
    kw = dict(w=_z(NZ + 1), rho=_z(NZ), dz=_z(NZ), dt=1.0)
    return [
        ("host memory", aer, kw, HOST),
        ("twelve members, host memory", _state(), kw, HOST),
        ("no aerosol member", {k: v for k, v in _state().items() if k not in aer}, kw, "members out of nc, nwfa, nifa"),
        ("float16", {k: _z(N, NZ, dtype=torch.float16) for k in aer}, kw, "float64 or float32"),
        ("w of nz values", aer, dict(kw, w=_z(NZ)), "face velocities"),
        ("w [ncol, nz]", aer, dict(kw, w=_z(N, NZ)), "face velocities"),
        ("unknown member", dict(aer, ccn=aer["nc"]), kw, "unknown members"),
        ("unknown want", aer, dict(kw, want=("sum", "flux")), "unknown output"),
        ("nothing wanted", aer, dict(kw, want=()), "nothing requested"),
        ("dt < 0", aer, dict(kw, dt=-1.0), "dt must be > 0"),
    ]


@pytest.mark.parametrize("case", _advect_cases(), ids=lambda c: c[0])
def test_advect_aero_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import advect_aero
    _, st, kw, says = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="kid_advect_aero") as e:
        advect_aero(_bare(), st, **kw)
    assert says in str(e.value), str(e.value)
    with pytest.raises(th.KidmpError, match="kid_advect_aero"):
        _bare().kid_advect_aero(st, **kw)


def _slab_cases():
    aer = {k: _z(N, NZ) for k in ("nc", "nwfa", "nifa")}
    kw = dict(u=_z(NX, NZ), w=_z(NX, NZ + 1), rho=_z(NZ), dz=_z(NZ), dx=100.0, dt=1.0, nx=NX)
    return [
        ("host memory", aer, kw, HOST),
        ("nx = 2", aer, dict(kw, nx=2, u=_z(2, NZ), w=_z(2, NZ + 1)), "nx must be >= 3"),
        ("nx = 0", aer, dict(kw, nx=0), "nx must be >= 3"),
        ("ncol % nx != 0", aer, dict(kw, nx=4, u=_z(4, NZ), w=_z(4, NZ + 1)), "not a multiple of nx"),
        ("w of nz values", aer, dict(kw, w=_z(NX, NZ)), "w must be"),
        ("u shared, w per slab", aer, dict(kw, w=_z(N, NZ + 1)), "both be shared"),
        ("unknown member", dict(aer, ccn=aer["nc"]), kw, "unknown members"),
        ("dx = 0", aer, dict(kw, dx=0.0), "dx must be > 0"),
    ]


@pytest.mark.parametrize("case", _slab_cases(), ids=lambda c: c[0])
def test_advect_slab_aero_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import advect_slab_aero
    _, st, kw, says = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="kid_advect_slab_aero") as e:
        advect_slab_aero(_bare(), st, **kw)
    assert says in str(e.value), str(e.value)
    with pytest.raises(th.KidmpError, match="kid_advect_slab_aero"):
        _bare().kid_advect_slab_aero(st, **kw)


def test_update_aero_rejects_bad_arguments_before_the_library(monkeypatch):
    import torch
    import kid_amd.thompson as th
    from kid_amd import update_aero
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    aer = {k: _z(N, NZ) for k in ("nc", "nwfa", "nifa")}
    for bad, says in ((lambda: update_aero(_bare(), aer, 1.0, aer), HOST),
                      (lambda: update_aero(_bare(), aer, 1.0, aer, aer, aer, aer), "at most three"),
                      (lambda: update_aero(_bare(), aer, 0.0, aer), "dt must be > 0"),
                      (lambda: update_aero(_bare(), aer, 1.0, [aer["nc"]]), "must be a dict"),
                      (lambda: update_aero(_bare(), {"qc": aer["nc"]}, 1.0, aer), "members out of nc, nwfa, nifa"),
                      (lambda: update_aero(_bare(), dict(aer, ccn=aer["nc"]), 1.0, aer), "unknown members"),
                      (lambda: _bare().kid_update_aero({k: v.to(torch.float16) for k, v in aer.items()}, 1.0), "float64 or float32")):
        with pytest.raises(th.KidmpError, match="kid_update_aero") as e:
            bad()
        assert says in str(e.value), str(e.value)


def test_the_runs_reject_bad_arguments_before_the_library(monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import run_aero, run_slab_aero
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    st = _state()
    args = (1.0, 1.0e5, 0.286, _z(N, NZ), _z(NZ), _z(NZ))                        # dt, p0, r_on_cp, exner, dz, rho
    w1, u2, w2 = _z(NZ + 1), _z(NX, NZ), _z(NX, NZ + 1)
    for bad, says in ((lambda: run_aero(_bare(), st, 3, *args, w1), HOST),
                      (lambda: run_aero(_bare(), st, 3, *args, _z(NZ)), "face velocities"),
                      (lambda: run_aero(_bare(), {k: v for k, v in st.items() if k != "nifa"}, 3, *args, w1), "state['nifa'] is required"),
                      (lambda: run_aero(_bare(), dict(st, ccn=st["nc"]), 3, *args, w1), "unknown members"),
                      (lambda: _bare().kid_run_aero(st, 3, *args, w1, nwfa_source=_z(NZ)), "nwfa_source must be a tensor [ncol]")):
        with pytest.raises(th.KidmpError, match="kid_run_aero") as e:
            bad()
        assert says in str(e.value), str(e.value)
    for bad, says in ((lambda: run_slab_aero(_bare(), st, 3, *args, 100.0, NX, u2, w2), HOST),
                      (lambda: run_slab_aero(_bare(), st, 3, *args, 100.0, 2, u2, w2), "nx must be >= 3"),
                      (lambda: run_slab_aero(_bare(), st, 3, *args, 100.0, NX, u2, _z(N, NZ + 1)), "both be shared"),
                      (lambda: _bare().kid_run_slab_aero({k: v for k, v in st.items() if k != "nc"}, 3, *args, 100.0, NX, u2, w2),
                       "state['nc'] is required")):
        with pytest.raises(th.KidmpError, match="kid_run_slab_aero") as e:
            bad()
        assert says in str(e.value), str(e.value)
