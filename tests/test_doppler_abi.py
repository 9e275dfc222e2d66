"""The Doppler moments (include/kidmp_doppler.h, kid_amd/doppler.py) without a GPU: the four symbols exist in the built
library and in the new header, kid_amd/doppler.py declares them as the header has them, the header compiles as C99 and
C++11, a missing context is refused, the Python wrappers turn wrong arguments away before the library is called, and the
numpy reference of the GPU tests (tests/doppler_ref.py) gives known answers: each closed form against a trapezoid
quadrature of the integral it stands for."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import doppler_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_doppler.h")
SYMBOLS = ("kidmp_doppler_moments_device", "kidmp32_doppler_moments_device", "kidmp_doppler_moments_host", "kidmp32_doppler_moments_host")

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
    text = re.sub(r"typedef struct[^;{]*\{[^}]*\}[^;]*;", " ", text)
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


def test_the_python_declarations_match_the_header():
    import kid_amd
    import kid_amd.doppler as kd
    declared = kd.declare(_Stub()).entries
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
    for struct, elem in (("kidmp_doppler_out", "double"), ("kidmp32_doppler_out", "float")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _code(), re.S).group(1)
        assert body.split()[0] == elem
        members = [m.strip().lstrip("*") for m in body.replace(elem, "").replace(";", "").split(",")]
        assert tuple(members) == kd.DOPPLER_NAMES == kid_amd.DOPPLER_NAMES == ref.NAMES
    assert [n for n, _ in kd._DopplerOut._fields_] == list(kd.DOPPLER_NAMES) and all(t is C.c_void_p for _, t in kd._DopplerOut._fields_)
    assert kid_amd.DOPPLER_INPUTS == ref.INPUTS


def test_the_other_mirrors_do_not_declare_them():
    import kid_amd.fall as fl
    import kid_amd.stats as st
    import kid_amd.summary as sm
    import kid_amd.thompson as th
    for other in (th, st, sm, fl):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_doppler.h"\n'
                   "int use(kidmp_ctx *c, const double *a, kidmp_doppler_out *o)\n"
                   "{ return kidmp_doppler_moments_host(c, 1, 2, a, a, a, a, a, a, a, 0, o); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.doppler import _DopplerOut, library
    L = library()
    o = _DopplerOut()
    args = [None, 4, 120] + [None] * 8 + [C.byref(o)]
    assert L.kidmp_doppler_moments_host(*args) == -5                             # KIDMP_ESTATE
    assert L.kidmp32_doppler_moments_host(*args) == -5
    assert L.kidmp_doppler_moments_device(*args, None) == -5
    assert L.kidmp32_doppler_moments_device(*args, None) == -5


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


def _host_state(dtype=np.float64, n=N, nz=NZ):
    return {k: np.zeros((n, nz), dtype=dtype) for k in ref.INPUTS}


def _host_cases():
    good = _host_state
    return [
        ("not a dict", [np.zeros((N, NZ))], {}),
        ("torch for numpy", {k: __import__("torch").zeros(N, NZ, dtype=__import__("torch").float64) for k in ref.INPUTS}, {}),
        ("float16", _host_state(np.float16), {}),
        ("one-dimensional", {k: np.zeros(NZ) for k in ref.INPUTS}, {}),
        ("nz = 1", _host_state(nz=1), {}),
        ("nz = 257", _host_state(nz=257), {}),
        ("qr missing", {k: v for k, v in good().items() if k != "qr"}, {}),
        ("mixed dtypes", dict(good(), qs=np.zeros((N, NZ), dtype=np.float32)), {}),
        ("shapes differ", dict(good(), qr=np.zeros((N, NZ + 1))), {}),
        ("not contiguous", dict(good(), p=np.zeros((NZ, N)).T), {}),
        ("unknown name", good(), dict(want=("vd", "vz_i"))),
        ("a name twice", good(), dict(want=("vd", "vd"))),
        ("want a number", good(), dict(want=3)),
        ("nothing wanted", good(), dict(want=())),
        ("w shape", good(), dict(w=np.ones(NZ))),
        ("w dtype", good(), dict(w=np.ones((N, NZ), dtype=np.float32))),
        ("w a list", good(), dict(w=[[0.0] * NZ] * N)),
    ]


@pytest.mark.parametrize("case", _host_cases(), ids=lambda c: c[0])
def test_host_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import doppler_moments_host
    _, st, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="doppler_moments_host"):
        doppler_moments_host(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="doppler_moments_host"):
        _bare().doppler_moments_host(st, **kw)


def _device_cases():
    """Host tensors throughout: each case is wrong in one way and, being host memory, on the wrong device as well."""
    import torch
    good = lambda dt=torch.float64, nz=NZ: {k: torch.zeros(N, nz, dtype=dt) for k in ref.INPUTS}   # noqa: E731
    return [
        ("host memory", good(), {}),
        ("not a dict", [torch.zeros(N, NZ, dtype=torch.float64)], {}),
        ("numpy for torch", _host_state(), {}),
        ("float16", good(torch.float16), {}),
        ("one-dimensional", {k: torch.zeros(NZ, dtype=torch.float64) for k in ref.INPUTS}, {}),
        ("nz = 1", good(nz=1), {}),
        ("nz = 257", good(nz=257), {}),
        ("qr missing", {k: v for k, v in good().items() if k != "qr"}, {}),
        ("mixed dtypes", dict(good(), qg=torch.zeros(N, NZ, dtype=torch.float32)), {}),
        ("shapes differ", dict(good(), nr=torch.zeros(N, NZ + 1, dtype=torch.float64)), {}),
        ("not contiguous", dict(good(), p=torch.zeros(NZ, N, dtype=torch.float64).T), {}),
        ("unknown name", good(), dict(want=("doppler",))),
        ("a name twice", good(), dict(want=("sw", "dbz", "sw"))),
        ("nothing wanted", good(), dict(want=[])),
        ("w numpy", good(), dict(w=np.ones((N, NZ)))),
        ("w shape", good(), dict(w=torch.zeros(NZ, dtype=torch.float64))),
        ("w dtype", good(), dict(w=torch.zeros(N, NZ, dtype=torch.float32))),
    ]


@pytest.mark.parametrize("case", _device_cases(), ids=lambda c: c[0])
def test_device_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import doppler_moments
    _, st, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="doppler_moments"):
        doppler_moments(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="doppler_moments"):
        _bare().doppler_moments(st, **kw)


# ---- the numpy reference: each closed form against a trapezoid quadrature in log D over [1e-9 m, 200/lambda] ----
QUAD_RTOL = 1e-10


@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = ref.constants(o)
    o.close()
    return c


def _quadrature(lam_min, psd, speed, sigma_power, n=40001):
    """(<v sigma N>/<sigma N>, <v**2 sigma N>/<sigma N>) with sigma = D**sigma_power; D = exp(u), dD = D du."""
    u = np.linspace(np.log(1e-9), np.log(200.0 / lam_min), n)
    D = np.exp(u)
    wgt = D ** sigma_power * psd(D) * D
    v = speed(D)
    trapz = lambda y: float(np.sum((y[1:] + y[:-1]) * 0.5 * np.diff(u)))   # noqa: E731
    den = trapz(wgt)
    return trapz(v * wgt) / den, trapz(v * v * wgt) / den


def _column(nz=6, t=260.0, p=6.0e4, qv=1.0e-3):
    st = {k: np.zeros((1, nz)) for k in ref.INPUTS}
    st["t"][:], st["p"][:], st["qv"][:] = t, p, qv
    return st


def _rhof(t, p=6.0e4, qv=1.0e-3):
    return np.sqrt(ref.RHO_NOT / (0.622 * p / (287.04 * t * (qv + 0.622))))


def test_reference_rain_level_against_quadrature(consts):
    st = _column(t=285.0)
    st["qr"][0, 2], st["nr"][0, 2] = 1.0e-3, 5.0e3
    out = ref.doppler_moments(consts, st)
    rhof = _rhof(285.0)
    rho = ref.RHO_NOT / rhof ** 2
    lamr = (ref.ro.am_r * consts["crg"][2] * consts["org2"] * (5.0e3 * rho) / (1.0e-3 * rho)) ** (1.0 / 3.0)
    vz, v2 = _quadrature(lamr, lambda D: D ** ref.mu_r * np.exp(-lamr * D),
                         lambda D: rhof * ref.av_r * D ** ref.bv_r * np.exp(-ref.fv_r * D), 6.0)
    assert out["vz_r"][0, 2] == pytest.approx(vz, rel=QUAD_RTOL) and 0.45 < vz / rhof < 8.5
    assert out["m2"][0, 2] == pytest.approx(v2, rel=QUAD_RTOL)
    assert out["vd"][0, 2] == out["vz_r"][0, 2] and out["V"][0, 2] == out["vz_r"][0, 2]     # one species: its own speed
    assert out["sw"][0, 2] ** 2 == pytest.approx(v2 - vz * vz, rel=1e-8)
    # the integer powers the issue states for mu_r = 0, bv_r = 1
    assert out["vz_r"][0, 2] == pytest.approx(rhof * ref.av_r * 7 * lamr ** 7 / (lamr + ref.fv_r) ** 8, rel=1e-13)
    assert out["m2"][0, 2] == pytest.approx(rhof ** 2 * ref.av_r ** 2 * 56 * lamr ** 7 / (lamr + 2 * ref.fv_r) ** 9, rel=1e-13)
    assert out["dbz_s"][0, 2] == out["dbz_g"][0, 2] == -40.0 and out["dbz_r"][0, 2] > 0
    assert not out["vz_r"][0, [0, 1, 3, 4, 5]].any() and not out["vz_s"].any() and not out["vz_g"].any()


def test_reference_graupel_level_against_quadrature(consts):
    st = _column(t=255.0)
    st["qg"][0, 3] = 2.0e-3
    out = ref.doppler_moments(consts, st)
    rhof = _rhof(255.0)
    _, _, _, v, ilamg, _ = ref.ro.ze_terms(consts, st["qv"], st["qr"], st["nr"], st["qs"], st["qg"], st["t"], st["p"])
    lamg = 1.0 / ilamg[0, 3]
    vz, v2 = _quadrature(lamg, lambda D: D ** ref.mu_g * np.exp(-lamg * D), lambda D: rhof * ref.av_g * D ** ref.bv_g, 6.0)
    assert out["vz_g"][0, 3] == pytest.approx(vz, rel=QUAD_RTOL) and 1.3 < vz / rhof < 14.0
    assert out["m2"][0, 3] == pytest.approx(v2, rel=QUAD_RTOL)
    assert out["vd"][0, 3] == out["vz_g"][0, 3] and out["sw"][0, 3] > 0


@pytest.mark.parametrize("xDs", [1e-4, 2e-3])
def test_reference_snow_level_against_quadrature(xDs):
    Mrat, rhof = 1.0 / xDs, 1.17
    got_vz, got_v2 = ref.snow_moments(rhof, Mrat)
    vz, v2 = _quadrature(Mrat * ref.Lam1,
                         lambda D: ref.Kap0 * np.exp(-Mrat * ref.Lam0 * D) + ref.Kap1 * (Mrat * D) ** ref.mu_s * np.exp(-Mrat * ref.Lam1 * D),
                         lambda D: rhof * ref.av_s * D ** ref.bv_s * np.exp(-ref.fv_s * D), 2.0 * ref.bm_s)
    assert got_vz == pytest.approx(vz, rel=QUAD_RTOL) and got_v2 == pytest.approx(v2, rel=QUAD_RTOL)
    assert 0.3 * rhof < got_vz < 1.2 * rhof


def test_reference_snow_level_of_a_state(consts):
    """The state's own Mrat = smob/smoc reaches snow_moments: smoc is the Field fit at cse(1) = bm_s + 1."""
    st = _column(t=250.0)
    st["qs"][0, 1] = 1.0e-3
    out = ref.doppler_moments(consts, st)
    rhof = _rhof(250.0)
    smoc, smob = ref.snow_smoc(consts, np.array(250.0), np.array(1.0e-3 * ref.RHO_NOT / rhof ** 2))
    assert consts["cse"][0] == 3.0 and 1e-4 < smoc / smob < 1e-2
    vz, _ = ref.snow_moments(rhof, smob / smoc)
    assert out["vz_s"][0, 1] == pytest.approx(float(vz), rel=1e-13) and out["vd"][0, 1] == out["vz_s"][0, 1]


def test_reference_rain_and_snow_level_is_the_weighted_mean(consts):
    st = _column(t=272.0)
    st["qr"][0, 1], st["nr"][0, 1], st["qs"][0, 1] = 3.0e-4, 2.0e3, 1.5e-3
    w = np.zeros((1, 6))
    w[0, 1] = 0.75
    out = ref.doppler_moments(consts, st, w=w)
    ze_r, ze_s = 10.0 ** (out["dbz_r"][0, 1] / 10.0) * 1e-18, 10.0 ** (out["dbz_s"][0, 1] / 10.0) * 1e-18
    vr, vs = out["vz_r"][0, 1], out["vz_s"][0, 1]
    assert vs < out["V"][0, 1] < vr
    assert out["V"][0, 1] == pytest.approx((ze_r * vr + ze_s * vs) / (ze_r + ze_s), rel=1e-12)
    assert out["vd"][0, 1] == out["V"][0, 1] - 0.75
    assert out["sw"][0, 1] > 0 and out["sw"][0, 1] == ref.doppler_moments(consts, st)["sw"][0, 1]      # w does not enter
    assert out["dbz"][0, 1] == pytest.approx(10 * np.log10((ze_r + ze_s + 1e-22) * 1e18), abs=1e-12)


def test_reference_empty_level_is_plus_zero(consts):
    st = _column()
    st["qr"][0, 0], st["nr"][0, 0] = 1.0e-3, 1.0e4
    out = ref.doppler_moments(consts, st, w=np.full((1, 6), 2.0))
    for n in ("vd", "sw", "vz_r", "vz_s", "vz_g"):
        a = out[n][0, 1:]
        assert not a.view(np.uint64).any(), n                                    # +0.0: w is not applied to an empty level
    assert out["vd"][0, 0] == out["vz_r"][0, 0] - 2.0
    assert np.allclose(out["dbz"][0, 1:], ref.ro.EMPTY_DBZ) and (out["dbz_r"][0, 1:] == -40.0).all()


def test_reference_variance_is_never_negative(consts):
    import effrad_cases as ec
    st = ec.random_state(65, 48, 4242)
    out = ref.doppler_moments(consts, {k: st[k] for k in ref.INPUTS})
    var = out["m2"] - out["V"] ** 2
    some = out["present_r"] | out["present_s"] | out["present_g"]
    assert some.any() and (~some).any()
    assert (var[some] >= 0).all() and np.isfinite(out["sw"]).all() and (out["sw"] >= 0).all()
    assert all((out["present_" + x] & (out["vz_" + x] > 0)).sum() == out["present_" + x].sum() > 0 for x in "rsg")
