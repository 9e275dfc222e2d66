"""The fall speeds (include/kidmp_fall.h, kid_amd/fall.py) without a GPU: the four symbols exist in the built library and
in the new header, kid_amd/fall.py declares them as the header has them, the header compiles as C99 and C++11, a missing
context is refused, the Python wrappers turn wrong arguments away before the library is called, and the numpy reference
of the GPU tests (tests/fall_speeds_ref.py) gives known answers formed independently of the oracle's constants."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fall_cases as fc
import fall_speeds_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_fall.h")
SYMBOLS = ("kidmp_fall_speeds_device", "kidmp32_fall_speeds_device", "kidmp_fall_speeds_host", "kidmp32_fall_speeds_host")

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
    import kid_amd.fall as kf
    declared = kf.declare(_Stub()).entries
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
    for struct, elem in (("kidmp_fall_out", "double"), ("kidmp32_fall_out", "float")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _code(), re.S).group(1)
        assert body.split()[0] == elem
        members = [m.strip().lstrip("*") for m in body.replace(elem, "").replace(";", "").split(",")]
        assert tuple(members) == kf.FALL_NAMES == kid_amd.FALL_NAMES == ref.NAMES
    assert [n for n, _ in kf._FallOut._fields_] == list(kf.FALL_NAMES) and all(t is C.c_void_p for _, t in kf._FallOut._fields_)
    assert kid_amd.FALL_INPUTS == ref.INPUTS == fc.KEYS


def test_the_other_mirrors_do_not_declare_them():
    import kid_amd.stats as st
    import kid_amd.summary as sm
    import kid_amd.thompson as th
    for other in (th, st, sm):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_fall.h"\n'
                   "int use(kidmp_ctx *c, const double *a, kidmp_fall_out *o, int32_t *n)\n"
                   "{ return kidmp_fall_speeds_host(c, 1, 2, a, a, a, a, a, a, a, a, a, 0, a, 0, 1.0, o, n); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.fall import _FallOut, library
    L = library()
    o = _FallOut()
    args = [None, 4, 120] + [None] * 11 + [0, 10.0, C.byref(o), None]
    assert L.kidmp_fall_speeds_host(*args) == -5                                 # KIDMP_ESTATE
    assert L.kidmp32_fall_speeds_host(*args) == -5
    assert L.kidmp_fall_speeds_device(*args, None) == -5
    assert L.kidmp32_fall_speeds_device(*args, None) == -5


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
    good, dz = _host_state, np.ones(NZ)
    return [
        ("not a dict", [np.zeros((N, NZ))], {}),
        ("torch for numpy", {k: __import__("torch").zeros(N, NZ, dtype=__import__("torch").float64) for k in ref.INPUTS}, {}),
        ("float16", _host_state(np.float16), {}),
        ("one-dimensional", {k: np.zeros(NZ) for k in ref.INPUTS}, {}),
        ("nz = 1", _host_state(nz=1), {}),
        ("nz = 257", _host_state(nz=257), {}),
        ("qr missing", {k: v for k, v in good().items() if k != "qr"}, {}),
        ("mixed dtypes", dict(good(), qi=np.zeros((N, NZ), dtype=np.float32)), {}),
        ("shapes differ", dict(good(), qr=np.zeros((N, NZ + 1))), {}),
        ("not contiguous", dict(good(), p=np.zeros((NZ, N)).T), {}),
        ("unknown name", good(), dict(want=("vt_r", "vt_c"))),
        ("a name twice", good(), dict(want=("vt_r", "vt_r"))),
        ("want a number", good(), dict(want=3)),
        ("nothing wanted", good(), dict(want=())),
        ("boost shape", good(), dict(boost=np.ones(NZ))),
        ("boost dtype", good(), dict(boost=np.ones((N, NZ), dtype=np.float32))),
        ("dz without dt", good(), dict(dz=dz)),
        ("dt without dz", good(), dict(dt=10.0)),
        ("dt = 0", good(), dict(dz=dz, dt=0.0)),
        ("dt a NaN", good(), dict(dz=dz, dt=float("nan"))),
        ("dz dtype", good(), dict(dz=dz.astype(np.float32), dt=10.0)),
        ("dz length", good(), dict(dz=np.ones(NZ + 1), dt=10.0)),
        ("dz a list", good(), dict(dz=[1.0] * NZ, dt=10.0)),
        ("dz strided", good(), dict(dz=np.ones((N, 2 * NZ))[:, ::2], dt=10.0)),
    ]


@pytest.mark.parametrize("case", _host_cases(), ids=lambda c: c[0])
def test_host_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import fall_speeds_host
    _, st, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="fall_speeds_host"):
        fall_speeds_host(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="fall_speeds_host"):
        _bare().fall_speeds_host(st, **kw)


def _device_cases():
    """Host tensors throughout: each case is wrong in one way and, being host memory, on the wrong device as well."""
    import torch
    good = lambda dt=torch.float64: {k: torch.zeros(N, NZ, dtype=dt) for k in ref.INPUTS}   # noqa: E731
    return [
        ("host memory", good(), {}),
        ("numpy for torch", _host_state(), {}),
        ("float16", good(torch.float16), {}),
        ("nz = 257", {k: torch.zeros(N, 257, dtype=torch.float64) for k in ref.INPUTS}, {}),
        ("t missing", {k: v for k, v in good().items() if k != "t"}, {}),
        ("unknown name", good(), dict(want=("flux",))),
        ("boost numpy", good(), dict(boost=np.ones((N, NZ)))),
        ("dz numpy", good(), dict(dz=np.ones(NZ), dt=10.0)),
    ]


@pytest.mark.parametrize("case", _device_cases(), ids=lambda c: c[0])
def test_device_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import fall_speeds
    _, st, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="fall_speeds"):
        fall_speeds(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="fall_speeds"):
        _bare().fall_speeds(st, **kw)


# ---- the numpy reference on hand-built columns with known answers ----
@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = ref.constants(o)
    o.close()
    return c


def _column(nz=8, t=260.0, p=6.0e4, qv=1.0e-3):
    st = {k: np.zeros((1, nz)) for k in ref.INPUTS}
    st["t"][:], st["p"][:], st["qv"][:] = t, p, qv
    return st


def _rho(t, p=6.0e4, qv=1.0e-3):
    return 0.622 * p / (287.04 * t * (qv + 0.622))


def test_reference_rain_level_with_gammas_of_its_own(consts):
    """One rain level inside the limits of M:1459-1467: crg(6) = Gamma(bm_r+mu_r+bv_r+1) = Gamma(5), crg(3) = Gamma(4),
    org2 = 1/Gamma(mu_r+1), org3 = 1/crg(3) (M:485-505) from math.gamma; cre(3) = 4, cre(6) = 5."""
    st = _column(t=285.0)
    qr, nr1 = 1.0e-3, 5.0e3
    st["qr"][0, 3], st["nr"][0, 3] = qr, nr1
    out = ref.fall_speeds(consts, st)
    rho = _rho(285.0)
    crg3, crg6, org2 = math.gamma(4.0), math.gamma(5.0), 1.0 / math.gamma(1.0)
    org3 = 1.0 / crg3
    lamr = (math.pi * 1000.0 / 6.0 * crg3 * org2 * (nr1 * rho) / (qr * rho)) ** (1.0 / 3.0)
    assert 37.5e-6 < 3.672 / lamr < 2.5e-3                                       # not limited
    vtr = math.sqrt(101325.0 / (287.05 * 298.0) / rho) * 4854.0 * crg6 * org3 * lamr ** 4 / (lamr + 195.0) ** 5
    assert out["vt_r"][0, 3] == pytest.approx(vtr, rel=1e-9)                     # PI of M:35 has ten digits
    pi_ = ref.PI
    lamr = (pi_ * 1000.0 / 6.0 * crg3 * org2 * (nr1 * rho) / (qr * rho)) ** (1.0 / 3.0)
    vtr = math.sqrt(101325.0 / (287.05 * 298.0) / rho) * 4854.0 * crg6 * org3 * lamr ** 4 / (lamr + 195.0) ** 5
    assert out["vt_r"][0, 3] == pytest.approx(vtr, rel=1e-13)
    assert out["flux_r"][0, 3] == pytest.approx(vtr * qr * rho, rel=1e-13)
    assert 1.0 < vtr < 10.0


def test_reference_ice_level_with_gammas_of_its_own(consts):
    """One ice level inside the limits of M:1432-1438: cig(2) = Gamma(bm_i+mu_i+1) = Gamma(4), cig(3) = Gamma(5),
    oig1 = 1/Gamma(1), oig2 = 1/cig(2) (M:467-482)."""
    st = _column()
    qi, ni1 = 1.0e-5, 1.0e4
    st["qi"][0, 2], st["ni"][0, 2] = qi, ni1
    out = ref.fall_speeds(consts, st)
    rho = _rho(260.0)
    cig2, cig3, oig1 = math.gamma(4.0), math.gamma(5.0), 1.0 / math.gamma(1.0)
    oig2 = 1.0 / cig2
    lami = (ref.PI * 890.0 / 6.0 * cig2 * oig1 * (ni1 * rho) / (qi * rho)) ** (1.0 / 3.0)
    assert 5.0e-6 < 4.0 / lami < 300.0e-6                                        # not limited
    vti = math.sqrt(101325.0 / (287.05 * 298.0) / rho) * 1847.5 * cig3 * oig2 / lami
    assert out["vt_i"][0, 2] == pytest.approx(vti, rel=1e-13)
    assert out["flux_i"][0, 2] == pytest.approx(vti * qi * rho, rel=1e-13)
    assert out["flux_i"][0, 5] == 0.0 and out["flux_i"][0, 1] == out["vt_i"][0, 2] * 1.0e-12     # R1 where absent


def test_reference_inheritance_from_one_rain_level(consts):
    st = _column(nz=130, t=285.0)
    st["qr"][0, 70], st["nr"][0, 70] = 2.0e-3, 3.0e3
    out = ref.fall_speeds(consts, st)
    for n in ("vt_r", "vt_nr"):
        v = out[n][0]
        assert v[70] > 0 and (v[:70].view(np.uint64) == v[70:71].view(np.uint64)).all() and not v[71:].any()
    assert (ref.source_level(out["has_r"])[0] == np.where(np.arange(130) <= 70, 70, -1)).all()
    assert not out["vt_i"].any() and not out["vt_s"].any() and not out["vt_g"].any()


def test_reference_snow_takes_the_three_branches(consts):
    """M:3300-3305: at T_0 + 0.05 the plain product; at T_0 + 0.2 over fast rain the second argument of the MAX; at T_0 - 1
    the plain product with the default boost 1.0."""
    st = _column(nz=3)
    st["t"][0] = [ref.T_0 + 0.05, ref.T_0 + 0.2, ref.T_0 - 1.0]
    st["qs"][0] = 1.0e-3
    st["qr"][0], st["nr"][0] = 3.0e-3, 1.0e3
    out = ref.fall_speeds(consts, st)
    vts, vtr, got = out["vts0"][0], out["vt_r"][0], out["vt_s"][0]
    assert got[0] == vts[0] * 1.5
    second = vts[1] * ((vtr[1] - vts[1] * 1.5) / ((ref.T_0 + 0.2) - ref.T_0))
    assert got[1] == second and second > vts[1] * 1.5
    assert got[2] == vts[2] * 1.0
    boosted = ref.fall_speeds(consts, st, boost=np.full((1, 3), 1.25))
    assert boosted["vt_s"][0, 2] == vts[2] * 1.25 and boosted["vt_s"][0, 0] == vts[0] * 1.25


def test_reference_graupel_above_freezing_returns_the_rain_speed(consts):
    st = _column(nz=4, t=280.0)
    st["qg"][0, 1:3] = 1.0e-5
    st["qr"][0, 1], st["nr"][0, 1] = 5.0e-3, 5.0e2                               # fast rain at level 1 only
    out = ref.fall_speeds(consts, st)
    assert out["vt_g"][0, 1] == out["vt_r"][0, 1] > 5.0
    assert 0 < out["vt_g"][0, 2] < out["vt_r"][0, 1] and out["vt_r"][0, 2] == 0.0
    assert out["vt_g"][0, 0] == out["vt_g"][0, 1] and out["vt_g"][0, 3] == 0.0


@pytest.mark.parametrize("seed", fc.NSTEP_SEEDS)
def test_nstep_seeds_keep_clear_of_integers(consts, seed):
    """On the states of the GPU test for nstep, INT's argument is farther than 1e-9 relative from an integer at every
    level that attains a column's maximum: the GPU test's allowance is unused by the reference itself."""
    st, dz = fc.nstep_state(seed)
    out = ref.fall_speeds(consts, st, dz=dz, dt=fc.NSTEP_DT)
    arg, n = out["int_arg"], out["nstep"]
    assert n.shape == (fc.NSTEP_NCOL, 4) and (n >= 1).all() and n.max() > 20
    at_max = np.floor(np.where(np.isnan(arg), 0., arg)) == n[..., None]
    near = np.abs(arg - np.rint(arg)) <= 1e-9 * np.abs(arg)
    assert not (at_max & near & ~np.isnan(arg)).any()
    per_column = ref.fall_speeds(consts, st, dz=np.ascontiguousarray(np.broadcast_to(dz, st["t"].shape)), dt=fc.NSTEP_DT)
    assert np.array_equal(per_column["nstep"], n)
