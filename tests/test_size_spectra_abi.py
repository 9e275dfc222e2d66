"""The size spectra (include/kidmp_spectra.h, kid_amd/spectra.py) without a GPU: the five symbols exist in the built
library and in the new header, kid_amd/spectra.py declares them as the header has them, the header compiles as C99 and
C++11, a missing context is refused, the Python wrappers turn wrong arguments away before the library is called, and the
numpy reference of the GPU tests (tests/size_spectra_ref.py) gives known answers formed independently of the kernel."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import effrad_cases as ec
import size_spectra_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_spectra.h")
ENTRIES = ("kidmp_size_spectra_device", "kidmp32_size_spectra_device", "kidmp_size_spectra_host", "kidmp32_size_spectra_host")
SYMBOLS = ENTRIES + ("kidmp_spectra_default_grid",)

SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "size_t": (C.c_size_t,), "double": (C.c_double,),
           "float": (C.c_float,), "int": (C.c_int, C.c_int32)}


def _code():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes():
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of the header (the method of
    test_fall_speeds_abi.py)."""
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
    import kid_amd.spectra as ks
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
        if e.restype not in SCALARS[ret]:
            wrong.append("%s: returns `%s`, declared %s" % (name, ret, getattr(e.restype, "__name__", e.restype)))
    assert not wrong, "\n".join(wrong)
    code = _code()
    for struct, elem, names in (("kidmp_spectra_out", "double", ks.SPECTRA_PARAMS), ("kidmp32_spectra_out", "float", ks.SPECTRA_PARAMS),
                                ("kidmp_spectra_bins", "double", tuple("n_" + x for x in ks.SPECTRA_SPECIES)),
                                ("kidmp32_spectra_bins", "float", tuple("n_" + x for x in ks.SPECTRA_SPECIES))):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, re.S).group(1)
        assert body.split()[0] == elem
        members = [m.strip().lstrip("*") for m in body.replace(elem, "").replace(";", "").split(",")]
        assert tuple(members) == names, struct
    assert ks.SPECTRA_PARAMS == kid_amd.SPECTRA_PARAMS == ref.PARAMS and ks.SPECTRA_SPECIES == kid_amd.SPECTRA_SPECIES == ref.SPECIES
    assert kid_amd.SPECTRA_INPUTS == ref.INPUTS == ec.NAMES
    assert [n for n, _ in ks._SpectraOut._fields_] == list(ks.SPECTRA_PARAMS) and all(t is C.c_void_p for _, t in ks._SpectraOut._fields_)
    assert [n for n, _ in ks._SpectraBins._fields_] == ["n_" + x for x in ks.SPECTRA_SPECIES]
    # the grids: two arrays of KIDMP_SPECTRA_NSPECIES pointers and one of int32, in the header's order; the macros
    macro = dict(re.findall(r"#define (KIDMP_SPECTRA_\w+) (\d+)", open(HEADER).read()))
    assert int(macro["KIDMP_SPECTRA_NSPECIES"]) == len(ks.SPECTRA_SPECIES) == 5
    assert int(macro["KIDMP_SPECTRA_MAX_BINS"]) == ks.SPECTRA_MAX_BINS == ref.MAX_BINS == 256
    assert int(macro["KIDMP_SPECTRA_DEFAULT_BINS"]) == ks.SPECTRA_DEFAULT_BINS == ref.DEFAULT_BINS == ref.nbins
    assert [int(macro["KIDMP_SPECTRA_" + x.upper()]) for x in ks.SPECTRA_SPECIES] == [0, 1, 2, 3, 4]
    body = " ".join(re.search(r"typedef struct kidmp_spectra_grids \{(.*?)\} kidmp_spectra_grids;", code, re.S).group(1).split())
    assert body == ("const double *D[KIDMP_SPECTRA_NSPECIES]; const double *dD[KIDMP_SPECTRA_NSPECIES]; int32_t nb[KIDMP_SPECTRA_NSPECIES];")
    assert [(n, t._length_, t._type_) for n, t in ks._SpectraGrids._fields_] == [("D", 5, C.c_void_p), ("dD", 5, C.c_void_p), ("nb", 5, C.c_int32)]
    assert C.sizeof(ks._SpectraGrids) == 5 * 8 + 5 * 8 + 5 * 4 + 4


def test_the_other_mirrors_do_not_declare_them():
    import kid_amd.fall as kf
    import kid_amd.stats as st
    import kid_amd.summary as sm
    import kid_amd.thompson as th
    for other in (th, st, sm, kf):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_spectra.h"\n'
                   "int use(kidmp_ctx *c, const double *a, kidmp_spectra_out *o, kidmp_spectra_bins *b, kidmp_spectra_grids *g, double *d)\n"
                   "{ g->nb[KIDMP_SPECTRA_R] = kidmp_spectra_default_grid(c, KIDMP_SPECTRA_R, d, d, KIDMP_SPECTRA_MAX_BINS);\n"
                   "  return kidmp_size_spectra_host(c, 1, 2, a, a, a, a, 0, a, a, a, a, a, a, o, b, g); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.spectra import _SpectraBins, _SpectraGrids, _SpectraOut, library
    L = library()
    o, b, g = _SpectraOut(), _SpectraBins(), _SpectraGrids()
    args = [None, 4, 120] + [None] * 11 + [C.byref(o), C.byref(b), C.byref(g)]
    assert L.kidmp_size_spectra_host(*args) == -5                                # KIDMP_ESTATE
    assert L.kidmp32_size_spectra_host(*args) == -5
    assert L.kidmp_size_spectra_device(*args, None) == -5
    assert L.kidmp32_size_spectra_device(*args, None) == -5
    assert L.kidmp_spectra_default_grid(None, 2, None, None, 0) == -5


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
    D = np.linspace(1e-4, 1e-3, 7)
    return [
        ("not a dict", [np.zeros((N, NZ))], {}),
        ("torch for numpy", {k: __import__("torch").zeros(N, NZ, dtype=__import__("torch").float64) for k in ref.INPUTS}, {}),
        ("float16", _host_state(np.float16), {}),
        ("one-dimensional", {k: np.zeros(NZ) for k in ref.INPUTS}, {}),
        ("nz = 1", _host_state(nz=1), {}),
        ("nz = 257", _host_state(nz=257), {}),
        ("qr missing", {k: v for k, v in good().items() if k != "qr"}, {}),
        ("qc missing", {k: v for k, v in good().items() if k != "qc"}, {}),
        ("mixed dtypes", dict(good(), qi=np.zeros((N, NZ), dtype=np.float32)), {}),
        ("shapes differ", dict(good(), qr=np.zeros((N, NZ + 1))), {}),
        ("not contiguous", dict(good(), p=np.zeros((NZ, N)).T), {}),
        ("unknown name", good(), dict(want=("r", "lam_x"))),
        ("a name twice", good(), dict(want=("r", "r"))),
        ("want a number", good(), dict(want=3)),
        ("nothing wanted", good(), dict(want=())),
        ("grids a list", good(), dict(grids=[(D, D)])),
        ("grids of an unknown species", good(), dict(grids={"x": (D, D)})),
        ("a grid that is no pair", good(), dict(grids={"r": D})),
        ("a grid of lists", good(), dict(grids={"r": (list(D), list(D))})),
        ("D and dD differ in length", good(), dict(grids={"r": (D, D[:-1].copy())})),
        ("a grid in binary32", good(), dict(grids={"r": (D.astype(np.float32), D.astype(np.float32))})),
        ("a grid of 257 bins", good(), dict(grids={"r": (np.ones(257), np.ones(257))})),
        ("an empty grid", good(), dict(grids={"r": (np.ones(0), np.ones(0))})),
        ("a two-dimensional grid", good(), dict(grids={"r": (np.ones((2, 3)), np.ones((2, 3)))})),
        ("a strided grid", good(), dict(grids={"r": (np.ones(14)[::2], np.ones(7))})),
        ("out a list", good(), dict(out=[np.zeros((N, 100, NZ))])),
        ("out of the wrong shape", good(), dict(want=("r",), out={"r": np.zeros((N, NZ, 100))})),
        ("out of the wrong dtype", good(), dict(want=("lam_r",), out={"lam_r": np.zeros((N, NZ), dtype=np.float32)})),
    ]


@pytest.mark.parametrize("case", _host_cases(), ids=lambda c: c[0])
def test_host_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import size_spectra_host
    _, st, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="size_spectra_host"):
        size_spectra_host(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="size_spectra_host"):
        _bare().size_spectra_host(st, **kw)


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
        ("unknown name", good(), dict(want=("n0",))),
        ("a numpy grid", good(), dict(grids={"r": (np.ones(3), np.ones(3))})),
        ("out numpy", good(), dict(want=("r",), out={"r": np.zeros((N, 100, NZ))})),
    ]


@pytest.mark.parametrize("case", _device_cases(), ids=lambda c: c[0])
def test_device_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import size_spectra
    _, st, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="size_spectra"):
        size_spectra(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="size_spectra"):
        _bare().size_spectra(st, **kw)


def test_default_grid_refuses_an_unknown_species_before_the_library(monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import default_grid
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="default_grid"):
        default_grid(_bare(), "x")


# ---- the numpy reference: known answers formed independently of the kernel ----
@pytest.fixture(scope="module")
def consts():
    return ref.constants()


@pytest.fixture(scope="module")
def grids():
    return ref.default_grids()


def test_reference_grids_equal_the_oracles(grids):
    """M:605-657 in numpy against the C oracle's bins (oracle/thompson_oracle_init.c, make_bins): Dc/dtc are sums of 1e-6 and
    equal bit for bit; the others go through EXP and LOG of arguments up to ~12 in magnitude, where one ulp of the argument
    is 12 ulp of the value: 2e-14 relative covers two libms."""
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    try:
        for x, (d, dt) in dict(c=("Dc", "dtc"), i=("Di", "dti"), r=("Dr", "dtr"), s=("Ds", "dts"), g=("Dg", "dtg")).items():
            D, dD = grids[x]
            assert D.shape == dD.shape == (100,) and (np.diff(D) > 0).all() and (dD > 0).all()
            tol = 0.0 if x == "c" else 2e-14
            assert np.abs(o.const(d) / D - 1).max() <= tol and np.abs(o.const(dt) / dD - 1).max() <= tol, x
    finally:
        o.close()
    assert grids["c"][0][0] == 1e-6 and grids["c"][0][-1] == pytest.approx(100e-6, rel=1e-13)
    assert grids["r"][0][0] == pytest.approx(math.sqrt(50e-6 * 50e-6 * 100 ** 0.01), rel=1e-13)
    assert grids["g"][1].sum() == pytest.approx(0.05 - 250e-6, rel=1e-13)


def _column(n, t=260.0, p=6.0e4, qv=1.0e-3):
    st = {k: np.zeros((n, 2)) for k in ref.INPUTS}
    st["t"][:], st["p"][:], st["qv"][:] = t, p, qv
    return st, 0.622 * p / (287.04 * t * (qv + 0.622))


def test_reference_rain_mass_is_captured(consts, grids):
    """Sum_b am_r D_b**3 N_r(b) within 0.4 % of rr for mvd_r in [3e-4, 1e-3] m on the scheme's grid (the worst is 0.35 %).
    The number is not asserted: the grid starts at 50 um."""
    n = 64
    st, rho = _column(n, t=285.0, p=9.0e4, qv=5.0e-3)
    mvd = np.linspace(3e-4, 1e-3, n)
    qr = 1.0e-3
    nr = math.gamma(1.0) / math.gamma(4.0) * (qr * rho) * (3.672 / mvd) ** 3 / (ref.PI * 1000.0 / 6.0)   # M:1459 solved for nr
    st["qr"][:, 0], st["nr"][:, 0] = qr, nr / rho
    out = ref.size_spectra(consts, st, want=("r",), warm=True)
    assert np.allclose(3.672 / out["lam_r"][:, 0], mvd, rtol=1e-12)              # not limited
    D = grids["r"][0]
    mass = (ref.PI * 1000.0 / 6.0 * D[None, :] ** 3 * out["r"][:, :, 0]).sum(axis=1)
    err = np.abs(mass / (qr * rho) - 1)
    print("rain: captured mass off by up to %.3g" % err.max())
    assert err.max() <= 0.004
    assert not out["r"][:, :, 1].any() and not out["lam_r"][:, 1].any()           # the level without rain


def test_reference_graupel_mass_is_captured(consts, grids):
    """The same for graupel with 1/lamg in [5e-4, 3e-3] m."""
    n = 200
    st, rho = _column(n)
    st["qg"][:, 0] = np.logspace(-5, -1.6, n)
    out = ref.size_spectra(consts, st, want=("g",))
    ilamg = 1.0 / out["lam_g"][:, 0]
    sel = (ilamg >= 5e-4) & (ilamg <= 3e-3)
    assert sel.sum() > 20 and ilamg[sel].min() < 5.5e-4 and ilamg[sel].max() > 2.5e-3
    D = grids["g"][0]
    mass = (ref.PI * 500.0 / 6.0 * D[None, :] ** 3 * out["g"][:, :, 0]).sum(axis=1)
    err = np.abs(mass / (st["qg"][:, 0] * rho) - 1)[sel]
    print("graupel: captured mass off by up to %.3g" % err.max())
    assert err.max() <= 0.004


# measured with this reference on the PSDs below (printed by the tests): cloud water 8.5e-10, cloud ice 1.9e-3, snow 8.8e-3;
# each bound is twice the measured value
CAPTURED = {"c": 1.7e-9, "i": 3.8e-3, "s": 1.76e-2}


def test_reference_cloud_water_mass_is_captured(consts, grids):
    """Droplets well inside the 1..100 um grid: Nt_c = 100 cm-3 and qc from 0.1 to 1 g/kg (mean volume diameters 12..26 um)."""
    n = 32
    st, rho = _column(n, t=280.0, p=8.0e4, qv=6.0e-3)
    st["qc"][:, 0] = np.linspace(1e-4, 1e-3, n)
    out = ref.size_spectra(consts, st, want=("c",), warm=True)
    assert (out["nu_c"][:, 0] == 12).all()                                       # NINT(1000.E6/100.E6) + 2
    D = grids["c"][0]
    mass = (ref.PI * 1000.0 / 6.0 * D[None, :] ** 3 * out["c"][:, :, 0]).sum(axis=1)
    number = out["c"][:, :, 0].sum(axis=1)
    err = np.abs(mass / (st["qc"][:, 0] * rho) - 1)
    print("cloud water: captured mass off by up to %.3g, number by up to %.3g" % (err.max(), np.abs(number / 100e6 - 1).max()))
    assert err.max() <= CAPTURED["c"]


def test_reference_cloud_ice_mass_is_captured(consts, grids):
    """Ice with mean size 4/lami in [100, 150] um, inside the limits of M:1432-1438 and the 13 um .. 1 mm grid."""
    n = 32
    st, rho = _column(n, t=245.0)
    xDi = np.linspace(100e-6, 150e-6, n)
    qi = 1.0e-5
    ni = math.gamma(1.0) / math.gamma(4.0) * (qi * rho) / (ref.PI * 890.0 / 6.0) * (4.0 / xDi) ** 3
    st["qi"][:, 0], st["ni"][:, 0] = qi, ni / rho
    out = ref.size_spectra(consts, st, want=("i",))
    assert np.allclose(4.0 / out["lam_i"][:, 0], xDi, rtol=1e-12)                # not limited
    D = grids["i"][0]
    mass = (ref.PI * 890.0 / 6.0 * D[None, :] ** 3 * out["i"][:, :, 0]).sum(axis=1)
    err = np.abs(mass / (qi * rho) - 1)
    print("cloud ice: captured mass off by up to %.3g" % err.max())
    assert err.max() <= CAPTURED["i"]


def test_reference_snow_mass_is_captured(consts, grids):
    """Heavy snow of 5 to 10 g/kg at 268 K, whose mass sits above the grid's first bin at 200 um (lighter or colder snow
    keeps a tenth and more of its mass below it): the second moment of the bins, am_s Sum D**2 N_s, against rs."""
    n = 32
    st, rho = _column(n, t=268.0)
    st["qs"][:, 0] = np.linspace(5e-3, 1e-2, n)
    out = ref.size_spectra(consts, st, want=("s",))
    D = grids["s"][0]
    mass = (0.069 * D[None, :] ** 2 * out["s"][:, :, 0]).sum(axis=1)
    err = np.abs(mass / (st["qs"][:, 0] * rho) - 1)
    print("snow: captured mass off by up to %.3g" % err.max())
    assert err.max() <= CAPTURED["s"]
    assert np.array_equal(out["smob"][:, 0], st["qs"][:, 0] * rho * (1.0 / 0.069))


def test_reference_applies_the_700_rule(consts, grids):
    """An exponential whose argument exceeds 700 is exact +0.0; just below it the bin is a normal number."""
    st, rho = _column(1)
    st["qi"][0, 0], st["ni"][0, 0] = 1.0e-9, 1.0e9 / rho                         # limited to xDi = 5 um: lami = 8e5
    out = ref.size_spectra(consts, st, want=("i",))
    lami = out["lam_i"][0, 0]
    assert lami == pytest.approx(4.0 / 5e-6, rel=1e-12)
    arg = lami * grids["i"][0]
    assert arg.max() > 780 and arg.min() < 20
    N = out["i"][0, :, 0]
    assert (N[arg > 700] == 0).all() and not np.signbit(N).any() and (N[arg <= 700] > 1e-300).all() and (arg > 700).sum() >= 2
    assert np.array_equal(out["i_arg"][0, :, 0], arg)
