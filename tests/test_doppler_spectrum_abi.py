"""The Doppler spectrum (include/kidmp_dspectrum.h, kid_amd/dspectrum.py) without a GPU: the four symbols exist in the
built library and in the new header, kid_amd/dspectrum.py declares them as the header has them, the header compiles as
C99 and C++11, a missing context is refused, the Python wrappers turn wrong arguments away before the library is called,
the position-to-slot function holds under ASan + UBSan as a host program, and the numpy reference of the GPU tests
(tests/doppler_spectrum_ref.py) converges to the closed forms of tests/doppler_ref.py and keeps the deposit's invariants.

Convergence, measured here (the assertions allow max(2 * measured, ROUNDING_FLOOR) with ROUNDING_FLOOR = 2e-13: a figure
at the level of rounding moves by more than its own size with a few ulp of numpy's exp and pow, so twice such a figure
is no bound; the floor binds for rain's and graupel's two velocity moments only):
  log-spaced 256 bins over [1e-6 m, 0.3 m] (geometric centres, widths the differences of the edges), eight hand-built
  levels per species (lamr 2.7e2..4.6e4, Mrat 2.7e2..5.0e3, lamg 4.6e2..6.7e3):
    |sum z_b/ze - 1|          rain 1.011e-4   snow 1.011e-4   graupel 1.011e-4   (h**2/24 of the width D*2 sinh(h/2) against
                                                                                   D*h, h = ln(3e5)/256: the same for all)
    |sum v z/sum z / vz - 1|  rain 7.6e-14    snow 2.03e-10   graupel 1.1e-15
    |sum v2 z/sum z / v2 - 1| rain 7.7e-14    snow 2.10e-10   graupel 2.0e-15
  the scheme's own 100 bins, the same levels, over the slopes for which the grid captures the echo:
    rain, lamr 2.4e3..4.6e4 (Dr = 50 um..5 mm):   4.43e-2, 9.14e-3, 1.82e-2 (both ends: -4.4e-2 at 2.4e3, -8.8e-3 at 4.6e4;
                                                  between 5e3 and 2.2e4 within 9e-5)
    snow, Mrat 2.7e2..2.2e3 (Ds = 200 um..2 cm):  8.11e-3, 4.68e-3, 6.73e-3
    graupel, lamg 4.6e2..6.7e3 (Dg = 250 um..5 cm): 1.65e-3, 1.34e-3, 1.67e-3
  outside those ranges the echo is missing, not misplaced: rain at lamr = 1.2e3 loses 64 % of ze, at 5.5e2 98 %, at 2.7e2
  all of it (the reflectivity-weighted mean diameter 7/lamr passes the grid's 5 mm); snow at Mrat = 5.0e3 loses 16 %
  (its small particles lie under Ds' 200 um).
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import doppler_ref as dref
import doppler_spectrum_ref as ref
import size_spectra_ref as ssr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_dspectrum.h")
SLOT_HEADER_DIR = os.path.join(ROOT, "kid_amd", "csrc")
SYMBOLS = ("kidmp_doppler_spectrum_device", "kidmp32_doppler_spectrum_device", "kidmp_doppler_spectrum_host", "kidmp32_doppler_spectrum_host")

SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "size_t": (C.c_size_t,), "double": (C.c_double,),
           "float": (C.c_float,), "int": (C.c_int, C.c_int32)}


def _code():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes():
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of the header (the method of
    test_doppler_abi.py)."""
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
    import kid_amd.dspectrum as kd
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
    for struct, elem in (("kidmp_dspectrum_out", "double"), ("kidmp32_dspectrum_out", "float")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _code(), re.S).group(1)
        assert body.split()[0] == elem
        members = [m.strip().lstrip("*") for m in body.replace(elem, "").replace(";", "").split(",")]
        assert tuple(members) == kd.DSPECTRUM_NAMES == kid_amd.DSPECTRUM_NAMES == ref.NAMES
    assert [n for n, _ in kd._DSpectrumOut._fields_] == list(kd.DSPECTRUM_NAMES) and all(t is C.c_void_p for _, t in kd._DSpectrumOut._fields_)
    assert kid_amd.DSPECTRUM_INPUTS == ref.INPUTS
    code = _code()
    assert int(re.search(r"#define KIDMP_DSPECTRUM_MAX_NV (\d+)", open(HEADER).read()).group(1)) == kd.DSPECTRUM_MAX_NV == 256
    assert int(re.search(r"#define KIDMP_DSPECTRUM_MAX_BINS (\d+)", open(HEADER).read()).group(1)) == kd.DSPECTRUM_MAX_BINS == 256
    assert "kidmp_dspectrum_grids" in code and len(kd.DSPECTRUM_SPECIES) == 3


def test_the_other_mirrors_do_not_declare_them():
    import kid_amd.doppler as dp
    import kid_amd.spectra as sp
    import kid_amd.thompson as th
    for other in (th, dp, sp):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_dspectrum.h"\n'
                   "int use(kidmp_ctx *c, const double *a, kidmp_dspectrum_grids *g, kidmp_dspectrum_out *o)\n"
                   "{ return kidmp_doppler_spectrum_host(c, 1, 2, a, a, a, a, a, a, a, 0, -2.0, 0.25, 64, g, o); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.dspectrum import _DSpectrumGrids, _DSpectrumOut, library
    L = library()
    o, g = _DSpectrumOut(), _DSpectrumGrids()
    args = [None, 4, 120] + [None] * 8 + [0.0, 0.1, 64, C.byref(g), C.byref(o)]
    assert L.kidmp_doppler_spectrum_host(*args) == -5                             # KIDMP_ESTATE
    assert L.kidmp32_doppler_spectrum_host(*args) == -5
    assert L.kidmp_doppler_spectrum_device(*args, None) == -5
    assert L.kidmp32_doppler_spectrum_device(*args, None) == -5


# ---- the position-to-slot function under ASan + UBSan, as a host program of its own ----
def test_slot_function_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "dspectrum_slot_check"
    # the sanitizers' runtimes are linked statically: the program is instrumented by itself and runs in the environment as it is
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
                   + static + ["-Wall", "-Wextra", "-Werror", "-I", SLOT_HEADER_DIR,
                               os.path.join(ROOT, "tests", "native", "dspectrum_slot_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("slot ok") and "runtime error" not in run.stderr, run.stdout + run.stderr


def test_reference_slot_is_the_header_function():
    nv = 7
    p = np.array([np.nan, -np.inf, np.inf, -1e308, 1e308, -1.0, -0.25, 0.0, 0.25, 3.0, 6.0, 6.5, 7.0, 7.5])
    j, f = ref.slot(p, nv)
    assert j.tolist() == [-1, -1, 6, -1, 6, -1, -1, 0, 0, 3, 6, 6, 6, 6]
    assert f.tolist() == [0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.75, 0.0, 0.25, 0.0, 0.0, 0.5, 1.0, 1.0]


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
GRID = dict(v0=-2.0, dv=0.25, nv=64)


def _host_state(dtype=np.float64, n=N, nz=NZ):
    return {k: np.zeros((n, nz), dtype=dtype) for k in ref.INPUTS}


def _host_cases():
    good = _host_state
    D = np.ones(10)
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
        ("unknown name", good(), dict(want=("total", "ice"))),
        ("a name twice", good(), dict(want=("rain", "rain"))),
        ("want a number", good(), dict(want=3)),
        ("nothing wanted", good(), dict(want=())),
        ("w shape", good(), dict(w=np.ones(NZ))),
        ("w dtype", good(), dict(w=np.ones((N, NZ), dtype=np.float32))),
        ("w a list", good(), dict(w=[[0.0] * NZ] * N)),
        ("nv = 0", good(), dict(nv=0)),
        ("nv = 257", good(), dict(nv=257)),
        ("nv a float", good(), dict(nv=64.0)),
        ("dv = 0", good(), dict(dv=0.0)),
        ("dv < 0", good(), dict(dv=-0.25)),
        ("dv NaN", good(), dict(dv=float("nan"))),
        ("dv inf", good(), dict(dv=float("inf"))),
        ("dv denormal", good(), dict(dv=5e-324)),
        ("v0 inf", good(), dict(v0=float("inf"))),
        ("v0 a string", good(), dict(v0="low")),
        ("grids a list", good(), dict(grids=[D, D])),
        ("grids unknown species", good(), dict(grids={"i": (D, D)})),
        ("grids half given", good(), dict(grids={"r": (D, None)})),
        ("grids not a pair", good(), dict(grids={"s": D})),
        ("grids nb = 0", good(), dict(grids={"g": (np.ones(0), np.ones(0))})),
        ("grids nb = 257", good(), dict(grids={"g": (np.ones(257), np.ones(257))})),
        ("grids sizes differ", good(), dict(grids={"r": (D, np.ones(11))})),
        ("grids float32", good(), dict(grids={"r": (D.astype(np.float32), D.astype(np.float32))})),
        ("grids two-dimensional", good(), dict(grids={"r": (np.ones((2, 5)), np.ones((2, 5)))})),
        ("out a list", good(), dict(out=[np.zeros((N, 64, NZ))])),
        ("out shape", good(), dict(out={"total": np.zeros((N, NZ, 64))})),
        ("out dtype", good(), dict(out={"total": np.zeros((N, 64, NZ), dtype=np.float32)})),
        ("out below shape", good(), dict(want=("below",), out={"below": np.zeros((N, 64, NZ))})),
    ]


@pytest.mark.parametrize("case", _host_cases(), ids=lambda c: c[0])
def test_host_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import doppler_spectrum_host
    _, st, kw = case
    kw = dict(GRID, **kw)
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="doppler_spectrum_host"):
        doppler_spectrum_host(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="doppler_spectrum_host"):
        _bare().doppler_spectrum_host(st, **kw)


def _device_cases():
    """Host tensors throughout: each case is wrong in one way and, being host memory, on the wrong device as well."""
    import torch
    good = lambda dt=torch.float64, nz=NZ: {k: torch.zeros(N, nz, dtype=dt) for k in ref.INPUTS}   # noqa: E731
    D = torch.ones(10, dtype=torch.float64)
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
        ("unknown name", good(), dict(want=("spectrum",))),
        ("a name twice", good(), dict(want=("snow", "total", "snow"))),
        ("nothing wanted", good(), dict(want=[])),
        ("w numpy", good(), dict(w=np.ones((N, NZ)))),
        ("w shape", good(), dict(w=torch.zeros(NZ, dtype=torch.float64))),
        ("w dtype", good(), dict(w=torch.zeros(N, NZ, dtype=torch.float32))),
        ("nv = 0", good(), dict(nv=0)),
        ("nv = 257", good(), dict(nv=257)),
        ("dv = 0", good(), dict(dv=0.0)),
        ("dv NaN", good(), dict(dv=float("nan"))),
        ("v0 NaN", good(), dict(v0=float("nan"))),
        ("grids numpy", good(), dict(grids={"r": (np.ones(10), np.ones(10))})),
        ("grids half given", good(), dict(grids={"r": (D, None)})),
        ("grids unknown species", good(), dict(grids={"c": (D, D)})),
        ("grids nb = 257", good(), dict(grids={"s": (torch.ones(257, dtype=torch.float64),) * 2})),
        ("out numpy", good(), dict(out={"total": np.zeros((N, 64, NZ))})),
    ]


@pytest.mark.parametrize("case", _device_cases(), ids=lambda c: c[0])
def test_device_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import doppler_spectrum
    _, st, kw = case
    kw = dict(GRID, **kw)
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="doppler_spectrum"):
        doppler_spectrum(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="doppler_spectrum"):
        _bare().doppler_spectrum(st, **kw)


def test_velocity_grid():
    from kid_amd import velocity_grid
    from kid_amd.thompson import KidmpError
    v = velocity_grid(-2.0, 0.25, 64)
    assert v.dtype == np.float64 and v.shape == (64,) and v[0] == -2.0 and v[1] == -1.75 and v[63] == -2.0 + 63 * 0.25
    for bad in ((0.0, 0.0, 4), (0.0, 0.1, 0), (0.0, 0.1, 257), (float("nan"), 0.1, 4)):
        with pytest.raises(KidmpError, match="velocity_grid"):
            velocity_grid(*bad)


# ---- the numpy reference ----
@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = dref.constants(o)
    o.close()
    return c


hand_levels, fine_grid, FINE_MEASURED = ref.hand_levels, ref.fine_grid, ref.FINE_MEASURED


def convergence(consts, x, D, dD):
    """(slope-like parameter, sum z/ze - 1, vz error, v2 error) per level of hand_levels(x) on the grid (D, dD)."""
    st = hand_levels(x)
    closed = dref.doppler_moments(consts, st)                 # one species per level: V = vz_x, m2 = v2_x
    lv = ref.levels(consts, st)
    s0, v1, v2 = ref.bin_moments(consts, st, x, D, dD)
    assert lv[x]["present"].all()
    slope = lv[x]["Mrat"] if x == "s" else lv[x]["lam"]
    return slope[0], s0[0] / lv[x]["ze"][0] - 1.0, v1[0] / closed["V"][0] - 1.0, v2[0] / closed["m2"][0] - 1.0


@pytest.mark.parametrize("x", ["r", "s", "g"])
def test_definitions_converge_on_a_fine_grid(consts, x):
    D, dD = fine_grid()
    slope, e0, e1, e2 = convergence(consts, x, D, dD)
    worst = tuple(float(np.abs(e).max()) for e in (e0, e1, e2))
    print("fine grid %s: slope %.3g..%.3g, max |sum z/ze - 1| %.3e, vz %.3e, v2 %.3e" % (x, slope.min(), slope.max(), *worst))
    for got, measured in zip(worst, FINE_MEASURED[x]):
        assert got <= max(2.0 * measured, ref.ROUNDING_FLOOR), (x, worst)


OWN_MEASURED = {"r": (4.43e-2, 9.14e-3, 1.82e-2), "s": (8.11e-3, 4.68e-3, 6.73e-3), "g": (1.65e-3, 1.34e-3, 1.67e-3)}
OWN_LEVELS = {"r": slice(3, 8), "s": slice(0, 5), "g": slice(0, 8)}   # the slopes for which the grid captures the echo


@pytest.mark.parametrize("x", ["r", "s", "g"])
def test_definitions_on_the_schemes_own_bins(consts, x):
    D, dD = ssr.default_grids()[x]
    slope, e0, e1, e2 = convergence(consts, x, D, dD)
    k = OWN_LEVELS[x]
    worst = tuple(float(np.abs(e[k]).max()) for e in (e0, e1, e2))
    print("own grid %s: slope %.3g..%.3g, max |sum z/ze - 1| %.3e, vz %.3e, v2 %.3e; sum z/ze - 1 of all levels %s"
          % (x, slope[k].min(), slope[k].max(), *worst, ["%.2e" % v for v in e0]))
    for got, measured in zip(worst, OWN_MEASURED[x]):
        assert got <= 2.0 * measured, (x, worst)
    if x == "r":
        assert (e0[:3] < -0.6).all()                          # what the grid does not capture is missing, not misplaced
    if x == "s":
        assert e0[7] < -0.15


# ---- the deposit's invariants ----
# The slots' sum and the bins' sum add the same mass in two orders: 2 x 300 parts against 300 terms.  A recursive sum of n
# positive terms carries a rounding error of about sqrt(n)/2 ulp of the sum, 12 and 9 here; measured: 4.6 ulp at the most.
SUM_ULPS = 16
@pytest.fixture(scope="module")
def mixed_state():
    import effrad_cases as ec
    st = ec.random_state(40, 12, 777)
    return {k: np.ascontiguousarray(st[k]) for k in ref.INPUTS}


def test_deposit_conserves_the_sum(consts, mixed_state):
    rng = np.random.Generator(np.random.PCG64(5))
    w = rng.uniform(-8.0, 8.0, mixed_state["t"].shape)
    out = ref.doppler_spectrum(consts, mixed_state, -1.0, 0.125, 48, w=w, default=ssr.default_grids())
    assert (out["below"] > 0).any() and (out["above"] > 0).any() and (out["total"] > 0).any()
    total = out["total"].sum(axis=1) + out["below"] + out["above"]
    want = out["sum_r"] + out["sum_s"] + out["sum_g"]
    eps = np.finfo(float).eps
    ulps = float(np.max(np.where(want > 0, np.abs(total - want) / np.where(want > 0, eps * want, 1.0), 0.0)))
    print("deposit: the slots' sum against the bins' sum, largest difference %.2f ulp of the sum" % ulps)
    assert (np.abs(total - want) <= SUM_ULPS * eps * want).all()
    for x, name in zip("rsg", ("rain", "snow", "graupel")):
        inside = (out["below"] == 0) & (out["above"] == 0)
        got = out[name].sum(axis=1)
        assert (np.abs(got - out["sum_" + x])[inside] <= SUM_ULPS * eps * out["sum_" + x][inside]).all(), name
    empty = want == 0
    assert empty.any() and not out["total"].transpose(0, 2, 1)[empty].view(np.uint64).any()


def test_deposit_conserves_the_first_moment_inside_the_grid(consts):
    st = hand_levels("r")
    v0, dv, nv = -1.0, 0.0625, 256
    out = ref.doppler_spectrum(consts, st, v0, dv, nv, default=ssr.default_grids(), want=("total", "below", "above"))
    assert not out["below"].any() and not out["above"].any()
    D, dD = ssr.default_grids()["r"]
    s0, v1, _ = ref.bin_moments(consts, st, "r", D, dD)
    vgrid = v0 + dv * np.arange(nv)
    got = (out["total"] * vgrid[None, :, None]).sum(axis=1) / out["total"].sum(axis=1)
    assert np.abs(got / v1 - 1.0).max() < 1e-13


def test_shifting_w_by_dv_shifts_the_spectrum_by_one_bin(consts, mixed_state):
    v0, dv, nv = -4.0, 0.25, 64                               # dv a power of two: v - w - dv is exact where v - w is
    w = np.full(mixed_state["t"].shape, 1.5)
    a = ref.doppler_spectrum(consts, mixed_state, v0, dv, nv, w=w, default=ssr.default_grids(), want=("total",))
    b = ref.doppler_spectrum(consts, mixed_state, v0, dv, nv, w=w + dv, default=ssr.default_grids(), want=("total",))
    assert (a["total"] > 0).any()
    scale = a["total"].sum(axis=1, keepdims=True)            # an ulp of the position moves an ulp of the level's echo
    assert (np.abs(b["total"][:, 1:nv - 3, :] - a["total"][:, 2:nv - 2, :]) <= 1e-13 * scale).all()
