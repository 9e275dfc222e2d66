"""The bright band (include/kidmp_brightband.h, kid_amd/brightband.py) without a GPU: the four entries (and the helper that
writes the default configuration) exist in the built library and in the new header, kid_amd/brightband.py declares them as
the header has them, the header compiles as C99 and C++11, a missing context is refused, the Python wrappers turn wrong
arguments away before the library is called, the defaults are the stated ones, the per-particle mixing model
(kid_amd/csrc/kidmp_brightband_mix.h) gives the same text as a host program with and without ASan + UBSan, and the numpy
reference of the GPU tests (tests/bright_band_ref.py) behaves as recorded here.

The enhancement E_x = (sum n s)/(sum n s0) of the reference on the scheme's own 100 bins, for the eight hand-built levels
of doppler_spectrum_ref.hand_levels (snow: Mrat 2.7e2 .. 5.0e3; graupel: lamg 4.6e2 .. 6.7e3), first .. last level:

                        fm    snow, default eps_w    graupel     | eps_w = 1 (vacuum): E/(1-fm)**2 - 1, largest
  water is the matrix   0.05  7.888 .. 4.031         3.333       | snow 3.3e-15   graupel 2.2e-16
                        0.25  84.99 .. 12.44         8.088       | snow 2.4e-15   graupel 5.6e-16
                        0.5   208.1 .. 12.50         8.041       | snow 3.7e-15   graupel 4.4e-16
                        0.75  205.9 .. 8.501         6.297       | snow 1.1e-15   graupel 1.1e-15
                        0.99  8.988 .. 4.445         4.376       | snow 4.9e-15   graupel 2.6e-14
  the core is the matrix 0.05 1.115 .. 1.169         1.181       | snow 2.8e-3    graupel 4.5e-3
                        0.25  1.638 .. 1.924         1.979       | snow 1.6e-2    graupel 2.6e-2
                        0.5   2.431 .. 2.952         3.015       | snow 3.9e-2    graupel 6.1e-2
                        0.75  3.374 .. 3.869         3.874       | snow 7.4e-2    graupel 1.2e-1
                        0.99  4.305 .. 4.299         4.293       | snow 1.3e-1    graupel 2.0e-1

What the table shows and the tests assert: E is finite and positive everywhere; graupel's E does not depend on the level
(every volume of a graupel particle goes with D**3, so the ratio is the same in every bin); towards fm = 1 both
topologies tend to |K_w|**2/0.176 * (rho_i/rho_w)**2 = 4.30, the water sphere of the melted mass; with water as the matrix
the vacuum limit E = (1 - fm)**2 holds to rounding (the largest figure is cancellation in eps_p - 1 at fm = 0.99).  With
the ice-air core as the matrix the vacuum limit is NOT an identity -- Maxwell-Garnett is not symmetric in matrix and
inclusion, and vacuum inclusions in a matrix of eps_c do not give K(eps_p) V = K(eps_c) c -- and holds only to the figures
of the last column, largest for dense particles; the assertion there is 4 x those figures.
"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bright_band_ref as ref
import doppler_ref as dref
import doppler_spectrum_ref as dsr
import refl_oracle as ro
import size_spectra_ref as ssr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_brightband.h")
MIX_HEADER_DIR = os.path.join(ROOT, "kid_amd", "csrc")
ENTRIES = ("kidmp_bright_band_device", "kidmp32_bright_band_device", "kidmp_bright_band_host", "kidmp32_bright_band_host")
SYMBOLS = ENTRIES + ("kidmp_brightband_defaults",)

SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "size_t": (C.c_size_t,), "double": (C.c_double,),
           "float": (C.c_float,), "int": (C.c_int, C.c_int32), "void": (None,)}

FMS = (0.05, 0.25, 0.5, 0.75, 0.99)
# the last column of the table: |E/(1-fm)**2 - 1| of the vacuum limit with the core as the matrix, snow and graupel
ICE_MATRIX_VACUUM = {0.05: (2.82e-3, 4.53e-3), 0.25: (1.60e-2, 2.57e-2), 0.5: (3.87e-2, 6.14e-2), 0.75: (7.36e-2, 1.15e-1),
                     0.99: (1.32e-1, 1.98e-1)}
ULP = 2.220446049250313e-16


def _code():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes():
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of the header (the method of
    test_doppler_spectrum_abi.py)."""
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
    import kid_amd.brightband as kb
    declared = kb.declare(_Stub()).entries
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
    for struct, elem in (("kidmp_brightband_out", "double"), ("kidmp32_brightband_out", "float")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _code(), re.S).group(1)
        assert body.split()[0] == elem
        members = [m.strip().lstrip("*") for m in re.sub(r"\b(%s|int32_t)\b" % elem, "", body).replace(";", ",").split(",") if m.strip()]
        assert tuple(members) == kb.BRIGHTBAND_NAMES == kid_amd.BRIGHTBAND_NAMES == ref.NAMES
    assert [n for n, _ in kb._BrightBandOut._fields_] == list(kb.BRIGHTBAND_NAMES) and all(t is C.c_void_p for _, t in kb._BrightBandOut._fields_)
    cfg = re.search(r"typedef struct kidmp_brightband_cfg \{(.*?)\} kidmp_brightband_cfg;", _code(), re.S).group(1)
    names = [m.strip() for m in re.sub(r"\b(double|int32_t)\b", "", cfg).replace(";", ",").split(",") if m.strip()]
    assert names == [n for n, _ in kb._BrightBandCfg._fields_]
    assert [t for _, t in kb._BrightBandCfg._fields_] == [C.c_double] * 6 + [C.c_int32]
    assert kid_amd.BRIGHTBAND_INPUTS == ref.INPUTS
    raw = open(HEADER).read()
    assert int(re.search(r"#define KIDMP_BB_MAX_BINS (\d+)", raw).group(1)) == kb.BRIGHTBAND_MAX_BINS == 256
    assert int(re.search(r"#define KIDMP_BB_WATER_MATRIX (\d+)", raw).group(1)) == kb.WATER_MATRIX == ref.WATER_MATRIX
    assert int(re.search(r"#define KIDMP_BB_ICE_MATRIX (\d+)", raw).group(1)) == kb.ICE_MATRIX == ref.ICE_MATRIX
    assert int(re.search(r"#define KIDMP_BB_NSPECIES (\d+)", raw).group(1)) == len(kb.BRIGHTBAND_SPECIES) == 2


def test_the_other_mirrors_do_not_declare_them():
    import kid_amd.doppler as dp
    import kid_amd.dspectrum as ds
    import kid_amd.thompson as th
    for other in (th, dp, ds):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_brightband.h"\n'
                   "int use(kidmp_ctx *c, const double *a, kidmp_brightband_cfg *f, kidmp_brightband_grids *g, kidmp_brightband_out *o)\n"
                   "{ kidmp_brightband_defaults(f); f->topology = KIDMP_BB_ICE_MATRIX;\n"
                   "  return kidmp_bright_band_host(c, 1, 2, a, a, a, a, a, a, a, f, g, o); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.brightband import _BrightBandGrids, _BrightBandOut, library
    L = library()
    o, g = _BrightBandOut(), _BrightBandGrids()
    args = [None, 4, 120] + [None] * 7 + [None, C.byref(g), C.byref(o)]
    assert L.kidmp_bright_band_host(*args) == -5                                  # KIDMP_ESTATE
    assert L.kidmp32_bright_band_host(*args) == -5
    assert L.kidmp_bright_band_device(*args, None) == -5
    assert L.kidmp32_bright_band_device(*args, None) == -5


def test_the_defaults():
    """eps_i gives |K_i|**2 = 0.176 within 2 ulp, eps_w gives |K_w|**2 = 0.934 to three digits; the library, the Python
    mirror and the reference hold the same numbers."""
    from kid_amd.brightband import BrightBandCfg, _BrightBandCfg, default_eps_i, library
    c = _BrightBandCfg()
    library().kidmp_brightband_defaults(C.byref(c))
    py = BrightBandCfg()
    assert (c.eps_w_re, c.eps_w_im, c.rho_w, c.rho_i, c.kw2, c.topology) == (79.5, 24.9, 1000.0, 900.0, 0.93, 0)
    assert (py.eps_w, py.rho_w, py.rho_i, py.kw2, py.topology) == (complex(79.5, 24.9), 1000.0, 900.0, 0.93, 0)
    assert c.eps_i == py.eps_i == default_eps_i() == ref.default_eps_i()
    ki = (c.eps_i - 1.0) / (c.eps_i + 2.0)
    assert abs(ki * ki - 0.176) <= 2 * 2.0 ** -55, ki * ki                      # 2 ulp: an ulp of 0.176 is 2**-55
    kr, kim = ref.cK(79.5, 24.9)
    assert "%.3f" % (kr * kr + kim * kim) == "0.934"


# ---- the mixing model as a host program of its own, with and without ASan + UBSan ----
def test_mixing_model_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    # the sanitizers' runtimes are linked statically: the program is instrumented by itself and runs in the environment as it is
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else ["-static-libsan"]
    common = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", MIX_HEADER_DIR,
              os.path.join(ROOT, "tests", "native", "brightband_mix_check.cpp")]
    san, plain = tmp_path / "mix_san", tmp_path / "mix_plain"
    subprocess.run(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + static
                   + ["-o", str(san)], check=True)
    subprocess.run(common + ["-o", str(plain)], check=True)
    a = subprocess.run([str(san)], capture_output=True, text=True)
    b = subprocess.run([str(plain)], capture_output=True, text=True)
    assert a.returncode == 0 and a.stdout.strip().endswith("mix ok") and "runtime error" not in a.stderr, a.stdout[-2000:] + a.stderr
    assert b.returncode == 0 and a.stdout == b.stdout and len(a.stdout.splitlines()) > 1500


def test_reference_mixing_is_the_header_function(tmp_path):
    """tests/bright_band_ref.py and kidmp_brightband_mix.h give the same bits: the host program's hex floats are parsed
    and recomputed."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    exe = tmp_path / "mix"
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", MIX_HEADER_DIR,
                    os.path.join(ROOT, "tests", "native", "brightband_mix_check.cpp"), "-o", str(exe)], check=True)
    lines = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    rows = [ln for ln in lines if len(ln) == 6 and ln[0] in "01"]
    assert len(rows) == 2 * 2 * 65 * 3
    for topo, sp, D, fm, w, _ in rows:
        cfg = ref.default_cfg(topology=int(topo))
        D, fm, w = float.fromhex(D), float.fromhex(fm), float.fromhex(w)
        b = ref.bin_consts(cfg, "sg"[int(sp)], D)
        assert float(ref.wet(cfg, b, np.float64(fm))) == w, (topo, sp, D, fm)


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


def _cfg(**kw):
    from kid_amd import BrightBandCfg
    return BrightBandCfg(**kw)


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
        ("unknown name", good(), dict(want=("dbz", "dbz_r"))),
        ("a name twice", good(), dict(want=("enh_s", "enh_s"))),
        ("want a number", good(), dict(want=3)),
        ("nothing wanted", good(), dict(want=())),
        ("cfg a dict", good(), dict(cfg={"topology": 0})),
        ("cfg eps_w NaN", good(), dict(cfg=_cfg(eps_w=complex(float("nan"), 0.0)))),
        ("cfg eps_w a string", good(), dict(cfg=_cfg(eps_w="water"))),
        ("cfg eps_i inf", good(), dict(cfg=_cfg(eps_i=float("inf")))),
        ("cfg rho_w = 0", good(), dict(cfg=_cfg(rho_w=0.0))),
        ("cfg rho_i < 0", good(), dict(cfg=_cfg(rho_i=-900.0))),
        ("cfg kw2 = 0", good(), dict(cfg=_cfg(kw2=0.0))),
        ("cfg kw2 NaN", good(), dict(cfg=_cfg(kw2=float("nan")))),
        ("cfg topology 2", good(), dict(cfg=_cfg(topology=2))),
        ("cfg topology a bool", good(), dict(cfg=_cfg(topology=True))),
        ("grids a list", good(), dict(grids=[D, D])),
        ("grids unknown species", good(), dict(grids={"r": (D, D)})),
        ("grids half given", good(), dict(grids={"s": (D, None)})),
        ("grids not a pair", good(), dict(grids={"s": D})),
        ("grids nb = 0", good(), dict(grids={"g": (np.ones(0), np.ones(0))})),
        ("grids nb = 257", good(), dict(grids={"g": (np.ones(257), np.ones(257))})),
        ("grids sizes differ", good(), dict(grids={"s": (D, np.ones(11))})),
        ("grids float32", good(), dict(grids={"s": (D.astype(np.float32), D.astype(np.float32))})),
        ("grids two-dimensional", good(), dict(grids={"g": (np.ones((2, 5)), np.ones((2, 5)))})),
        ("out a list", good(), dict(out=[np.zeros((N, NZ))])),
        ("out shape", good(), dict(out={"dbz": np.zeros((NZ, N))})),
        ("out dtype", good(), dict(out={"dbz": np.zeros((N, NZ), dtype=np.float32)})),
        ("out k0 dtype", good(), dict(want=("k0",), out={"k0": np.zeros(N, dtype=np.int64)})),
        ("out k0 shape", good(), dict(want=("k0",), out={"k0": np.zeros((N, NZ), dtype=np.int32)})),
    ]


@pytest.mark.parametrize("case", _host_cases(), ids=lambda c: c[0])
def test_host_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import bright_band_host
    _, st, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="bright_band_host"):
        bright_band_host(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="bright_band_host"):
        _bare().bright_band_host(st, **kw)


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
        ("nz = 1", good(nz=1), {}),
        ("nz = 257", good(nz=257), {}),
        ("qr missing", {k: v for k, v in good().items() if k != "qr"}, {}),
        ("mixed dtypes", dict(good(), qg=torch.zeros(N, NZ, dtype=torch.float32)), {}),
        ("unknown name", good(), dict(want=("bright",))),
        ("a name twice", good(), dict(want=("k0", "dbz", "k0"))),
        ("nothing wanted", good(), dict(want=[])),
        ("cfg a tuple", good(), dict(cfg=(79.5, 24.9))),
        ("cfg rho_w NaN", good(), dict(cfg=_cfg(rho_w=float("nan")))),
        ("cfg topology -1", good(), dict(cfg=_cfg(topology=-1))),
        ("grids numpy", good(), dict(grids={"s": (np.ones(10), np.ones(10))})),
        ("grids half given", good(), dict(grids={"g": (D, None)})),
        ("grids unknown species", good(), dict(grids={"c": (D, D)})),
        ("grids nb = 257", good(), dict(grids={"s": (torch.ones(257, dtype=torch.float64),) * 2})),
        ("out numpy", good(), dict(out={"dbz": np.zeros((N, NZ))})),
    ]


@pytest.mark.parametrize("case", _device_cases(), ids=lambda c: c[0])
def test_device_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import bright_band
    _, st, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="bright_band"):
        bright_band(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="bright_band"):
        _bare().bright_band(st, **kw)


# ---- the numpy reference on hand-built levels: the table of the module docstring ----
@pytest.fixture(scope="module")
def consts():
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = dref.constants(o)
    o.close()
    return c


def _parameters(consts, x):
    st = dsr.hand_levels(x)
    _, _, _, v, ilamg, N0_g = ro.ze_terms(consts, st["qv"], st["qr"], st["nr"], st["qs"], st["qg"], st["t"], st["p"])
    if x == "s":
        smoc, smob = dref.snow_smoc(consts, v["temp"], v["rs"])
        return dict(smob=smob, smoc=smoc), st["t"].shape
    return dict(N0=N0_g, lam=1.0 / ilamg), st["t"].shape


@pytest.mark.parametrize("x", ref.SPECIES)
def test_enhancement_of_the_reference_on_hand_built_levels(consts, x):
    own = ssr.default_grids()
    par, shape = _parameters(consts, x)
    k_w2 = sum(k * k for k in ref.cK(79.5, 24.9))
    for topo, name in ((ref.WATER_MATRIX, "water matrix"), (ref.ICE_MATRIX, "ice matrix")):
        for fm in FMS:
            E = ref.enhancement(ref.default_cfg(topology=topo), x, par, np.full(shape, fm), *own[x])[0]
            V = ref.enhancement(ref.default_cfg(topology=topo, eps_w=complex(1.0, 0.0)), x, par, np.full(shape, fm), *own[x])[0]
            dev = float(np.max(np.abs(V / (1.0 - fm) ** 2 - 1.0)))
            print("%s %-12s fm %.2f  E %s  vacuum dev %.2e" % (x, name, fm, " ".join("%.4g" % e for e in E), dev))
            assert np.isfinite(E).all() and (E > 0).all() and np.isfinite(V).all() and (V > 0).all()
            if x == "g":
                assert np.max(np.abs(E / E[0] - 1.0)) < 1e-12                       # the same ratio in every bin
            if topo == ref.WATER_MATRIX:
                assert dev <= max(4 * 2.6e-14, 64 * ULP), dev                     # the vacuum limit, E = (1 - fm)**2
            else:
                assert dev <= 4 * ICE_MATRIX_VACUUM[fm]["sg".index(x)], dev       # no identity: see the module docstring
        # towards fm = 1: the water sphere of the melted mass, |K_w|**2/K_i**2 * (rho_i/rho_w)**2; at 0.99 within 5 %
        # for graupel in either topology and for the core as the matrix
        E99 = ref.enhancement(ref.default_cfg(topology=topo), x, par, np.full(shape, 0.99), *own[x])[0]
        sphere = k_w2 / ref.k_ice(ref.default_cfg()) ** 2 * 0.81
        if x == "g" or topo == ref.ICE_MATRIX:
            assert np.max(np.abs(E99 / sphere - 1.0)) < 0.05, (E99, sphere)
    # where nothing melts the ratio is exactly 1.0
    E0 = ref.enhancement(ref.default_cfg(), x, par, np.zeros(shape), *own[x])
    assert (E0 == 1.0).all()


@pytest.mark.parametrize("x", ref.SPECIES)
def test_reference_density_is_the_size_spectras(consts, x):
    """n = N_x(D)*dD of tests/bright_band_ref.py against tests/size_spectra_ref.spectrum on the same parameters: the same
    formulas, up to the rounding of r**3 against r*r*r."""
    par, shape = _parameters(consts, x)
    D, dD = ssr.default_grids()[x]
    if x == "s":
        sp = dict(has_s=np.ones(shape, bool), smob=par["smob"], smoc=par["smoc"])
    else:
        sp = dict(has_g=np.ones(shape, bool), lam_g=par["lam"], n0_g=par["N0"])
    want = ssr.spectrum(sp, x, D, dD)["N"]                                         # [1, nb, nz]
    got = np.stack([ref.density(x, par, D[b], dD[b]) for b in range(len(D))], axis=1)
    assert got.shape == want.shape and (want > 0).any()
    assert np.allclose(got, want, rtol=8 * ULP, atol=0.0)


def test_melting_level_and_fractions_of_the_reference():
    t = np.array([[280.0, 276.0, 274.0, 272.0, 268.0], [280.0, 276.0, 272.0, 270.0, 268.0], [270.0] * 5, [280.0] * 5])
    Lr = np.array([[1, 1, 1, 0, 0], [1, 1, 0, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 0]], dtype=bool)
    Ls = np.array([[1, 1, 1, 1, 1], [0, 0, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0]], dtype=bool)
    Lg = np.zeros_like(Ls)
    k0 = ref.melting_level(t, Lr, Ls, Lg)
    assert k0.tolist() == [3, 2, -1, -1] and k0.dtype == np.int32
    rs = np.array([[1e-4, 2e-4, 5e-4, 4e-4, 1e-4], [1e-12, 1e-12, 3e-4, 3e-4, 3e-4], [1e-4] * 5, [1e-12] * 5])
    fm = ref.melt_fraction(k0, Ls, rs)
    assert fm[0].tolist() == [1.0 - 1e-4 / 4e-4, 1.0 - 2e-4 / 4e-4, 0.05, 0.0, 0.0]      # the 0.05 floor where rs[k] > rs[k0]
    assert (fm[1:] == 0.0).all() and not np.signbit(fm).any()
    assert math.isclose(ref.melt_fraction(np.array([1], dtype=np.int32), np.ones((1, 2), bool), np.array([[1e-9, 1.0]]))[0, 0], 0.99)
