"""The spectrum processor (include/kidmp_specproc.h, kid_amd/specproc.py) without a GPU: the entries exist in the built
library and in the header, kid_amd/specproc.py declares them as the header has them, the header compiles as C99 and C++11,
a missing context is refused, the wrapper refuses wrong input before the library is reached, and the window arithmetic of
kid_amd/csrc/kidmp_specproc_window.h -- the half-width, the weights, their norm, the tails and the detection rule, the
very functions the kernel calls -- runs as a host program of its own, with and without ASan + UBSan, against
tests/specproc_ref.py on the covering cases of tests/specproc_cases.py: H, s and the detection mask to the bit, what holds an
exponential to the bound stated at the test.  Nothing is loaded into Python under a sanitizer.
"""
import ctypes as C
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import specproc_cases as cases
import specproc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_specproc.h")
CSRC = os.path.join(ROOT, "kid_amd", "csrc")
SYMBOLS = ("kidmp_spectrum_process_device", "kidmp32_spectrum_process_device")
SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "double": (C.c_double,), "float": (C.c_float,), "int": (C.c_int, C.c_int32),
           "void": (None,)}
EINVAL, ESTATE = -1, -5
ULP = 2.220446049250313e-16


def _sp():
    return importlib.import_module("kid_amd.specproc")


def _code():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes():
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of the header."""
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
    assert sorted(_prototypes()) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    raw = open(HEADER).read()
    assert '#include "kidmp.h"' in raw
    assert "project's own" in raw.lower() and "unpinned" in raw
    raw = " ".join(raw.replace("\n *", " ").split())                 # the comment as running text
    assert "no host-array entries and no Fortran binding" in raw
    for word in ("random noise realisations", "spectral averaging", "peaks", "aliasing or folding", "non-uniform velocity grids"):
        assert word in raw, word


def test_the_python_declarations_match_the_header():
    import kid_amd
    sp = _sp()
    declared = sp.declare(_Stub()).entries
    protos = _prototypes()
    assert sorted(declared) == sorted(protos) == sorted(sp._declarations())
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
    for struct, elem in (("kidmp_specproc_out", "double"), ("kidmp32_specproc_out", "float")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _code(), re.S).group(1)
        assert body.split()[0] == elem
        members = [m.strip().lstrip("*") for m in re.sub(r"\b(%s|int32_t)\b" % elem, "", body).replace(";", ",").split(",") if m.strip()]
        assert tuple(members) == sp.SPECPROC_NAMES == kid_amd.SPECPROC_NAMES == ref.NAMES
        assert re.search(r"int32_t \*nbins;", body)
    assert [n for n, _ in sp._SpecOut._fields_] == list(sp.SPECPROC_NAMES) and all(t is C.c_void_p for _, t in sp._SpecOut._fields_)
    cfg = re.search(r"typedef struct kidmp_specproc_cfg \{(.*?)\} kidmp_specproc_cfg;", _code(), re.S).group(1)
    fields = []
    for decl in cfg.split(";"):
        if decl.strip():
            t, names = decl.split(None, 1)
            fields += [(n.strip(), {"double": C.c_double, "int32_t": C.c_int32}[t]) for n in names.split(",")]
    assert fields == list(sp._SpecCfg._fields_)
    assert [n for n, _ in fields] == ["cut", "snr_min", "add_noise"]
    raw = open(HEADER).read()
    assert int(re.search(r"#define KIDMP_SPECPROC_MAX_NV (\d+)", raw).group(1)) == sp.SPECPROC_MAX_NV == 256
    assert int(re.search(r"#define KIDMP_SPECPROC_MAX_HALF (\d+)", raw).group(1)) == sp.SPECPROC_MAX_HALF == ref.MAX_HALF == cases.CAP == 256
    window = open(os.path.join(CSRC, "kidmp_specproc_window.h")).read()
    assert re.search(r"constexpr int MAX_HALF = 256;", window) and re.search(r"constexpr double EXP_MAX = 700\.;", window) and ref.EXP_MAX == 700.0
    kernel = open(os.path.join(CSRC, "kidmp_specproc.hip")).read()
    assert re.search(r"constexpr int SP_TJ = %d;" % cases.TILE, kernel) and re.search(r"constexpr int SP_WCAP = %d;" % cases.KEPT, kernel)
    d = sp.SpecCfg()
    assert (d.cut, d.snr_min, d.add_noise) == (4.0, 1.0, False)
    assert kid_amd.spectrum_process is sp.spectrum_process and kid_amd.SpecCfg is sp.SpecCfg
    assert callable(kid_amd.ThompsonMP.spectrum_process)


def test_only_the_specproc_mirror_declares_them():
    import kid_amd.dspectrum as ds
    import kid_amd.thompson as th
    sc = importlib.import_module("kid_amd.scan")            # kid_amd.scan, the attribute, is the function
    for other in (th, ds, sc):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_specproc.h"\n'
                   "int use(kidmp_ctx *c, const double *a, const float *b, kidmp_specproc_cfg *f, kidmp_specproc_out *o, kidmp32_specproc_out *p)\n"
                   "{ f->cut = 4.0; f->snr_min = 1.0; f->add_noise = 0; o->nbins = p->nbins; o->spec = 0; p->sw = 0;\n"
                   "  if (kidmp_spectrum_process_device(c, 3, 16, a, -1.0, 0.1, KIDMP_SPECPROC_MAX_NV, a, 0, a, 16, f, o, 0)) return 1;\n"
                   "  return kidmp32_spectrum_process_device(c, 3, 16, b, -1.0, 0.1, KIDMP_SPECPROC_MAX_HALF, b, 16, b, 0, f, p, 0); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    sp = _sp()
    L = sp.library()
    o, c = sp._SpecOut(), sp._SpecCfg(4.0, 1.0, 0)
    args = [None, 3, 16, None, -1.0, 0.1, 64, None, 0, None, 0, C.byref(c), C.byref(o), None]
    assert L.kidmp_spectrum_process_device(*args) == ESTATE and L.kidmp32_spectrum_process_device(*args) == ESTATE
    assert L.kidmp_last_error(None)


def _write_cases(path, cs):
    h = lambda v: float(v).hex()   # noqa: E731
    with open(path, "w") as f:
        f.write("%d\n" % len(cs))
        for inv_dv, cut, snr_min, sigmas, pairs in cs:
            f.write("%s %s %s %d %d\n" % (h(inv_dv), h(cut), h(snr_min), len(sigmas), len(pairs)))
            f.write(" ".join(h(s) for s in sigmas) + "\n")
            f.write(" ".join("%s %s" % (h(b), h(n)) for b, n in pairs) + "\n")


def _num(tok):
    return float.fromhex(tok) if "n" not in tok else float(tok)     # nan, -nan, inf


def test_window_under_sanitizers_equals_the_reference(tmp_path):
    """H, s and the detection mask hold no exponential and equal the restatement's to the bit.  A weight is fastmath.h's
    exponential (within 2 ulp of the true value, kid_amd/csrc/fastmath.h) against numpy's (within 1 ulp) of the same
    argument: at most 4 ulp apart.  G and T_m are sums of at most 2 H + 1 such non-negative weights added in the same order
    on both sides, so each sum inherits the 4 ulp of its terms and one more half ulp per addition can differ: (4 + H) ulp."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    # the sanitizers' runtimes are linked statically: the program is instrumented by itself and runs in the environment as it is
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else ["-static-libsan"]
    common = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
              os.path.join(ROOT, "tests", "native", "specproc_window_check.cpp")]
    san, plain = tmp_path / "specproc_san", tmp_path / "specproc_plain"
    subprocess.run(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + static
                   + ["-o", str(san)], check=True)
    subprocess.run(common + ["-o", str(plain)], check=True)
    cs = cases.window_cases()
    _write_cases(tmp_path / "cases.txt", cs)
    a = subprocess.run([str(san), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    b = subprocess.run([str(plain), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert a.returncode == 0 and a.stdout.strip().endswith("specproc ok") and "runtime error" not in a.stderr and "Sanitizer" not in a.stderr, \
        a.stdout[-2000:] + a.stderr
    assert b.returncode == 0 and a.stdout == b.stdout
    lines = iter(b.stdout.splitlines())
    halves, worst, zeros = set(), 0.0, 0
    for n, (inv_dv, cut, snr_min, sigmas, pairs) in enumerate(cs):
        assert next(lines) == "c %d" % n
        sig = np.array(sigmas, dtype=np.float64)
        s, H = ref.window(sig, inv_dv, cut)
        g, G = ref.weights(s, H)
        T = ref.tails(g, H)
        for m in range(len(sigmas)):
            tag, gH, gs, gG = next(lines).split()
            assert tag == "w" and int(gH) == H[m], (n, m, sigmas[m], gH, H[m])
            assert ref.bits(np.float64(_num(gs)))[()] == ref.bits(s[m])[()], (n, m, "s")
            halves.add(int(gH))
            bound = (4.0 + H[m]) * ULP
            assert abs(_num(gG) - G[m]) <= bound * G[m], (n, m, "G", gG, G[m])
            if H[m] == 0:
                assert _num(gG) == 1.0 == G[m]
            for d in range(1, H[m] + 1):
                tag, gd, gv = next(lines).split()
                assert tag == "g" and int(gd) == d
                gv = _num(gv)
                if g[d, m] == 0.0:
                    assert gv == 0.0 and np.signbit(gv) == np.signbit(g[d, m])
                    zeros += 1
                else:
                    worst = max(worst, abs(gv - g[d, m]) / g[d, m] / ULP)
                    assert abs(gv - g[d, m]) <= 4.0 * ULP * g[d, m], (n, m, d, gv, g[d, m])
            for t in range(H[m], 0, -1):
                tag, gt, gv = next(lines).split()
                assert tag == "t" and int(gt) == t
                assert abs(_num(gv) - T[t, m]) <= bound * T[t, m], (n, m, "T", t, gv, T[t, m])
        with np.errstate(invalid="ignore"):
            det = np.array([b_ for b_, _ in pairs]) > snr_min * np.array([n_ for _, n_ in pairs])
        for p in range(len(pairs)):
            assert next(lines) == "d %d" % det[p], (n, p, pairs[p])
    assert next(lines) == "specproc ok"
    print("weights: at most %.2f ulp from numpy's exponential; %d exact zeros" % (worst, zeros))
    assert {0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256} <= halves and zeros > 0
    # by hand: with cut = 4 and dv = 1/8 the ratios of the cases give these half-widths, and what is no width gives none
    for h, r in cases.RATIOS.items():
        assert ref.window(np.array([r * cases.DV]), 1.0 / cases.DV, cases.CUT)[1][0] == (256 if h == "cap" else h) == cases.expected_half(r)
    nothing = np.array([0.0, -0.0, -1.0, float("nan"), float("-inf")])
    assert (ref.window(nothing, 8.0, 4.0)[1] == 0).all() and ref.window(np.array([float("inf")]), 8.0, 4.0)[1][0] == 256


def test_the_restatement_on_cases_by_hand():
    """sigma/dv = 0.25 with cut = 4: H = 1, g_1 = exp(-8), G = 1 + 2 g_1.  A unit bin in the middle comes back as
    (g_1, 1, g_1)/G, one at bin 0 loses g_1/G below the grid, and the moments of a single detected bin are its centre."""
    g1 = np.exp(-8.0)
    x = np.zeros((1, 5, 2))
    x[0, 2, 0] = 1.0
    x[0, 0, 1] = 1.0
    r = ref.process(x, -1.0, 0.5, sigma=np.array([0.125, 0.125]), parts=True)
    assert (r["H"] == 1).all() and r["G"][0, 0] == 1.0 + (g1 + g1)
    G = r["G"][0, 0]
    assert np.array_equal(r["spec"][0, :, 0], np.array([0.0, g1 / G, 1.0 / G, g1 / G, 0.0]))
    assert np.array_equal(r["spec"][0, :, 1], np.array([1.0 / G, g1 / G, 0.0, 0.0, 0.0]))
    assert r["lost_below"][0, 1] == g1 / G and r["lost_below"][0, 0] == 0.0 and (r["lost_above"] == 0.0).all()
    assert list(r["nbins"][0]) == [3, 2] and r["v_lo"][0, 0] == -0.5 and r["v_hi"][0, 0] == 0.5 and abs(r["vm"][0, 0]) < 1e-16
    none = ref.process(x, -1.0, 0.5)
    assert np.array_equal(ref.bits(none["spec"]), ref.bits(x)) and (none["lost_below"] == 0).all() and list(none["nbins"][0]) == [1, 1]
    assert none["vm"][0, 0] == 0.0 and none["vm"][0, 1] == -1.0 and (none["sw"] == 0).all() and (none["skew"] == 0).all() and (none["kurt"] == 0).all()
    assert none["dbz"][0, 0] == 10.0 * np.log10(1e18)
    empty = ref.process(np.zeros((1, 5, 2)), -1.0, 0.5, sigma=np.array([0.3, 0.0]))
    assert (empty["dbz"] == -40.0).all() and (empty["nbins"] == 0).all() and all((empty[n] == 0).all() for n in ("vm", "sw", "skew", "kurt", "v_lo", "v_hi"))
    # conservation and the kernel's own variance
    xs = cases.spectrum(2, 25, 3, seed=1)
    r = ref.process(xs, cases.V0, cases.DV, sigma=cases.DV * np.array([2.0, 0.25, 8.0]), parts=True)
    total = r["B"].sum(axis=1) + r["lost_below"] + r["lost_above"]
    assert np.abs(total - xs.sum(axis=1)).max() <= 64 * ULP * xs.sum(axis=1).max()
    assert np.allclose(ref.kernel_variance(r["g"], r["G"], r["H"])[0], [4.0, 2.0 * g1 / (1.0 + 2.0 * g1), 64.0], rtol=2e-3)


# ---- the wrapper refuses wrong input before the library is reached ----
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called")


def test_wrapper_rejects_bad_arguments_before_the_library(monkeypatch):
    import torch
    import kid_amd.thompson as th
    from kid_amd import SpecCfg, ThompsonMP
    m = ThompsonMP.__new__(ThompsonMP)                      # no kidmp_init: there is no device here
    m._h, m.device, m.iiwarm = None, 0, False
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    spec = torch.zeros(3, 25, 12, dtype=torch.float64)      # host memory: refused at the first tensor at the latest
    nan, inf = float("nan"), float("inf")
    calls = [dict(spec=np.zeros((3, 25, 12))), dict(spec=torch.zeros(3, 12, dtype=torch.float64)), dict(spec=torch.zeros(3, 25, 1, dtype=torch.float64)),
             dict(spec=torch.zeros(3, 257, 12, dtype=torch.float64)), dict(spec=torch.zeros(3, 0, 12, dtype=torch.float64)),
             dict(spec=torch.zeros(3, 25, 12, dtype=torch.int32)), dict(dv=0.0), dict(dv=-0.1), dict(dv=nan), dict(dv=inf), dict(dv="fine"),
             dict(v0=nan), dict(v0=inf), dict(cfg=4.0), dict(cfg=SpecCfg(cut=0.0)), dict(cfg=SpecCfg(cut=-1.0)), dict(cfg=SpecCfg(cut=nan)),
             dict(cfg=SpecCfg(cut=inf)), dict(cfg=SpecCfg(snr_min=-0.5)), dict(cfg=SpecCfg(snr_min=nan)), dict(cfg=SpecCfg(snr_min=inf)),
             dict(cfg=SpecCfg(cut="wide")), dict(want=()), dict(want=("vm", "vm")), dict(want=("zdr",)), dict(want=3), dict(out=[]), dict()]
    for kw in calls:
        args = dict(spec=spec, v0=-1.0, dv=0.1, cfg=SpecCfg(), want=("vm",))
        args.update(kw)
        with pytest.raises(th.KidmpError, match="spectrum_process"):
            m.spectrum_process(**args)
