"""The cloud radar (include/kidmp_mie.h, kid_amd/mie.py) without a GPU: the entries exist in the built library and in the
header, kid_amd/mie.py declares them as the header has them, the header compiles as C99 and C++11, a missing context is
refused, every bad configuration is refused, and the Lorenz-Mie sphere of kid_amd/csrc/kidmp_mie_sphere.h is held against
two references of tests/mie_ref.py.

kidmp_mie_sphere against mie_bh, the header restated operation for operation in Python floats: bit-equal, Q_ext and
Q_back, at all forty (m, x) below; kidmp_mie_bins against bins_bh likewise on the scheme's own grids.  (sin, cos, pow, exp
and sqrt are the host libm's on both sides.)

kidmp_mie_sphere against mie_scipy, an independent form (a_n, b_n from scipy.special.jv / yv of half-integer order and
complex argument).  max(|Q_ext/ref - 1|, |Q_back/ref - 1|) measured for the C++ series with scipy 1.15:

    m \\ x        1e-3     0.01     0.1      0.5      1        2        5        10       20       49
    3.0+1.7i     1.6e-15  1.3e-15  1.8e-15  1.7e-15  6.7e-16  1.3e-15  6.2e-15  6.1e-15  4.4e-15  1.2e-14
    8.9+1.4i     4.4e-15  1.8e-15  5.6e-15  1.9e-15  8.9e-16  4.3e-14  4.5e-13  5.9e-15  4.8e-15  1.6e-14
    1.3+0.002i   5.2e-14  5.4e-14  1.3e-14  1.4e-14  1.6e-15  1.1e-14  1.6e-15  2.4e-15  7.8e-14  2.6e-07
    1.78+0.003i  5.9e-14  2.3e-14  9.4e-14  6.1e-15  3.2e-15  1.5e-14  2.1e-15  2.6e-14  1.1e-08  2.5e-06

The assertion is ten times the table, entry by entry.  The large entries at x = 20 and 49 for the weak absorbers are the
Bessel form's own loss (Y_{n+1/2} of a nearly real argument beyond the turning point), not the series': there the series
agrees with its restatement to the bit and the two weak absorbers bracket the same pattern.

Rayleigh limit, D = 5 mm, m = 8.9+1.4i: Q_back/(4 x**4 |K|**2) - 1 = -1.06e-3 at 1 m and -1.06e-5 at 10 m (second order in
x); at 3.2 mm the same drop scatters 3.4e-4 of its Rayleigh value and a 0.5 mm drop 2.2 times it; at 10 cm the 5 mm drop
is 12 % below.
"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mie_ref as ref
import size_spectra_ref as ssr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_mie.h")
CSRC = os.path.join(ROOT, "kid_amd", "csrc")
ENTRIES = ("kidmp_mie_radar_device", "kidmp32_mie_radar_device", "kidmp_mie_radar_host", "kidmp32_mie_radar_host")
SYMBOLS = ENTRIES + ("kidmp_mie_defaults", "kidmp_mie_sphere", "kidmp_mie_bins", "kidmp_mie_table_create", "kidmp_mie_table_destroy",
                     "kidmp_mie_table_get")
SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "size_t": (C.c_size_t,), "double": (C.c_double,),
           "float": (C.c_float,), "int": (C.c_int, C.c_int32), "void": (None,)}
EINVAL, ESTATE = -1, -5

MS = (complex(3.0, 1.7), complex(8.9, 1.4), complex(1.3, 0.002), complex(1.78, 0.003))
XS = (1e-3, 0.01, 0.1, 0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 49.0)
# the table of the module docstring
VS_SCIPY = ((1.6e-15, 1.3e-15, 1.8e-15, 1.7e-15, 6.7e-16, 1.3e-15, 6.2e-15, 6.1e-15, 4.4e-15, 1.2e-14),
            (4.4e-15, 1.8e-15, 5.6e-15, 1.9e-15, 8.9e-16, 4.3e-14, 4.5e-13, 5.9e-15, 4.8e-15, 1.6e-14),
            (5.2e-14, 5.4e-14, 1.3e-14, 1.4e-14, 1.6e-15, 1.1e-14, 1.6e-15, 2.4e-15, 7.8e-14, 2.6e-07),
            (5.9e-14, 2.3e-14, 9.4e-14, 6.1e-15, 3.2e-15, 1.5e-14, 2.1e-15, 2.6e-14, 1.1e-08, 2.5e-06))
# illustrative W-band permittivities (tests/test_gpu_mie_radar.py)
W_BAND = dict(wavelength=3.19e-3, eps_w=complex(7.7, 14.2), eps_i=complex(3.17, 0.01), rho_w=1000.0, rho_i=917.0, kw2=0.75)


def _code():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes():
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of the header."""
    text = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", " ", _code(), flags=re.M)
    text = re.sub(r"typedef struct[^;{]*\{[^}]*\}[^;]*;", " ", text)
    text = re.sub(r"typedef struct \w+ \w+;", " ", text)
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


def _mie_cfg(**kw):
    from kid_amd import MieCfg
    return MieCfg(**kw)


def test_symbols_are_exported_and_prototyped():
    lib = os.path.join(ROOT, "kid_amd", "libkidmp.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(lib)
    assert sorted(_prototypes()) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert '#include "kidmp.h"' in open(HEADER).read()


def test_the_python_declarations_match_the_header():
    import kid_amd
    import kid_amd.mie as km
    declared = km.declare(_Stub()).entries
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
    for struct, elem in (("kidmp_mie_out", "double"), ("kidmp32_mie_out", "float")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _code(), re.S).group(1)
        assert body.split()[0] == elem
        members = [m.strip().lstrip("*") for m in re.sub(r"\b%s\b" % elem, "", body).replace(";", ",").split(",") if m.strip()]
        assert tuple(members) == km.MIE_NAMES == kid_amd.MIE_NAMES
    assert [n for n, _ in km._MieOut._fields_] == list(km.MIE_NAMES) and all(t is C.c_void_p for _, t in km._MieOut._fields_)
    cfg = re.search(r"typedef struct kidmp_mie_cfg \{(.*?)\} kidmp_mie_cfg;", _code(), re.S).group(1)
    names = [m.strip() for m in re.sub(r"\bdouble\b", "", cfg).replace(";", ",").split(",") if m.strip()]
    assert names == [n for n, _ in km._MieCfg._fields_] and all(t is C.c_double for _, t in km._MieCfg._fields_)
    assert names == ["wavelength", "eps_w_re", "eps_w_im", "eps_i_re", "eps_i_im", "rho_w", "rho_i", "kw2"]
    grids = re.search(r"typedef struct kidmp_mie_grids \{(.*?)\} kidmp_mie_grids;", _code(), re.S).group(1)
    assert re.findall(r"(\w+)\[KIDMP_MIE_NSPECIES\]", grids) == [n for n, _ in km._MieGrids._fields_] == ["D", "dD", "nb"]
    raw = open(HEADER).read()
    assert int(re.search(r"#define KIDMP_MIE_MAX_BINS (\d+)", raw).group(1)) == km.MIE_MAX_BINS == 256
    assert int(re.search(r"#define KIDMP_MIE_NSPECIES (\d+)", raw).group(1)) == len(km.MIE_SPECIES) == 3
    assert int(re.search(r"#define KIDMP_MIE_NROWS (\d+)", raw).group(1)) == len(km.MIE_ROWS) == len(ref.ROWS) == 5
    assert km.MIE_ROWS == ref.ROWS and km.MIE_SPECIES == ref.SPECIES


def test_only_the_mie_mirror_declares_them():
    import kid_amd.brightband as bb
    import kid_amd.doppler as dp
    import kid_amd.mie as km
    import kid_amd.thompson as th
    assert sorted(km._declarations()) == sorted(SYMBOLS)
    for other in (th, dp, bb):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_mie.h"\n'
                   "int use(kidmp_ctx *c, const double *a, kidmp_mie_cfg *f, kidmp_mie_grids *g, kidmp_mie_out *o, double *r)\n"
                   "{ kidmp_mie_table *t; int32_t nb; kidmp_mie_defaults(f); f->wavelength = 3.19e-3;\n"
                   "  if (kidmp_mie_sphere(1.0, 1.3, 0.0, r, r + 1) || kidmp_mie_bins(f, KIDMP_MIE_S, 1, a, r)) return 1;\n"
                   "  if (kidmp_mie_table_create(c, f, g, &t) || kidmp_mie_table_get(t, KIDMP_MIE_G, &nb, r, r, r, f)) return 2;\n"
                   "  nb = kidmp_mie_radar_host(c, t, 1, 2, a, a, a, a, a, a, a, a, a, 0, a, a, 0, o);\n"
                   "  kidmp_mie_table_destroy(t); return nb; }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.mie import _MieCfg, _MieGrids, _MieOut, library
    L = library()
    o, g, c = _MieOut(), _MieGrids(), _MieCfg()
    L.kidmp_mie_defaults(C.byref(c))
    args = [None, None, 4, 120] + [None] * 8 + [None, 0, None, None, 0, C.byref(o)]
    assert L.kidmp_mie_radar_host(*args) == ESTATE and L.kidmp32_mie_radar_host(*args) == ESTATE
    assert L.kidmp_mie_radar_device(*args, None) == ESTATE and L.kidmp32_mie_radar_device(*args, None) == ESTATE
    h = C.c_void_p(1)
    assert L.kidmp_mie_table_create(None, C.byref(c), C.byref(g), C.byref(h)) == ESTATE and h.value is None
    assert L.kidmp_mie_table_get(None, 0, None, None, None, None, None) == EINVAL
    L.kidmp_mie_table_destroy(None)


def test_the_defaults():
    from kid_amd.mie import MieCfg, _MieCfg, default_eps_i, library
    import kid_amd.brightband as bb
    c = _MieCfg()
    library().kidmp_mie_defaults(C.byref(c))
    py = MieCfg()
    assert (c.wavelength, c.eps_w_re, c.eps_w_im, c.eps_i_im, c.rho_w, c.rho_i, c.kw2) == (0.10, 79.5, 24.9, 0.0, 1000.0, 900.0, 0.93)
    assert c.eps_i_re == default_eps_i() == bb.default_eps_i() == py.eps_i.real and py.eps_i.imag == 0.0
    assert (py.wavelength, py.eps_w, py.rho_w, py.rho_i, py.kw2) == (0.10, complex(79.5, 24.9), 1000.0, 900.0, 0.93)


def test_every_bad_configuration_is_refused():
    """KIDMP_EINVAL from the library itself (kidmp_mie_bins needs no context), nothing written; the Python mirror refuses
    the same before the library is reached."""
    from kid_amd import KidmpError, mie_bins
    from kid_amd.mie import _MieCfg, library
    L = library()
    D = np.array([1e-3, 2e-3])
    rows = np.full((5, 2), -7.0)
    good = dict(wavelength=3.19e-3, eps_w_re=7.7, eps_w_im=14.2, eps_i_re=3.17, eps_i_im=0.01, rho_w=1000.0, rho_i=917.0, kw2=0.75)
    call = lambda species=0, nb=2, d=D, **kw: L.kidmp_mie_bins(C.byref(_MieCfg(**dict(good, **kw))), species, nb, d.ctypes.data, rows.ctypes.data)   # noqa: E731
    nan, inf = float("nan"), float("inf")
    bad = [dict(wavelength=0.0), dict(wavelength=-1.0), dict(wavelength=nan), dict(wavelength=inf), dict(eps_w_re=nan), dict(eps_w_im=inf),
           dict(eps_w_im=-0.1), dict(eps_i_re=inf), dict(eps_i_im=nan), dict(eps_i_im=-1e-9), dict(eps_i_re=-1.0, eps_i_im=0.0),
           dict(rho_w=0.0), dict(rho_w=nan), dict(rho_i=0.0), dict(rho_i=-917.0), dict(rho_i=inf), dict(kw2=0.0), dict(kw2=-0.9), dict(kw2=nan)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert L.kidmp_last_error(None), kw
    assert call(species=3) == EINVAL and call(species=-1) == EINVAL and call(nb=0) == EINVAL
    assert call(d=np.array([1e-3, 0.0])) == EINVAL and call(d=np.array([nan, 1e-3])) == EINVAL
    assert L.kidmp_mie_bins(None, 0, 2, D.ctypes.data, rows.ctypes.data) == EINVAL
    assert (rows == -7.0).all()
    assert call() == 0 and np.isfinite(rows).all() and (rows > 0).all()
    py = dict(wavelength=3.19e-3, eps_w=complex(7.7, 14.2), eps_i=complex(3.17, 0.01), rho_w=1000.0, rho_i=917.0, kw2=0.75)
    for kw in (dict(wavelength=0.0), dict(wavelength=nan), dict(eps_w=complex(7.7, -1.0)), dict(eps_w="water"), dict(eps_i=complex(inf, 0.0)),
               dict(rho_w=0.0), dict(rho_i=-1.0), dict(kw2=0.0), dict(kw2=nan)):
        with pytest.raises(KidmpError, match="mie_bins"):
            mie_bins(_mie_cfg(**dict(py, **kw)), "r", D)
    with pytest.raises(KidmpError, match="mie_bins"):
        mie_bins(_mie_cfg(**py), "c", D)
    with pytest.raises(KidmpError, match="mie_bins"):
        mie_bins({"wavelength": 1.0}, "r", D)


def test_sphere_refusals():
    from kid_amd import KidmpError, mie_sphere
    from kid_amd.mie import library
    L = library()
    q = (C.c_double * 2)(-7.0, -7.0)
    pd = C.POINTER(C.c_double)
    a, b = C.cast(q, pd), C.cast(C.byref(q, 8), pd)
    nan, inf = float("nan"), float("inf")
    for x, mr, mi in ((0.0, 1.3, 0.0), (-1.0, 1.3, 0.0), (nan, 1.3, 0.0), (inf, 1.3, 0.0), (1.0, 0.0, 0.1), (1.0, nan, 0.0), (1.0, 1.3, -0.1),
                      (1.0, 1.3, inf), (1e9, 1.3, 0.0)):
        assert L.kidmp_mie_sphere(x, mr, mi, a, b) == EINVAL, (x, mr, mi)
    assert L.kidmp_mie_sphere(1.0, 1.3, 0.0, None, b) == EINVAL and tuple(q) == (-7.0, -7.0)
    with pytest.raises(KidmpError):
        mie_sphere(0.0, 1.3)


@pytest.mark.parametrize("im", range(len(MS)), ids=[str(m) for m in MS])
def test_sphere_against_the_restatement_and_the_independent_form(im):
    from kid_amd import mie_sphere
    m = MS[im]
    for ix, x in enumerate(XS):
        qe, qb = mie_sphere(x, m)
        be, bb_ = ref.mie_bh(x, m)
        assert (qe, qb) == (be, bb_), (m, x, qe.hex(), be.hex(), qb.hex(), bb_.hex())
        se, sb = ref.mie_scipy(x, m)
        dev = max(abs(qe / se - 1.0), abs(qb / sb - 1.0))
        print("m = %s x = %g: %.1e (table %.1e)" % (m, x, dev, VS_SCIPY[im][ix]))
        assert dev <= 10.0 * VS_SCIPY[im][ix], (m, x, dev)
        assert qe > 0.0 and qb > 0.0


@pytest.mark.parametrize("x", ref.SPECIES)
def test_bins_against_the_restatement_on_the_default_grids(x):
    """Bit-equal rows on the scheme's own 100 bins at the default 10 cm and at 3.19 mm; s_ext >= 0, mass > 0, v0 > 0."""
    from kid_amd import mie_bins
    D = ssr.default_grids()[x][0]
    for kw in ({}, W_BAND):
        cfg = _mie_cfg(**kw)
        rows = mie_bins(cfg, x, D)
        want = ref.bins_bh(cfg, x, D)
        assert rows.shape == (5, 100) and np.array_equal(rows.view(np.uint64), want.view(np.uint64)), kw
        assert np.isfinite(rows).all() and (rows[0] > 0).all() and (rows[1] > 0).all()
        assert (rows[2] >= 0).all() and (rows[3] > 0).all() and (rows[4] > 0).all()


def test_rayleigh_limit_on_every_rain_bin():
    """Q_back/(4 x**4 |K|**2) - 1 falls with x**2: below 1e-4 at 10 m on every rain bin of the default grid, and the
    deviation at 1 m is 50 to 200 times that at 10 m (100 to second order).  The figures of the module docstring hold."""
    from kid_amd import mie_sphere
    m = complex(8.9, 1.4)
    k2 = ref.absK2(m * m)

    def deviation(D, lam):
        x = math.pi * D / lam
        return mie_sphere(x, m)[1] / (4.0 * x ** 4 * k2) - 1.0
    assert abs(deviation(5e-3, 1.0) / -1.06e-3 - 1.0) < 0.01 and abs(deviation(5e-3, 10.0) / -1.06e-5 - 1.0) < 0.01
    assert abs(deviation(5e-3, 3.2e-3) + 1.0 - 3.4e-4) < 0.1e-4 and abs(deviation(0.5e-3, 3.2e-3) + 1.0 - 2.2) < 0.05
    assert abs(deviation(5e-3, 0.10) + 0.12) < 0.01
    for D in ssr.default_grids()["r"][0]:
        d10, d1 = deviation(D, 10.0), deviation(D, 1.0)
        assert abs(d10) < 1e-4, (D, d10)
        assert 50.0 <= d1 / d10 <= 200.0, (D, d1, d10)


def test_rayleigh_rows_return_the_closed_forms_constants():
    """At 100 m, with the defaults' |K_i|**2 = 0.176, rho_i = 900 and kw2 = 0.93, s_mie/s_ray of snow and graupel is 1 and
    rain's is |K_w|**2/kw2, up to the second-order Mie term: a multiple of x**2 and of |m x|**2 with factors of order one,
    bounded here by 2 |eps| x**2 at the largest bin, eps the permittivity of the substance (an upper bound of the
    mixture's)."""
    from kid_amd import mie_bins
    cfg = _mie_cfg(wavelength=100.0)
    for x, limit, eps in (("s", 1.0, cfg.eps_i), ("g", 1.0, cfg.eps_i), ("r", ref.absK2(complex(79.5, 24.9)) / 0.93, cfg.eps_w)):
        D = ssr.default_grids()[x][0]
        rows = mie_bins(cfg, x, D)
        assert np.max(np.abs(rows[0] / rows[1] / limit - 1.0)) < 2.0 * abs(eps) * (math.pi * D.max() / 100.0) ** 2 + 1e-12, x


# ---- the per-particle model as a host program of its own, with and without ASan + UBSan ----
def test_sphere_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    # the sanitizers' runtimes are linked statically: the program is instrumented by itself and runs in the environment as it is
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else ["-static-libsan"]
    common = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
              os.path.join(ROOT, "tests", "native", "mie_sphere_check.cpp")]
    san, plain = tmp_path / "mie_san", tmp_path / "mie_plain"
    subprocess.run(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + static
                   + ["-o", str(san)], check=True)
    subprocess.run(common + ["-o", str(plain)], check=True)
    a = subprocess.run([str(san)], capture_output=True, text=True)
    b = subprocess.run([str(plain)], capture_output=True, text=True)
    assert a.returncode == 0 and a.stdout.strip().endswith("mie ok") and "runtime error" not in a.stderr and "Sanitizer" not in a.stderr, \
        a.stdout[-2000:] + a.stderr
    assert b.returncode == 0 and a.stdout == b.stdout and len(a.stdout.splitlines()) == 40 + 2 * 3 * 24 + 1
    # the program's numbers are the library's and the restatement's
    from kid_amd import mie_sphere
    for ln in (ln.split() for ln in b.stdout.splitlines()):
        if ln[0] == "q":
            x, mr, mi, qe, qb = (float.fromhex(v) for v in ln[1:])
            assert mie_sphere(x, complex(mr, mi)) == (qe, qb) == ref.mie_bh(x, complex(mr, mi))


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


def _fake_table(model):
    from kid_amd import MieTable
    t = MieTable.__new__(MieTable)
    t._t, t.model = C.c_void_p(1), model
    return t


def test_wrappers_reject_bad_arguments_before_the_library(monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import MIE_INPUTS, MieTable
    N, NZ = 4, 30
    good = lambda: {k: np.zeros((N, NZ)) for k in MIE_INPUTS}   # noqa: E731
    m = _bare()
    t = _fake_table(m)
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    monkeypatch.setattr(MieTable, "close", lambda self: None)
    dz = np.ones(NZ)
    cases = [
        ([np.zeros((N, NZ))], {}), ({k: v.astype(np.float16) for k, v in good().items()}, {}), ({k: np.zeros(NZ) for k in MIE_INPUTS}, {}),
        ({k: np.zeros((N, 1)) for k in MIE_INPUTS}, {}), ({k: np.zeros((N, 257)) for k in MIE_INPUTS}, {}),
        ({k: v for k, v in good().items() if k != "qr"}, {}), (dict(good(), qs=np.zeros((N, NZ), dtype=np.float32)), {}),
        (dict(good(), p=np.zeros((NZ, N)).T), {}), (good(), dict(want=("dbz", "sw"))), (good(), dict(want=("vd", "vd"))), (good(), dict(want=())),
        (good(), dict(want=3)), (good(), dict(want=("pia_up",))), (good(), dict(want=("pia_total",))), (good(), dict(dz=np.ones(NZ + 1), want=("pia_up",))),
        (good(), dict(dz=[1.0] * NZ)), (good(), dict(dz=dz.astype(np.float32))), (good(), dict(k_gas=np.ones((NZ, N)))), (good(), dict(w=np.ones(NZ))),
        (good(), dict(out=[np.zeros((N, NZ))])), (good(), dict(out={"dbz": np.zeros((NZ, N))})),
        (good(), dict(want=("pia_total",), dz=dz, out={"pia_total": np.zeros((N, NZ))})),
    ]
    for st, kw in cases:
        with pytest.raises(th.KidmpError, match="mie_radar_host"):
            m.mie_radar_host(t, st, **kw)
    for bad_table in (None, "table", _fake_table(_bare())):
        with pytest.raises(th.KidmpError, match="mie_radar_host"):
            m.mie_radar_host(bad_table, good())
    import torch
    with pytest.raises(th.KidmpError, match="mie_radar"):
        m.mie_radar(t, {k: torch.zeros(N, NZ, dtype=torch.float64) for k in MIE_INPUTS})   # host memory
    with pytest.raises(th.KidmpError, match="mie_radar"):
        m.mie_radar(t, good())
    for grids in ([1], {"c": (dz, dz)}, {"r": (dz, None)}, {"r": (np.ones(0), np.ones(0))}, {"s": (np.ones(257), np.ones(257))},
                  {"g": (dz, np.ones(NZ + 1))}, {"g": (dz.astype(np.float32), dz.astype(np.float32))}):
        with pytest.raises(th.KidmpError, match="MieTable"):
            m.mie_table(None, grids)
    with pytest.raises(th.KidmpError, match="MieTable"):
        m.mie_table({"wavelength": 0.1})
