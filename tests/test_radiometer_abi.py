"""The radiometer (include/kidmp_radiometer.h, kid_amd/radiometer.py) without a GPU: the entries exist in the built library
and in the new header only, kid_amd/radiometer.py declares them as the header has them, the header compiles as C99 and
C++11, a missing context is refused, every bad configuration is refused, and the sphere's Q_sca and g
(kid_amd/csrc/kidmp_mie_sphere.h), the layer and the adding (kid_amd/csrc/kidmp_radiometer_layer.h) are held against
tests/radiometer_ref.py.

kidmp_radiometer_sphere against sphere_bh, the header restated operation for operation in Python floats: bit-equal at all
forty (m, x) of tests/test_mie_abi.py, with Q_ext and Q_back the bits of kidmp_mie_sphere; kidmp_radiometer_bins against
bins_bh likewise on the scheme's own grids.

kidmp_radiometer_sphere against sphere_scipy, the independent Bessel form of tests/mie_ref.py extended to Q_sca and g.
max(|Q_sca/ref - 1|, |g/ref - 1|) measured for the C++ series with scipy 1.15:

    m \\ x        1e-3     0.01     0.1      0.5      1        2        5        10       20       49
    3.0+1.7i     3.9e-04  5.0e-10  3.3e-12  7.8e-15  8.9e-16  5.6e-16  3.2e-15  3.1e-15  6.9e-15  2.2e-16
    8.9+1.4i     4.4e-05  5.5e-11  3.4e-13  1.1e-15  1.0e-15  6.7e-15  9.5e-15  2.7e-15  5.7e-15  5.6e-16
    1.3+0.002i   3.4e-03  4.3e-09  2.7e-11  7.4e-14  9.3e-15  5.4e-15  8.9e-16  1.3e-15  3.7e-15  8.3e-09
    1.78+0.003i  1.2e-03  1.6e-09  9.4e-12  1.4e-14  2.7e-15  5.1e-15  2.7e-15  4.4e-15  1.9e-09  7.8e-07

The assertion is ten times the table, entry by entry.  The large entries at x = 20 and 49 for the weak absorbers are the
Bessel form's own loss, as in tests/test_mie_abi.py.  Those at x <= 0.1 are the series' and are g's alone (Q_sca alone
measures 6e-10 at 1e-3 and below 1e-13 from 0.01 on): there g = O(x**2) rests on a_2 and b_1, of order x**5, whose
psi_2 = (3/x) psi_1 - psi_0 the upward recurrence forms by cancellation, losing a factor of order x**-4 of the rounding
(a 60-digit evaluation puts the Bessel form within 2e-8 of the truth at 1e-3 and the series 4e-4 to 3e-3 off).  g is then
below 1e-6 itself, and s_bsc = (Q_sca - g Q_sca)/2 moves by less than 1e-9 of its value; the scheme's smallest bin sits at
x = 1.6e-3 at 10 cm.

Algebra on the restatement alone: a = 1 - R - T within 4 ulp of 1; adding the identity returns the operand to the bit; the
scans in the kernel's order and sequential() -- the same layers added one by one -- differ on the case columns by at most
29 ulp of a brightness temperature (measured here; 17 on the absorbing table), and the test holds them to four times that.
"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mie_ref
import radiometer_cases as rc
import radiometer_ref as ref
import size_spectra_ref as ssr
import test_mie_abi as tma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_radiometer.h")
CSRC = os.path.join(ROOT, "kid_amd", "csrc")
ENTRIES = ("kidmp_radiometer_device", "kidmp32_radiometer_device", "kidmp_radiometer_host", "kidmp32_radiometer_host")
SYMBOLS = ENTRIES + ("kidmp_radiometer_defaults", "kidmp_radiometer_sphere", "kidmp_radiometer_bins", "kidmp_radiometer_table_create",
                     "kidmp_radiometer_table_destroy", "kidmp_radiometer_table_get")
SCALARS = tma.SCALARS
EINVAL, ESTATE = -1, -5
MS, XS, W_BAND = tma.MS, tma.XS, tma.W_BAND
# the table of the module docstring
VS_SCIPY = ((3.9e-04, 5.0e-10, 3.3e-12, 7.8e-15, 8.9e-16, 5.6e-16, 3.2e-15, 3.1e-15, 6.9e-15, 2.2e-16),
            (4.4e-05, 5.5e-11, 3.4e-13, 1.1e-15, 1.0e-15, 6.7e-15, 9.5e-15, 2.7e-15, 5.7e-15, 5.6e-16),
            (3.4e-03, 4.3e-09, 2.7e-11, 7.4e-14, 9.3e-15, 5.4e-15, 8.9e-16, 1.3e-15, 3.7e-15, 8.3e-09),
            (1.2e-03, 1.6e-09, 9.4e-12, 1.4e-14, 2.7e-15, 5.1e-15, 2.7e-15, 4.4e-15, 1.9e-09, 7.8e-07))
SCAN_VS_SEQUENTIAL = 29.0                                   # ulp, the largest difference measured on the case columns
ULP = 2.220446049250313e-16


def _code():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes(path=HEADER):
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of a header."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", " ", text, flags=re.M)
    text = re.sub(r"typedef struct[^;{]*\{[^}]*\}[^;]*;", " ", text)
    text = re.sub(r"typedef struct \w+ \w+;", " ", text)
    out = {}
    for ret, name, params in re.findall(r"([\w \t\n\*]+?)\b(kidmp(?:32)?_\w+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        out[name] = (" ".join(ret.split()), [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    return out


def _mie_cfg(**kw):
    from kid_amd import MieCfg
    return MieCfg(**kw)


# ---- ABI ----
def test_symbols_are_exported_and_prototyped_in_the_new_header_only():
    lib = os.path.join(ROOT, "kid_amd", "libkidmp.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(lib)
    assert sorted(_prototypes()) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert '#include "kidmp_mie.h"' in open(HEADER).read()
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):
        if other.endswith(".h") and other != "kidmp_radiometer.h":
            assert not set(SYMBOLS) & set(_prototypes(os.path.join(inc, other))), other
    assert len(_prototypes(os.path.join(inc, "kidmp.h"))) == 67 and len(_prototypes(os.path.join(inc, "kidmp_mie.h"))) == 10


def test_the_python_declarations_match_the_header():
    import kid_amd
    import kid_amd.radiometer as kr
    declared = kr.declare(tma._Stub()).entries
    protos = _prototypes()
    assert sorted(declared) == sorted(protos)
    wrong = []
    for name, (ret, params) in sorted(protos.items()):
        e = declared[name]
        if len(e.argtypes) != len(params):
            wrong.append("%s: %d arguments declared, the header has %d" % (name, len(e.argtypes), len(params)))
            continue
        for i, (p, t) in enumerate(zip(params, e.argtypes)):
            ok = tma._is_pointer(t) if "*" in p else t in SCALARS[re.sub(r"\bconst\b", "", p).split()[0]]
            if not ok:
                wrong.append("%s: argument %d is `%s`, declared %s" % (name, i, p, getattr(t, "__name__", t)))
        if e.restype not in SCALARS[ret]:
            wrong.append("%s: returns `%s`, declared %s" % (name, ret, getattr(e.restype, "__name__", e.restype)))
    assert not wrong, "\n".join(wrong)
    for struct, elem in (("kidmp_radiometer_out", "double"), ("kidmp32_radiometer_out", "float")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _code(), re.S).group(1)
        assert body.split()[0] == elem
        members = [m.strip().lstrip("*") for m in re.sub(r"\b%s\b" % elem, "", body).replace(";", ",").split(",") if m.strip()]
        assert tuple(members) == kr.RADIOMETER_NAMES == kid_amd.RADIOMETER_NAMES == ref.NAMES
    assert [n for n, _ in kr._RadiometerOut._fields_] == list(kr.RADIOMETER_NAMES) and all(t is C.c_void_p for _, t in kr._RadiometerOut._fields_)
    cfg = re.search(r"typedef struct kidmp_radiometer_cfg \{(.*?)\} kidmp_radiometer_cfg;", _code(), re.S).group(1)
    names = [m.strip() for m in re.sub(r"\bdouble\b", "", cfg).replace(";", ",").split(",") if m.strip()]
    assert names == [n for n, _ in kr._RadiometerCfg._fields_] == ["mu", "emissivity", "t_cosmic"]
    assert all(t is C.c_double for _, t in kr._RadiometerCfg._fields_)
    raw = open(HEADER).read()
    assert int(re.search(r"#define KIDMP_RADIOMETER_NROWS (\d+)", raw).group(1)) == len(kr.RADIOMETER_ROWS) == len(ref.ROWS) == 3
    assert kr.RADIOMETER_ROWS == ref.ROWS and kr.RADIOMETER_SUMMARY_NAMES == ref.SUMMARY == kr.RADIOMETER_NAMES[6:]
    assert kr.RADIOMETER_INPUTS == ref.INPUTS


def test_only_the_radiometer_mirror_declares_them():
    import kid_amd.mie as km
    import kid_amd.radiometer as kr
    import kid_amd.thompson as th
    assert sorted(kr._declarations()) == sorted(SYMBOLS)
    for other in (th, km):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_radiometer.h"\n'
                   "int use(kidmp_ctx *c, const double *a, kidmp_mie_cfg *f, kidmp_mie_grids *g, kidmp_radiometer_cfg *q, kidmp_radiometer_out *o, double *r)\n"
                   "{ kidmp_radiometer_table *t; int32_t nb; kidmp_mie_defaults(f); kidmp_radiometer_defaults(q); q->mu = 0.6;\n"
                   "  if (kidmp_radiometer_sphere(1.0, 1.3, 0.0, r, r + 1, r + 2, r + 3) || kidmp_radiometer_bins(f, KIDMP_MIE_S, 1, a, r)) return 1;\n"
                   "  if (kidmp_radiometer_table_create(c, f, g, &t) || kidmp_radiometer_table_get(t, KIDMP_MIE_G, &nb, r, r, r, f)) return 2;\n"
                   "  nb = kidmp_radiometer_host(c, t, q, 1, 2, a, a, a, a, a, a, a, a, a, 0, a, 0, a, o);\n"
                   "  kidmp_radiometer_table_destroy(t); return nb + KIDMP_RADIOMETER_NROWS; }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.mie import _MieCfg, _MieGrids
    from kid_amd.radiometer import _RadiometerCfg, _RadiometerOut, library
    L = library()
    o, g, c, r = _RadiometerOut(), _MieGrids(), _MieCfg(), _RadiometerCfg()
    L.kidmp_mie_defaults.argtypes, L.kidmp_mie_defaults.restype = [C.POINTER(_MieCfg)], None
    L.kidmp_mie_defaults(C.byref(c))
    L.kidmp_radiometer_defaults(C.byref(r))
    args = [None, None, C.byref(r), 4, 120] + [None] * 8 + [None, 0, None, 0, None, C.byref(o)]
    assert L.kidmp_radiometer_host(*args) == ESTATE and L.kidmp32_radiometer_host(*args) == ESTATE
    assert L.kidmp_radiometer_device(*args, None) == ESTATE and L.kidmp32_radiometer_device(*args, None) == ESTATE
    h = C.c_void_p(1)
    assert L.kidmp_radiometer_table_create(None, C.byref(c), C.byref(g), C.byref(h)) == ESTATE and h.value is None
    assert L.kidmp_radiometer_table_get(None, 0, None, None, None, None, None) == EINVAL
    L.kidmp_radiometer_table_destroy(None)
    L.kidmp_radiometer_defaults(None)


def test_the_defaults():
    from kid_amd import RadiometerCfg
    from kid_amd.radiometer import _RadiometerCfg, library
    r = _RadiometerCfg(-1.0, -1.0, -1.0)
    library().kidmp_radiometer_defaults(C.byref(r))
    py = RadiometerCfg()
    assert (r.mu, r.emissivity, r.t_cosmic) == (1.0, 1.0, 2.725) == (py.mu, py.emissivity, py.t_cosmic)


def test_every_bad_configuration_is_refused():
    """KIDMP_EINVAL from the library itself (kidmp_radiometer_bins needs no context), nothing written; the Python mirror
    refuses the same before the library is reached."""
    from kid_amd import KidmpError, radiometer_bins
    from kid_amd.mie import _MieCfg
    from kid_amd.radiometer import library
    L = library()
    D = np.array([1e-3, 2e-3])
    rows = np.full((3, 2), -7.0)
    good = dict(wavelength=3.19e-3, eps_w_re=7.7, eps_w_im=14.2, eps_i_re=3.17, eps_i_im=0.01, rho_w=1000.0, rho_i=917.0, kw2=0.75)
    call = lambda species=0, nb=2, d=D, **kw: L.kidmp_radiometer_bins(C.byref(_MieCfg(**dict(good, **kw))), species, nb, d.ctypes.data, rows.ctypes.data)   # noqa: E731
    nan, inf = float("nan"), float("inf")
    bad = [dict(wavelength=0.0), dict(wavelength=-1.0), dict(wavelength=nan), dict(wavelength=inf), dict(eps_w_re=nan), dict(eps_w_im=inf),
           dict(eps_w_im=-0.1), dict(eps_i_re=inf), dict(eps_i_im=nan), dict(eps_i_im=-1e-9), dict(eps_i_re=-1.0, eps_i_im=0.0),
           dict(rho_w=0.0), dict(rho_w=nan), dict(rho_i=0.0), dict(rho_i=-917.0), dict(rho_i=inf), dict(kw2=0.0), dict(kw2=nan)]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert L.kidmp_last_error(None), kw
    assert call(species=3) == EINVAL and call(species=-1) == EINVAL and call(nb=0) == EINVAL
    assert call(d=np.array([1e-3, 0.0])) == EINVAL and call(d=np.array([nan, 1e-3])) == EINVAL
    assert L.kidmp_radiometer_bins(None, 0, 2, D.ctypes.data, rows.ctypes.data) == EINVAL
    assert (rows == -7.0).all()
    assert call() == 0 and np.isfinite(rows).all() and (rows > 0).all()
    py = dict(wavelength=3.19e-3, eps_w=complex(7.7, 14.2), eps_i=complex(3.17, 0.01), rho_w=1000.0, rho_i=917.0, kw2=0.75)
    for kw in (dict(wavelength=0.0), dict(wavelength=nan), dict(eps_w=complex(7.7, -1.0)), dict(eps_w="water"), dict(eps_i=complex(inf, 0.0)),
               dict(rho_w=0.0), dict(rho_i=-1.0)):
        with pytest.raises(KidmpError, match="radiometer_bins"):
            radiometer_bins(_mie_cfg(**dict(py, **kw)), "r", D)
    with pytest.raises(KidmpError, match="radiometer_bins"):
        radiometer_bins(_mie_cfg(**py), "c", D)
    q = (C.c_double * 4)(-7.0, -7.0, -7.0, -7.0)
    pd = C.POINTER(C.c_double)
    p = [C.cast(C.byref(q, 8 * i), pd) for i in range(4)]
    for x, mr, mi in ((0.0, 1.3, 0.0), (-1.0, 1.3, 0.0), (nan, 1.3, 0.0), (inf, 1.3, 0.0), (1.0, 0.0, 0.1), (1.0, nan, 0.0), (1.0, 1.3, -0.1),
                      (1.0, 1.3, inf), (1e9, 1.3, 0.0)):
        assert L.kidmp_radiometer_sphere(x, mr, mi, *p) == EINVAL, (x, mr, mi)
    assert L.kidmp_radiometer_sphere(1.0, 1.3, 0.0, p[0], p[1], None, p[3]) == EINVAL and tuple(q) == (-7.0,) * 4


# ---- the sphere ----
@pytest.mark.parametrize("im", range(len(MS)), ids=[str(m) for m in MS])
def test_sphere_against_the_restatement_and_the_independent_form(im):
    from kid_amd import mie_sphere, radiometer_sphere
    m = MS[im]
    for ix, x in enumerate(XS):
        got = radiometer_sphere(x, m)
        want = ref.sphere_bh(x, m)[:4]
        assert got == want, (m, x, [v.hex() for v in got], [v.hex() for v in want])
        assert (got[0], got[2]) == mie_sphere(x, m) == mie_ref.mie_bh(x, m)
        _, ss, _, sg = ref.sphere_scipy(x, m)
        dev = max(abs(got[1] / ss - 1.0), abs(got[3] / sg - 1.0))
        print("m = %s x = %g: %.1e (table %.1e)" % (m, x, dev, VS_SCIPY[im][ix]))
        assert dev <= 10.0 * VS_SCIPY[im][ix], (m, x, dev)
        assert 0.0 < got[1] < got[0] and -1.0 < got[3] < 1.0
        # without absorption everything that is removed is scattered
        qe, qs, _, _ = radiometer_sphere(x, complex(m.real, 0.0))
        assert abs(qs / qe - 1.0) <= 10.0 * VS_SCIPY[im][ix], (m.real, x, qs / qe - 1.0)


def test_rayleigh_limits():
    """Q_sca/((8/3) x**4 |K|**2) - 1, g and (Q_ext - Q_sca)/(4 x Im K) - 1 fall with x**2: the deviation at x = 0.01 is 50 to
    200 times that at 0.001 (100 to second order), as tests/test_mie_abi.py asserts for Q_back."""
    from kid_amd import radiometer_sphere
    for m in (complex(8.9, 1.4), complex(3.0, 1.7), complex(1.78, 0.003)):
        e = m * m
        K = (e - 1.0) / (e + 2.0)

        def deviations(x):
            qe, qs, _, g = radiometer_sphere(x, m)
            return qs / ((8.0 / 3.0) * x ** 4 * abs(K) ** 2) - 1.0, g, (qe - qs) / (4.0 * x * K.imag) - 1.0
        big, small = deviations(0.01), deviations(0.001)
        for name, b, s in zip(("Q_sca", "g", "Q_abs"), big, small):
            print(m, name, b, s, b / s)
            assert abs(s) < abs(b) < 1e-2 and 50.0 <= b / s <= 200.0, (m, name, b, s)


@pytest.mark.parametrize("x", ref.SPECIES)
def test_bins_against_the_restatement_on_the_default_grids(x):
    """Bit-equal rows on the scheme's own 100 bins at the default 10 cm and at 3.19 mm; 0 <= g < 1 and s_bsc >= 0 on every
    bin; with Im(eps_i) = 0 snow and graupel do not absorb at all."""
    from kid_amd import radiometer_bins, radiometer_sphere
    D = ssr.default_grids()[x][0]
    for kw in ({}, W_BAND):
        cfg = _mie_cfg(**kw)
        rows = radiometer_bins(cfg, x, D)
        want = ref.bins_bh(cfg, x, D)
        assert rows.shape == (3, 100) and np.array_equal(rows.view(np.uint64), want.view(np.uint64)), kw
        assert np.isfinite(rows).all() and (rows[0] >= 0).all() and (rows[1] >= 0).all() and (rows[1] > 0).any() and (rows[2] > 0).all()
        if x != "r" and not kw:
            assert (rows[0].view(np.uint64) == 0).all()
        else:
            assert (rows[0] > 0).all()
        for d in D:
            mass = (mie_ref.PI_S / 6.0) * cfg.rho_w * d ** 3 if x == "r" else mie_ref.AM_S * d * d if x == "s" else mie_ref.AM_G * d ** 3
            g = radiometer_sphere(math.pi * float(d) / cfg.wavelength, complex(*mie_ref.index_of(cfg, x, float(d), mass)))[3]
            assert 0.0 <= g < 1.0, (kw, x, d, g)


# ---- the per-particle model and the layer as a host program of its own, with and without ASan + UBSan ----
def test_host_program_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    # the sanitizers' runtimes are linked statically: the program is instrumented by itself and runs in the environment as it is
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else ["-static-libsan"]
    common = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
              os.path.join(ROOT, "tests", "native", "radiometer_check.cpp")]
    san, plain = tmp_path / "rad_san", tmp_path / "rad_plain"
    subprocess.run(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + static
                   + ["-o", str(san)], check=True)
    subprocess.run(common + ["-o", str(plain)], check=True)
    a = subprocess.run([str(san)], capture_output=True, text=True)
    b = subprocess.run([str(plain)], capture_output=True, text=True)
    assert a.returncode == 0 and a.stdout.strip().endswith("radiometer ok") and "runtime error" not in a.stderr and "Sanitizer" not in a.stderr, \
        a.stdout[-2000:] + a.stderr
    lines = [ln.split() for ln in b.stdout.splitlines()]
    nl = sum(ln[0] == "l" for ln in lines)
    assert b.returncode == 0 and a.stdout == b.stdout and nl >= 12 and len(lines) == 40 + nl + nl * nl + 1
    # the program's numbers are the library's and the restatement's, with the host libm on both sides
    from kid_amd import radiometer_sphere
    states, taken = [], set()
    for ln in lines:
        if ln[0] == "q":
            x, mr, mi, qe, qs, qb, g = (float.fromhex(v) for v in ln[1:])
            assert radiometer_sphere(x, complex(mr, mi)) == (qe, qs, qb, g) == ref.sphere_bh(x, complex(mr, mi))[:4]
        elif ln[0] == "l":
            ta, b_, mu, t, e, f, R, T, a_ = (float.fromhex(v) for v in ln[1:])
            x = float(ref.layer_x(ta, b_))
            assert (e, f) == ref.host_ef(x / mu), ln
            want = tuple(float(v) for v in ref.layer(ta, b_, x, mu, e, f))
            assert (R, T, a_) == want, (ln, want)
            taken.add("identity" if ta == 0 and b_ == 0 else "conservative" if ta == 0 else "schwarzschild" if b_ == 0 else
                      "thick" if x / mu > 700 else "tiny" if ta < 1e-200 else "general")
            states.append(ref.state_of(R, T, a_, t))
        elif ln[0] == "c":
            i, j = int(ln[1]), int(ln[2])
            got = tuple(float.fromhex(v) for v in ln[3:])
            assert got == tuple(float(v) for v in ref.combine(states[i], states[j])), ln
    assert taken == {"identity", "conservative", "schwarzschild", "thick", "tiny", "general"}


# ---- algebra on the restatement alone ----
def _case_layers(name, nz):
    import doppler_ref as dref
    from kid_amd import radiometer_bins
    from oracle.oracle import Oracle
    o = Oracle(iiwarm=True)
    c = dref.constants(o)
    o.close()
    g = ssr.default_grids()
    table = {x: (g[x][0], g[x][1], radiometer_bins(_mie_cfg(**rc.TABLES[name]), x, g[x][0])) for x in ref.SPECIES}
    st, dz, k_gas, t_sfc = rc.state(nz)
    kg = k_gas if rc.USES_GAS[name] else None
    return c, table, st, dz, kg, t_sfc


@pytest.mark.parametrize("name", sorted(rc.TABLES))
def test_layer_closes_and_the_identity_is_neutral(name):
    c, table, st, dz, kg, t_sfc = _case_layers(name, 200)
    kabs, kbsc, temp = ref.optics(c, rc.cfg_of(name), table, st, kg)
    ta, b, R, T, E = ref.layers(kabs, kbsc, temp, dz, rc.RCFG["mu"])
    x = ref.layer_x(ta, b)
    e, f = ref.device_ef(x / rc.RCFG["mu"])
    a = ref.layer(ta, b, x, rc.RCFG["mu"], e, f)[2]
    print("a - (1 - R - T), ulp of 1: %.2f" % (float(np.max(np.abs(a - (1.0 - R - T)))) / ULP))
    assert (np.abs(a - (1.0 - R - T)) <= 4.0 * ULP).all() and (a >= 0).all()
    own = (R, R, T, E, E)
    ident = tuple(np.full_like(R, v) for v in ref.IDENTITY)
    for got in (ref.combine(own, ident), ref.combine(ident, own)):
        assert all(np.array_equal(u.view(np.uint64), v.view(np.uint64)) for u, v in zip(got, own))
    assert rc.branches(ta, b)[1] > 0 and (name == "absorbing" or min(rc.branches(ta, b)) > 0)


@pytest.mark.parametrize("name", sorted(rc.TABLES))
def test_scan_order_and_sequential_adding_agree(name):
    worst = 0.0
    for nz in rc.NZS:
        c, table, st, dz, kg, t_sfc = _case_layers(name, nz)
        a = ref.radiometer(c, rc.cfg_of(name), table, st, dz, kg, t_sfc, **rc.RCFG)
        b = ref.radiometer(c, rc.cfg_of(name), table, st, dz, kg, t_sfc, order=ref.sequential, **rc.RCFG)
        worst = max(worst, max(float(np.max(ref.ulps(a[k], b[k]))) for k in ("tb_up", "tb_down")))
    print("scan order against sequential adding, ulp: %.1f" % worst)
    assert worst <= 4.0 * SCAN_VS_SEQUENTIAL


# ---- the wrappers refuse wrong input before the library is reached ----
def _fake_table(model):
    from kid_amd import RadiometerTable
    t = RadiometerTable.__new__(RadiometerTable)
    t._t, t.model = C.c_void_p(1), model
    return t


def test_wrappers_reject_bad_arguments_before_the_library(monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import RADIOMETER_INPUTS, RadiometerCfg, RadiometerTable
    N, NZ = 4, 30
    good = lambda: {k: np.zeros((N, NZ)) for k in RADIOMETER_INPUTS}   # noqa: E731
    m = tma._bare()
    t = _fake_table(m)
    monkeypatch.setattr(th, "load_library", lambda *a: tma._NoLibrary())
    monkeypatch.setattr(RadiometerTable, "close", lambda self: None)
    dz = np.ones(NZ)
    nan = float("nan")
    cases = [
        ([np.zeros((N, NZ))], {}), ({k: v.astype(np.float16) for k, v in good().items()}, {}), ({k: np.zeros(NZ) for k in RADIOMETER_INPUTS}, {}),
        ({k: np.zeros((N, 1)) for k in RADIOMETER_INPUTS}, {}), ({k: np.zeros((N, 257)) for k in RADIOMETER_INPUTS}, {}),
        ({k: v for k, v in good().items() if k != "qr"}, dict(dz=dz)), (dict(good(), qs=np.zeros((N, NZ), dtype=np.float32)), dict(dz=dz)),
        (dict(good(), p=np.zeros((NZ, N)).T), dict(dz=dz)), (good(), dict(dz=dz, want=("tb_toa", "tb"))), (good(), dict(dz=dz, want=("refl", "refl"))),
        (good(), dict(dz=dz, want=())), (good(), dict(dz=dz, want=3)), (good(), dict(want=("tb_toa",))), (good(), dict(want=("tau_abs",))),
        (good(), dict(want=("k_abs", "trans"))), (good(), dict(dz=np.ones(NZ + 1))), (good(), dict(dz=[1.0] * NZ)), (good(), dict(dz=dz.astype(np.float32))),
        (good(), dict(dz=dz, k_gas=np.ones((NZ, N)))), (good(), dict(dz=dz, t_sfc=np.ones(NZ))), (good(), dict(dz=dz, t_sfc=[280.0] * N)),
        (good(), dict(dz=dz, out=[np.zeros(N)])), (good(), dict(dz=dz, out={"tb_toa": np.zeros((N, NZ))})),
        (good(), dict(dz=dz, want=("tb_up",), out={"tb_up": np.zeros(N)})),
        (good(), dict(dz=dz, rcfg=dict(mu=1.0))), (good(), dict(dz=dz, rcfg=RadiometerCfg(mu=0.0))), (good(), dict(dz=dz, rcfg=RadiometerCfg(mu=1.5))),
        (good(), dict(dz=dz, rcfg=RadiometerCfg(mu=nan))), (good(), dict(dz=dz, rcfg=RadiometerCfg(emissivity=-0.1))),
        (good(), dict(dz=dz, rcfg=RadiometerCfg(emissivity=1.1))), (good(), dict(dz=dz, rcfg=RadiometerCfg(t_cosmic=-1.0))),
        (good(), dict(dz=dz, rcfg=RadiometerCfg(t_cosmic=float("inf")))), (good(), dict(dz=dz, rcfg=RadiometerCfg(mu="one"))),
    ]
    for st, kw in cases:
        with pytest.raises(th.KidmpError, match="radiometer_host"):
            m.radiometer_host(t, st, **kw)
    for bad_table in (None, "table", _fake_table(tma._bare()), tma._fake_table(m)):
        with pytest.raises(th.KidmpError, match="radiometer_host"):
            m.radiometer_host(bad_table, good(), dz)
    import torch
    with pytest.raises(th.KidmpError, match="radiometer"):
        m.radiometer(t, {k: torch.zeros(N, NZ, dtype=torch.float64) for k in RADIOMETER_INPUTS}, torch.ones(NZ, dtype=torch.float64))   # host memory
    with pytest.raises(th.KidmpError, match="radiometer"):
        m.radiometer(t, good(), dz)
    for grids in ([1], {"c": (dz, dz)}, {"r": (dz, None)}, {"r": (np.ones(0), np.ones(0))}, {"s": (np.ones(257), np.ones(257))},
                  {"g": (dz, np.ones(NZ + 1))}, {"g": (dz.astype(np.float32), dz.astype(np.float32))}):
        with pytest.raises(th.KidmpError, match="RadiometerTable"):
            m.radiometer_table(None, grids)
    with pytest.raises(th.KidmpError, match="RadiometerTable"):
        m.radiometer_table({"wavelength": 0.1})
