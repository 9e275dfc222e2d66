"""The polarimetric radar (include/kidmp_polarimetric.h, kid_amd/polarimetric.py) without a GPU: the entries exist in the
built library and in the header, kid_amd/polarimetric.py declares them as the header has them, the header compiles as C99
and C++11, a missing context is refused, every bad configuration is refused with nothing written, and the spheroid of
kid_amd/csrc/kidmp_spheroid.h is held against its restatement in tests/polarimetric_ref.py.

kidmp_pol_spheroid and kidmp_pol_bins against the restatement (Python floats, operation for operation; sqrt, atan and exp
are the host libm's on both sides): the largest difference measured on the CPU, over every case of this file, is 0 ulp --
the two are bit-equal -- so the bound is the least one, 64 ulp of the largest row of the bin's |.|-kind (c_im, which
cancels to zero at the sphere, is held in ulp of c_re).  MEASURED_ULP below records it.

The shape factor: 1/3 exactly at r = 1; closed form and series agree to 1.2e-14 (relative) at the switch f**2 = 1/64
(4.7e-15 measured for this order of operations); L_a + 2 L_b = 1 to 2 ulp.  The moments at sigma = 0 are (1, 0, 1, 0, 0, 1) exactly.

Rain's Z_DR on the CPU, from the rows alone with n = exp(-lam D) dD on 256 bins to 8 mm and sigma = 0: 0.949 dB at
lam = 3000 1/m and 2.733 dB at lam = 1500 1/m for the default (Brandes) law.  (The scheme's own rain bins end at 4.9 mm
and give 0.928 and 1.973 dB; the default sigma of 10 degrees takes 0.08 and 0.25 dB off.)
"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import polarimetric_ref as ref
import size_spectra_ref as ssr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_polarimetric.h")
CSRC = os.path.join(ROOT, "kid_amd", "csrc")
ENTRIES = ("kidmp_polarimetric_device", "kidmp32_polarimetric_device", "kidmp_polarimetric_host", "kidmp32_polarimetric_host")
SYMBOLS = ENTRIES + ("kidmp_pol_defaults", "kidmp_pol_spheroid", "kidmp_pol_bins", "kidmp_pol_table_create", "kidmp_pol_table_destroy",
                     "kidmp_pol_table_get")
SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "size_t": (C.c_size_t,), "double": (C.c_double,),
           "float": (C.c_float,), "int": (C.c_int, C.c_int32), "void": (None,)}
EINVAL, ESTATE = -1, -5
ULP = 2.220446049250313e-16
MEASURED_ULP = 0.0                                              # library against restatement, see the module docstring
BOUND_ULP = max(4.0 * MEASURED_ULP, 64.0)
SWITCH_GAP = 1.2e-14                                            # closed form against series at f**2 = 1/64, relative

# a second configuration beside the defaults: illustrative C-band values, not taken from a table of record
OTHER_MIE = dict(wavelength=0.055, eps_w=complex(72.0, 35.0), eps_i=complex(3.17, 0.003), rho_w=1000.0, rho_i=917.0, kw2=0.93)
OTHER_POL = dict(axis_r_min=0.5, axis_s=0.6, axis_g=1.0, sigma=(0.0, 0.3, math.radians(40.0)))


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


def _cfgs(mie=None, pol=None):
    from kid_amd import MieCfg, PolCfg
    return MieCfg(**(mie or {})), PolCfg(**(pol or {}))


def _close(got, want, scale=None):
    """|got - want| <= BOUND_ULP ulp of max(|want|, scale)."""
    s = np.maximum(np.abs(want), 0.0 if scale is None else np.abs(scale))
    return bool(np.all(np.abs(got - want) <= BOUND_ULP * ULP * s))


# ---- the ABI ----
def test_symbols_are_exported_and_prototyped():
    lib = os.path.join(ROOT, "kid_amd", "libkidmp.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(lib)
    assert sorted(_prototypes()) == sorted(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert '#include "kidmp_mie.h"' in open(HEADER).read()


def test_the_python_declarations_match_the_header():
    import kid_amd
    import kid_amd.polarimetric as kp
    declared = kp.declare(_Stub()).entries
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
    for struct, elem in (("kidmp_pol_out", "double"), ("kidmp32_pol_out", "float")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _code(), re.S).group(1)
        assert body.split()[0] == elem
        members = [m.strip().lstrip("*") for m in re.sub(r"\b%s\b" % elem, "", body).replace(";", ",").split(",") if m.strip()]
        assert tuple(members) == kp.POL_NAMES == kid_amd.POL_NAMES == ref.NAMES
    assert [n for n, _ in kp._PolOut._fields_] == list(kp.POL_NAMES) and all(t is C.c_void_p for _, t in kp._PolOut._fields_)
    cfg = re.search(r"typedef struct kidmp_pol_cfg \{(.*?)\} kidmp_pol_cfg;", _code(), re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\w+\])?\s*[,;]", cfg)
    assert names == [n for n, _ in kp._PolCfg._fields_] == ["axis_r", "axis_r_min", "axis_s", "axis_g", "sigma", "force_quadrature"]
    assert C.sizeof(kp._PolCfg) == 96 and kp._PolCfg.force_quadrature.offset == 88
    raw = open(HEADER).read()
    assert int(re.search(r"#define KIDMP_POL_NROWS (\d+)", raw).group(1)) == len(kp.POL_ROWS) == len(ref.ROWS) == 7
    assert int(re.search(r"#define KIDMP_POL_NSCALARS (\d+)", raw).group(1)) == len(kp.POL_SCALARS) == 5
    assert kp.POL_ROWS == ref.ROWS and kp.POL_INPUTS == ref.INPUTS
    # the header says what is not modelled and that parity is unpinned
    for word in ("melting particles", "T-matrix", "differential attenuation", "backscatter differential phase", "LDR", "cloud ice",
                 "temperature-dependent", "unpinned", "illustrative, not values of record", "Ryzhkov"):
        assert word in raw, word


def test_only_the_polarimetric_mirror_declares_them():
    import kid_amd.mie as km
    import kid_amd.polarimetric as kp
    import kid_amd.radiometer as kr
    import kid_amd.thompson as th
    assert sorted(kp._declarations()) == sorted(SYMBOLS)
    for other in (th, km, kr):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_polarimetric.h"\n'
                   "int use(kidmp_ctx *c, const double *a, kidmp_mie_cfg *f, kidmp_pol_cfg *q, kidmp_mie_grids *g, kidmp_pol_out *o, double *r)\n"
                   "{ kidmp_pol_table *t; int32_t nb, u; kidmp_mie_defaults(f); kidmp_pol_defaults(q); q->sigma[KIDMP_MIE_R] = 0.1;\n"
                   "  if (kidmp_pol_spheroid(79.5, 24.9, 0.8, 0.1, r) || kidmp_pol_bins(f, q, KIDMP_MIE_S, 1, a, r)) return 1;\n"
                   "  if (kidmp_pol_table_create(c, f, q, g, &t) || kidmp_pol_table_get(t, KIDMP_MIE_G, &nb, r, r, r, f, q, &u, r)) return 2;\n"
                   "  nb = kidmp_polarimetric_host(c, t, 1, 2, a, a, a, a, a, a, a, o);\n"
                   "  kidmp_pol_table_destroy(t); return nb + KIDMP_POL_NROWS + KIDMP_POL_NSCALARS; }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.mie import _MieCfg, _MieGrids
    from kid_amd.polarimetric import _PolCfg, _PolOut, library
    L = library()
    o, g, c, p = _PolOut(), _MieGrids(), _MieCfg(), _PolCfg()
    L.kidmp_mie_defaults(C.byref(c))
    L.kidmp_pol_defaults(C.byref(p))
    args = [None, None, 4, 120] + [None] * 7 + [C.byref(o)]
    assert L.kidmp_polarimetric_host(*args) == ESTATE and L.kidmp32_polarimetric_host(*args) == ESTATE
    assert L.kidmp_polarimetric_device(*args, None) == ESTATE and L.kidmp32_polarimetric_device(*args, None) == ESTATE
    h = C.c_void_p(1)
    assert L.kidmp_pol_table_create(None, C.byref(c), C.byref(p), C.byref(g), C.byref(h)) == ESTATE and h.value is None
    assert L.kidmp_pol_table_get(None, 0, None, None, None, None, None, None, None, None) == EINVAL
    L.kidmp_pol_table_destroy(None)


def test_the_defaults():
    from kid_amd.polarimetric import PolCfg, _PolCfg, library
    c = _PolCfg()
    library().kidmp_pol_defaults(C.byref(c))
    py, rf = PolCfg(), ref.PolCfg()
    assert tuple(c.axis_r) == py.axis_r == rf.axis_r == (0.9951, 0.02510, -0.03644, 0.005303, -0.0002492)
    assert (c.axis_r_min, c.axis_s, c.axis_g, c.force_quadrature) == (0.2, 0.75, 0.8, 0)
    assert (py.axis_r_min, py.axis_s, py.axis_g, py.force_quadrature) == (0.2, 0.75, 0.8, False)
    assert tuple(c.sigma) == rf.sigma
    for got, deg in zip(py.sigma, (10.0, 40.0, 40.0)):
        assert abs(got - math.radians(deg)) <= ULP * got
    for got, want in zip(c.sigma, py.sigma):
        assert abs(got - want) <= ULP * want


# ---- the particle ----
def test_the_shape_factor():
    assert ref.shape(1.0) == (1.0 / 3.0, 1.0 / 3.0) and ref.shape(1.5) == (1.0 / 3.0, 1.0 / 3.0)
    f2 = 1.0 / 64.0
    gap = abs(ref.shape_closed(f2) / ref.shape_series(f2) - 1.0)
    print("closed form against series at the switch: %.2e" % gap)
    assert gap <= SWITCH_GAP
    # continuous across the switch: the two sides of f**2 = 1/64 an ulp of r apart
    r0 = 1.0 / math.sqrt(1.0 + f2)
    lo, hi = r0, r0
    while not 1.0 / (lo * lo) - 1.0 >= f2:
        lo = math.nextafter(lo, 0.0)
    while not 1.0 / (hi * hi) - 1.0 < f2:
        hi = math.nextafter(hi, 1.0)
    assert 1.0 / (lo * lo) - 1.0 >= f2 > 1.0 / (hi * hi) - 1.0 and hi - lo <= 4.0 * ULP
    assert abs(ref.shape(lo)[0] / ref.shape(hi)[0] - 1.0) <= SWITCH_GAP
    last = 1.0
    for r in (1e-3, 0.05, 0.2, 0.5, 0.75, 0.9, 0.99, lo, hi, 0.9925, 0.999, 0.9999999, 1.0):
        La, Lb = ref.shape(r)
        assert abs((La + 2.0 * Lb) - 1.0) <= 2.0 * ULP, r
        assert 1.0 / 3.0 <= La <= last * (1.0 + SWITCH_GAP) and Lb <= 1.0 / 3.0, r   # falls towards the sphere's 1/3
        last = La
    # a 2:1 oblate spheroid in closed form: f = sqrt(3), atan(f) = pi/3
    assert abs(ref.shape(0.5)[0] - (4.0 / 3.0) * (1.0 - math.pi / (3.0 * math.sqrt(3.0)))) < 1e-15


def test_the_moments_at_no_canting_and_at_random_orientation():
    from kid_amd import pol_spheroid
    assert ref.moments(0.0) == (1.0, 0.0, 1.0, 0.0, 0.0, 1.0)
    eps = complex(79.5, 24.9)
    for ratio in (0.3, 0.8, 0.995):
        rows = pol_spheroid(eps, ratio, 0.0)
        La, Lb = ref.shape(ratio)
        Pa, Pb = ref.spheroid_P((eps.real, eps.imag), La), ref.spheroid_P((eps.real, eps.imag), Lb)
        pa2, pb2 = Pa[0] * Pa[0] + Pa[1] * Pa[1], Pb[0] * Pb[0] + Pb[1] * Pb[1]
        assert rows[0] == pb2                                                     # s_h = D**6 |P_b|**2, exactly
        assert abs(rows[1] - pa2) <= 8.0 * ULP * pb2                              # s_v = |P_b - Delta|**2 = |P_a|**2
        assert rows[0] > rows[4] > rows[1] > 0.0 and rows[5] > 0.0 and rows[6] == 0.0
        c = complex(rows[2], rows[3])
        assert abs(c - complex(*Pb).conjugate() * complex(*Pa)) <= 8.0 * ULP * pb2
    A1, A2, A3, A4, A5, A7 = ref.moments(10.0)                                    # q = exp(-200): nothing is left of it
    assert (A1, A2, A3, A4) == (0.25, 0.25, 0.140625, 0.140625) and A5 == 0.046875 and 0.0 < A7 < 1e-86
    rows = pol_spheroid(eps, 0.5, 10.0)
    assert rows[0] == rows[1] and 0.0 < rows[5] < 1e-86


def test_the_sphere_limit_of_the_rows():
    """Every axis ratio 1: rows 0, 1, 2 and 4 are the same bits, row 3 and row 5 are +0.0, for any sigma."""
    from kid_amd import pol_bins, pol_spheroid
    for sigma in (0.0, 0.2, 3.0):
        rows = pol_spheroid(complex(3.17, 0.01), 1.0, sigma)
        assert rows[0].hex() == rows[1].hex() == rows[2].hex() == rows[4].hex() and rows[3].hex() == rows[5].hex() == (0.0).hex()
    mie, pol = _cfgs(pol=dict(axis_r=(1.0, 0.0, 0.0, 0.0, 0.0), axis_s=1.0, axis_g=1.0))
    for x in ref.SPECIES:
        rows = pol_bins(mie, pol, x, ssr.default_grids()[x][0])
        b = rows.view(np.uint64)
        assert (b[0] == b[1]).all() and (b[0] == b[2]).all() and (b[0] == b[4]).all() and (b[3] == 0).all() and (b[5] == 0).all(), x
        assert (rows[0] > 0).all() and (rows[6] > 0).all()


@pytest.mark.parametrize("which", ["defaults", "other"])
def test_spheroid_and_bins_against_the_restatement(which):
    from kid_amd import pol_bins, pol_spheroid
    mkw, pkw = ({}, {}) if which == "defaults" else (OTHER_MIE, OTHER_POL)
    mie, pol = _cfgs(mkw, pkw)
    rmie, rpol = ref.cfg_of(**mkw), ref.PolCfg(**pkw)
    worst = 0.0
    for x in ref.SPECIES:
        D = ssr.default_grids()[x][0]
        got, want = pol_bins(mie, pol, x, D), ref.bins(rmie, rpol, x, D)
        assert got.shape == (7, 100) and np.isfinite(got).all()
        for i in range(7):
            scale = want[2] if i == 3 else None                                   # c_im in ulp of c_re
            s = np.maximum(np.abs(want[i]), 0.0 if scale is None else np.abs(scale))
            worst = max(worst, float(np.max(np.abs(got[i] - want[i]) / (ULP * np.where(s > 0.0, s, 1.0)))))
            assert _close(got[i], want[i], scale), (x, ref.ROWS[i])
        assert (got[0] > 0).all() and (got[1] > 0).all() and (got[4] > 0).all() and (got[5] >= 0).all() and (got[6] > 0).all()
        assert (got[0] >= got[1]).all()                                           # oblate: never more at vertical polarisation
    for eps in (complex(79.5, 24.9), complex(3.17, 0.01), complex(1.3, 0.0)):
        for ratio in (1.0, 0.995, 0.8, 0.3):
            for sigma in (0.0, math.radians(10.0), math.radians(40.0)):
                got = pol_spheroid(eps, ratio, sigma)
                want = np.array(ref.spheroid_rows((eps.real, eps.imag), ratio, ref.moments(sigma), 1.0) + [0.0])
                for i in range(7):
                    scale = want[2] if i == 3 else None
                    s = max(abs(want[i]), 0.0 if scale is None else abs(scale))
                    if s > 0.0:
                        worst = max(worst, abs(got[i] - want[i]) / (ULP * s))
                    assert _close(got[i], want[i], scale), (eps, ratio, sigma, i)
    print("library against restatement: %.2f ulp at most" % worst)


def test_rain_zdr_from_the_rows_alone():
    """The CPU check of the default law at sigma = 0: n = exp(-lam D) dD on 256 bins to 8 mm, Z_DR = 10 log10(sum n s_h/sum n s_v)."""
    from kid_amd import pol_bins
    dD = np.full(256, 8e-3 / 256)
    D = (np.arange(256) + 0.5) * dD
    rows = pol_bins(*_cfgs(pol=dict(sigma=(0.0, 0.0, 0.0))), "r", D)
    zdr = {}
    for lam in (3000.0, 1500.0):
        n = np.exp(-lam * D) * dD
        zdr[lam] = 10.0 * math.log10(float(np.sum(n * rows[0]) / np.sum(n * rows[1])))
    print("zdr of rain: %.3f dB at 3000 1/m, %.3f dB at 1500 1/m" % (zdr[3000.0], zdr[1500.0]))
    assert abs(zdr[3000.0] - 0.95) < 0.005 and abs(zdr[1500.0] - 2.7) < 0.05


def test_every_bad_configuration_is_refused():
    """KIDMP_EINVAL from the library itself (kidmp_pol_bins needs no context), nothing written; the Python mirror refuses
    the same before the library is reached."""
    from kid_amd import KidmpError, pol_bins, pol_spheroid
    from kid_amd.mie import _MieCfg
    from kid_amd.polarimetric import _PolCfg, library
    L = library()
    D = np.array([1e-3, 2e-3])
    rows = np.full((7, 2), -7.0)
    good_m = _MieCfg()
    L.kidmp_mie_defaults(C.byref(good_m))

    def call(species=0, nb=2, d=D, mie=None, **kw):
        p = _PolCfg()
        L.kidmp_pol_defaults(C.byref(p))
        for k, v in kw.items():
            if isinstance(v, tuple):
                i, val = v
                getattr(p, k)[i] = val
            else:
                setattr(p, k, v)
        m = _MieCfg()
        L.kidmp_mie_defaults(C.byref(m))
        for k, v in (mie or {}).items():
            setattr(m, k, v)
        return L.kidmp_pol_bins(C.byref(m), C.byref(p), species, nb, d.ctypes.data, rows.ctypes.data)

    nan, inf = float("nan"), float("inf")
    bad = [dict(axis_r=(0, nan)), dict(axis_r=(4, inf)), dict(axis_r_min=0.0), dict(axis_r_min=-0.2), dict(axis_r_min=1.5), dict(axis_r_min=nan),
           dict(axis_s=0.0), dict(axis_s=1.0000001), dict(axis_s=nan), dict(axis_g=-0.8), dict(axis_g=2.0), dict(axis_g=inf),
           dict(sigma=(0, -1e-9)), dict(sigma=(1, -1.0)), dict(sigma=(2, nan)), dict(sigma=(0, inf)),
           dict(mie=dict(rho_i=0.0)), dict(mie=dict(eps_w_im=-0.1)), dict(mie=dict(wavelength=nan))]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert L.kidmp_last_error(None), kw
    assert call(species=3) == EINVAL and call(species=-1) == EINVAL and call(nb=0) == EINVAL
    assert call(d=np.array([1e-3, 0.0])) == EINVAL and call(d=np.array([nan, 1e-3])) == EINVAL
    p = _PolCfg()
    L.kidmp_pol_defaults(C.byref(p))
    assert L.kidmp_pol_bins(None, C.byref(p), 0, 2, D.ctypes.data, rows.ctypes.data) == EINVAL
    assert L.kidmp_pol_bins(C.byref(good_m), None, 0, 2, D.ctypes.data, rows.ctypes.data) == EINVAL
    assert (rows == -7.0).all()
    one = np.full(7, -7.0)
    for args in ((nan, 0.0, 0.8, 0.1), (79.5, -1.0, 0.8, 0.1), (-2.0, 0.0, 0.8, 0.1), (79.5, 24.9, 0.0, 0.1), (79.5, 24.9, 1.01, 0.1),
                 (79.5, 24.9, nan, 0.1), (79.5, 24.9, 0.8, -0.1), (79.5, 24.9, 0.8, inf)):
        assert L.kidmp_pol_spheroid(*args, one.ctypes.data) == EINVAL, args
    assert L.kidmp_pol_spheroid(79.5, 24.9, 0.8, 0.1, None) == EINVAL and (one == -7.0).all()
    assert call() == 0 and np.isfinite(rows).all() and call(axis_s=1.0, axis_r_min=1.0, sigma=(0, 0.0)) == 0
    mie, _ = _cfgs()
    from kid_amd import PolCfg
    for kw in (dict(axis_s=0.0), dict(axis_g=1.5), dict(axis_r_min=nan), dict(sigma=(0.1, -0.1, 0.1)), dict(sigma=(0.1, 0.1)), dict(axis_r=(1.0, 0.0)),
               dict(axis_r=(1.0, 0.0, 0.0, 0.0, inf)), dict(axis_s="flat")):
        with pytest.raises(KidmpError, match="pol_bins"):
            pol_bins(mie, PolCfg(**kw), "r", D)
    with pytest.raises(KidmpError, match="pol_bins"):
        pol_bins(mie, PolCfg(), "c", D)
    with pytest.raises(KidmpError, match="pol_bins"):
        pol_bins(mie, {"axis_s": 1.0}, "r", D)
    with pytest.raises(KidmpError):
        pol_spheroid(complex(79.5, 24.9), 0.0, 0.1)


# ---- the per-particle model as a host program of its own, with and without ASan + UBSan ----
def test_spheroid_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    # the sanitizers' runtimes are linked statically: the program is instrumented by itself and runs in the environment as it is
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else ["-static-libsan"]
    common = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
              os.path.join(ROOT, "tests", "native", "spheroid_check.cpp")]
    san, plain = tmp_path / "spheroid_san", tmp_path / "spheroid_plain"
    subprocess.run(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + static
                   + ["-o", str(san)], check=True)
    subprocess.run(common + ["-o", str(plain)], check=True)
    a = subprocess.run([str(san)], capture_output=True, text=True)
    b = subprocess.run([str(plain)], capture_output=True, text=True)
    assert a.returncode == 0 and a.stdout.strip().endswith("spheroid ok") and "runtime error" not in a.stderr and "Sanitizer" not in a.stderr, \
        a.stdout[-2000:] + a.stderr
    assert b.returncode == 0 and a.stdout == b.stdout and len(a.stdout.splitlines()) == 16 + 6 + 36 + 2 * 3 * 24 + 1
    # the program's numbers are the restatement's, at the bound of this file
    for ln in (ln.split() for ln in b.stdout.splitlines()):
        v = [float.fromhex(t) for t in ln[1:]] if ln[0] in "las" else None
        if ln[0] == "l":
            assert tuple(v[1:]) == ref.shape(v[0])
        elif ln[0] == "a":
            assert tuple(v[1:]) == ref.moments(v[0])
        elif ln[0] == "s":
            want = np.array(ref.spheroid_rows((v[0], v[1]), v[2], ref.moments(v[3]), 1.0))
            got = np.array(v[4:])
            assert _close(np.delete(got, 3), np.delete(want, 3)) and _close(got[3], want[3], want[2])


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
    from kid_amd import PolTable
    t = PolTable.__new__(PolTable)
    t._t, t.model = C.c_void_p(1), model
    return t


def test_wrappers_reject_bad_arguments_before_the_library(monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import POL_INPUTS, PolCfg, PolTable
    N, NZ = 4, 30
    good = lambda: {k: np.zeros((N, NZ)) for k in POL_INPUTS}   # noqa: E731
    m = _bare()
    t = _fake_table(m)
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    monkeypatch.setattr(PolTable, "close", lambda self: None)
    cases = [
        ([np.zeros((N, NZ))], {}), ({k: v.astype(np.float16) for k, v in good().items()}, {}), ({k: np.zeros(NZ) for k in POL_INPUTS}, {}),
        ({k: np.zeros((N, 1)) for k in POL_INPUTS}, {}), ({k: np.zeros((N, 257)) for k in POL_INPUTS}, {}),
        ({k: v for k, v in good().items() if k != "qr"}, {}), (dict(good(), qs=np.zeros((N, NZ), dtype=np.float32)), {}),
        (dict(good(), p=np.zeros((NZ, N)).T), {}), (good(), dict(want=("zdr", "dbz"))), (good(), dict(want=("kdp", "kdp"))), (good(), dict(want=())),
        (good(), dict(want=3)), (good(), dict(out=[np.zeros((N, NZ))])), (good(), dict(out={"zdr": np.zeros((NZ, N))})),
        (good(), dict(out={"zdr": np.zeros((N, NZ), dtype=np.float32)})),
    ]
    for st, kw in cases:
        with pytest.raises(th.KidmpError, match="polarimetric_host"):
            m.polarimetric_host(t, st, **kw)
    for bad_table in (None, "table", _fake_table(_bare())):
        with pytest.raises(th.KidmpError, match="polarimetric_host"):
            m.polarimetric_host(bad_table, good())
    import torch
    with pytest.raises(th.KidmpError, match="polarimetric"):
        m.polarimetric(t, {k: torch.zeros(N, NZ, dtype=torch.float64) for k in POL_INPUTS})   # host memory
    with pytest.raises(th.KidmpError, match="polarimetric"):
        m.polarimetric(t, good())
    dz = np.ones(NZ)
    for grids in ([1], {"c": (dz, dz)}, {"r": (dz, None)}, {"r": (np.ones(0), np.ones(0))}, {"s": (np.ones(257), np.ones(257))},
                  {"g": (dz, np.ones(NZ + 1))}, {"g": (dz.astype(np.float32), dz.astype(np.float32))}):
        with pytest.raises(th.KidmpError, match="PolTable"):
            m.pol_table(None, None, grids)
    with pytest.raises(th.KidmpError, match="PolTable"):
        m.pol_table({"wavelength": 0.1})
    with pytest.raises(th.KidmpError, match="PolTable"):
        m.pol_table(None, PolCfg(axis_g=0.0))
    with pytest.raises(th.KidmpError, match="PolTable"):
        m.pol_table(None, {"axis_g": 1.0})
