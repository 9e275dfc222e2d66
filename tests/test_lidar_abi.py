"""The lidar operator (include/kidmp_lidar.h, kid_amd/lidar.py) without a GPU: the four symbols exist in the built library
and in the new header, kid_amd/lidar.py declares them as the header has them, the header compiles as C99 and C++11, a
missing context is refused, the Python wrappers turn wrong arguments away before the library is called, and the numpy
reference of the GPU tests (tests/lidar_ref.py) gives known answers: each extinction against a trapezoid quadrature of
(pi/2) D**2 N_x(D), the telescoping identity of the attenuated backscatter, g against expm1, and the cloud-water optical
depth against the column summary's TAU_C.

Bounds (none is a measured number): the quadrature is held to QUAD_RTOL = 1e-10 as in test_doppler_abi.py; the identity
to 16 nz ulp of its right-hand side as the issue states it; g to 4 ulp (exp, sinh, one product and the 0.5 ulp of expm1
and its division); TAU_C to PI_GAP + 64 ulp relative per level term plus nz ulp for the order of the sums: 64 ulp for a cube
root, two divisions and a handful of products on each side, and PI_GAP = |pi/3.1415926536 - 1| = 3.3e-12 because the
scheme's ten-digit PI (M:35) is in am_r and so in re_qc, where the cross-section (pi/4) D**2 of the extinction has pi."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lidar_cases as lc
import lidar_ref as ref
import size_spectra_ref as ssr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_lidar.h")
SYMBOLS = ("kidmp_lidar_profiles_device", "kidmp32_lidar_profiles_device", "kidmp_lidar_profiles_host", "kidmp32_lidar_profiles_host")

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
    text = re.sub(r"enum\s*\{[^}]*\}\s*;", " ", text)
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
    import kid_amd.lidar as kl
    declared = kl.declare(_Stub()).entries
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
    for struct, elem in (("kidmp_lidar_out", "double"), ("kidmp32_lidar_out", "float")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _code(), re.S).group(1)
        assert body.split()[0] == elem
        members = [m.strip().lstrip("*") for m in body.replace(elem, "").replace(";", "").split(",")]
        assert tuple(members) == kl.LIDAR_NAMES == kid_amd.LIDAR_NAMES == ref.NAMES
    assert [n for n, _ in kl._LidarOut._fields_] == list(kl.LIDAR_NAMES) and all(t is C.c_void_p for _, t in kl._LidarOut._fields_)
    body = re.search(r"typedef struct kidmp_lidar_cfg \{(.*?)\} kidmp_lidar_cfg;", _code(), re.S).group(1)
    assert " ".join(body.split()) == "double s_ratio[5]; double eta, c_mol, beta_detect, trans_lost;"
    assert [n for n, _ in kl._LidarCfg._fields_] == ["s_ratio", "eta", "c_mol", "beta_detect", "trans_lost"]
    assert C.sizeof(kl._LidarCfg) == 9 * 8
    slots = re.search(r"enum \{(.*?)\};", _code(), re.S).group(1)
    names = [s.split("=")[0].strip().replace("KIDMP_LIDAR_", "").lower() for s in slots.split(",")]
    assert tuple(names) == kl.LIDAR_SUMMARY_NAMES == kid_amd.LIDAR_SUMMARY_NAMES == ref.SUMMARY_NAMES and len(names) == kl.LIDAR_SUMMARY_N
    assert kid_amd.LIDAR_INPUTS == ref.INPUTS
    d = ref.cfg()
    k = kl.LidarCfg()
    assert (tuple(k.s_ratio), k.eta, k.c_mol, k.beta_detect, k.trans_lost) == (d["s_ratio"], d["eta"], d["c_mol"], d["beta_detect"], d["trans_lost"])


def test_the_other_mirrors_do_not_declare_them():
    import kid_amd.doppler as dp
    import kid_amd.spectra as sp
    import kid_amd.summary as sm
    import kid_amd.thompson as th
    for other in (th, dp, sm, sp):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_lidar.h"\n'
                   "int use(kidmp_ctx *c, const double *a, kidmp_lidar_cfg *g, kidmp_lidar_out *o, double *s)\n"
                   "{ g->s_ratio[KIDMP_LIDAR_N_DN - 3] = 1.0;\n"
                   "  return kidmp_lidar_profiles_host(c, 1, 2, a, a, a, a, a, a, a, a, a, a, a, a, 0, g, o, s + KIDMP_LIDAR_SUMMARY_N); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    from kid_amd.lidar import _LidarOut, library
    L = library()
    o = _LidarOut()
    args = [None, 4, 120] + [None] * 12 + [0, None, C.byref(o), None]
    assert L.kidmp_lidar_profiles_host(*args) == -5                              # KIDMP_ESTATE
    assert L.kidmp32_lidar_profiles_host(*args) == -5
    assert L.kidmp_lidar_profiles_device(*args, None) == -5
    assert L.kidmp32_lidar_profiles_device(*args, None) == -5


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


def _bad_cfgs():
    return [
        ("cfg a number", dict(cfg=3.0)),
        ("cfg unknown key", dict(cfg=dict(etta=0.5))),
        ("cfg four ratios", dict(cfg=dict(s_ratio=(1.0, 2.0, 3.0, 4.0)))),
        ("cfg unknown species", dict(cfg=dict(s_ratio=dict(h=20.0)))),
        ("cfg ratio zero", dict(cfg=dict(s_ratio=(18.8, 0.0, 18.8, 25.0, 25.0)))),
        ("cfg ratio negative", dict(cfg=dict(s_ratio=dict(s=-25.0)))),
        ("cfg ratio nan", dict(cfg=dict(s_ratio=(18.8, 25.0, float("nan"), 25.0, 25.0)))),
        ("cfg eta zero", dict(cfg=dict(eta=0.0))),
        ("cfg eta above one", dict(cfg=dict(eta=1.0000001))),
        ("cfg eta text", dict(cfg=dict(eta="much"))),
        ("cfg c_mol negative", dict(cfg=dict(c_mol=-1e-32))),
        ("cfg c_mol zero with sr", dict(cfg=dict(c_mol=0.0), want=("att_up", "sr_dn"))),
        ("cfg beta inf", dict(cfg=dict(beta_detect=float("inf")))),
        ("cfg trans nan", dict(cfg=dict(trans_lost=float("nan")))),
    ]


def _host_cases():
    good = _host_state
    dz = np.full(NZ, 100.0)
    cases = [
        ("not a dict", [np.zeros((N, NZ))], {}),
        ("torch for numpy", {k: __import__("torch").zeros(N, NZ, dtype=__import__("torch").float64) for k in ref.INPUTS}, {}),
        ("float16", _host_state(np.float16), {}),
        ("one-dimensional", {k: np.zeros(NZ) for k in ref.INPUTS}, dict(dz=dz)),
        ("nz = 1", _host_state(nz=1), dict(dz=np.ones(1))),
        ("nz = 257", _host_state(nz=257), dict(dz=np.ones(257))),
        ("qc missing", {k: v for k, v in good().items() if k != "qc"}, dict(dz=dz)),
        ("mixed dtypes", dict(good(), qs=np.zeros((N, NZ), dtype=np.float32)), dict(dz=dz)),
        ("shapes differ", dict(good(), qr=np.zeros((N, NZ + 1))), dict(dz=dz)),
        ("not contiguous", dict(good(), p=np.zeros((NZ, N)).T), dict(dz=dz)),
        ("unknown name", good(), dict(dz=dz, want=("ext", "ext_h"))),
        ("a name twice", good(), dict(dz=dz, want=("ext", "ext"))),
        ("want a number", good(), dict(dz=dz, want=3)),
        ("nothing wanted", good(), dict(dz=dz, want=())),
        ("summary a number", good(), dict(dz=dz, summary=1)),
        ("dz missing for a depth", good(), dict(want=("ext", "tau_up"))),
        ("dz missing for the summary", good(), dict(want=("ext",), summary=True)),
        ("dz shape", good(), dict(dz=np.ones(NZ + 1))),
        ("dz dtype", good(), dict(dz=np.ones(NZ, dtype=np.float32))),
        ("dz a list", good(), dict(dz=[100.0] * NZ)),
        ("dz strided", good(), dict(dz=np.ones((N, 2 * NZ))[:, ::2])),
    ]
    return cases + [(n, good(), dict(kw, dz=dz)) for n, kw in _bad_cfgs()]


@pytest.mark.parametrize("case", _host_cases(), ids=lambda c: c[0])
def test_host_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import lidar_profiles_host
    _, st, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="lidar_profiles_host"):
        lidar_profiles_host(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="lidar_profiles_host"):
        _bare().lidar_profiles_host(st, **kw)


def _device_cases():
    """Host tensors throughout: each case is wrong in one way and, being host memory, on the wrong device as well."""
    import torch
    good = lambda dt=torch.float64, nz=NZ: {k: torch.zeros(N, nz, dtype=dt) for k in ref.INPUTS}   # noqa: E731
    dz = torch.full((NZ,), 100.0, dtype=torch.float64)
    cases = [
        ("host memory", good(), dict(dz=dz)),
        ("not a dict", [torch.zeros(N, NZ, dtype=torch.float64)], {}),
        ("numpy for torch", _host_state(), {}),
        ("float16", good(torch.float16), {}),
        ("one-dimensional", {k: torch.zeros(NZ, dtype=torch.float64) for k in ref.INPUTS}, dict(dz=dz)),
        ("nz = 1", good(nz=1), {}),
        ("nz = 257", good(nz=257), {}),
        ("qc missing", {k: v for k, v in good().items() if k != "qc"}, dict(dz=dz)),
        ("mixed dtypes", dict(good(), qg=torch.zeros(N, NZ, dtype=torch.float32)), dict(dz=dz)),
        ("shapes differ", dict(good(), nr=torch.zeros(N, NZ + 1, dtype=torch.float64)), dict(dz=dz)),
        ("unknown name", good(), dict(dz=dz, want=("lidar",))),
        ("a name twice", good(), dict(dz=dz, want=("sr_up", "ext", "sr_up"))),
        ("nothing wanted", good(), dict(dz=dz, want=[])),
        ("dz missing", good(), dict(want=("att_dn",))),
        ("dz numpy", good(), dict(dz=np.ones(NZ))),
        ("dz shape", good(), dict(dz=torch.zeros(N, dtype=torch.float64))),
    ]
    return cases + [(n, good(), dict(kw, dz=dz)) for n, kw in _bad_cfgs()]


@pytest.mark.parametrize("case", _device_cases(), ids=lambda c: c[0])
def test_device_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import lidar_profiles
    _, st, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="lidar_profiles"):
        lidar_profiles(_bare(), st, **kw)
    with pytest.raises(th.KidmpError, match="lidar_profiles"):
        _bare().lidar_profiles(st, **kw)


def test_a_configuration_is_taken_in_every_form():
    from kid_amd.lidar import LidarCfg, _cfg
    a = _cfg("t", dict(s_ratio=dict(i=30.0), eta=1.0), ())
    b = _cfg("t", LidarCfg(s_ratio=(18.8, 30.0, 18.8, 25.0, 25.0), eta=1), ())
    assert bytes(a) == bytes(b) and list(a.s_ratio) == [18.8, 30.0, 18.8, 25.0, 25.0] and a.eta == 1.0 and a.c_mol == 6.2446e-32
    assert _cfg("t", None, ()) is None and _cfg("t", dict(c_mol=0.0), ("att_up",)).c_mol == 0.0


# ---- the numpy reference ----
QUAD_RTOL = 1e-10
PI_GAP = lc.PI_GAP


@pytest.fixture(scope="module")
def consts():
    return ssr.constants()


def _quadrature(par, x, lam_min, n=40001):
    """(pi/2) * integral of D**2 N_x(D) dD for every level, trapezoid in u = log D over [1e-9 m, 200/lam_min]."""
    u = np.linspace(np.log(1e-9), np.log(200.0 / lam_min), n)
    D = np.exp(u)
    dens = ssr.spectrum(par, x, D, np.ones_like(D))["N"]                         # [..., n, nz]: N_x(D), dD = 1
    y = (0.5 * np.pi) * D[:, None] ** 3 * dens                                    # dD = D du
    return np.sum((y[..., 1:, :] + y[..., :-1, :]) * 0.5 * np.diff(u)[:, None], axis=-2)


@pytest.mark.parametrize("x", ref.SPECIES)
def test_reference_extinction_against_quadrature(consts, x):
    st = lc.one_species(x)
    o = ref.extinctions(consts, st)
    par, has = o["par"], o["has_" + x]
    assert has.sum() > 20 and not has.all()
    lam = {"c": par["lam_c"], "i": par["lam_i"], "r": par["lam_r"], "g": par["lam_g"]}.get(x)
    if x == "s":
        lam = np.where(has, par["smob"] / np.where(has, par["smoc"], 1.0), 1.0) * ssr.Lam1
    quad = _quadrature(par, x, lam[has].min())
    # Field et al.'s two-term fit is normalised to its second moment only to 2 %: the quadrature of snow's distribution
    # is smob times the second moment of the fit itself, which is a constant of the fit
    norm = 1.0
    if x == "s":
        norm = ssr.Kap0 * 2.0 / ssr.Lam0 ** 3 + ssr.Kap1 * math.gamma(3.0 + ssr.mu_s) / ssr.Lam1 ** (3.0 + ssr.mu_s)
        assert abs(norm - 1.0) < 0.03
    got = o["ext_" + x]
    assert got[has] == pytest.approx(quad[has] / norm, rel=QUAD_RTOL) and (got[has] > 0).all()
    assert not got[~has].view(np.uint64).any()                                   # +0.0 where the species is absent
    for y in ref.SPECIES:
        if y != x:
            assert not o["ext_" + y].view(np.uint64).any(), y
    p = ref.profiles(consts, st, None, ref.cfg())
    assert np.array_equal(p["ext"], got) and np.array_equal(p["bsc"], got / ref.cfg()["s_ratio"][ref.SPECIES.index(x)])
    print("ext_%s: %.3e .. %.3e m-1 over %d levels" % (x, got[has].min(), got[has].max(), has.sum()))


@pytest.mark.parametrize("x", ref.SPECIES)
def test_reference_telescoping_identity(consts, x):
    """sum_k att(k) dz_k = (1 - E(2 tau_total))/(2 eta S) for one species without molecules, from the ground and from space."""
    st = lc.one_species(x)
    nz = st["t"].shape[1]
    dz = lc.uneven_dz(nz)
    S = 31.0 + ref.SPECIES.index(x)
    cf = ref.cfg(s_ratio=[S] * 5, eta=0.45, c_mol=0.0)
    o = ref.profiles(consts, st, dz, cf)
    tau = float(o["tau_column"][0, 0])
    assert 0.05 < tau < 30.0, tau
    rhs = (1.0 - float(ref.E(2.0 * tau))) / (2.0 * 0.45 * S)
    for d in ("up", "dn"):
        lhs = float(np.sum(o["att_" + d][0] * dz))
        assert abs(lhs - rhs) <= 16 * nz * np.spacing(rhs), (d, lhs, rhs)
    assert o["tau_up"][0, 0] == 0.0 and o["tau_dn"][0, -1] == 0.0
    assert o["tau_up"][0, -1] + o["dtau"][0, -1] == pytest.approx(tau, rel=1e-14)


def test_reference_g_against_expm1():
    x = np.concatenate([np.logspace(-300, 3, 6061), [0.0, 5e-324, 1e-310, 0.9999999999, 1.0, 1.0000000001, 699.99, 700.0, 700.01]])
    got = ref.g(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(x > 0, -np.expm1(-x) / np.where(x > 0, x, 1.0), 1.0)
    err = np.abs(got - want) / np.spacing(want)
    print("g: max error %.2f ulp" % err.max())
    assert err.max() <= 4.0
    assert got[x == 0.0] == 1.0 and (got[x < 1e-17] == 1.0).all() and (np.diff(ref.g(np.sort(x))) <= 0).all()


def test_reference_cloud_water_depth_is_the_summarys_tau_c(consts, oracle_warm):
    st, dz, cols, tau_terms = lc.select_liquid(oracle_warm)
    assert list(cols) == [0, 2, 3, 5, 7]                                         # 1, 4 and 6 hold a clamped level
    o = ref.profiles(consts, st, dz, ref.cfg())
    mine = o["ext_c"] * dz
    nz = dz.size
    for c in cols:
        has = st["qc"][c] > ssr.R1
        assert has.sum() > 10
        assert np.abs(mine[c] - tau_terms[c])[has].max() <= (PI_GAP + 64 * ref.U) * tau_terms[c][has].max() and not mine[c][~has].any()
        a, b = math.fsum(mine[c]), math.fsum(tau_terms[c])
        assert abs(a - b) <= (PI_GAP + (64 + nz) * ref.U) * b and b > 1.0
    left_out = [c for c in range(st["t"].shape[0]) if c not in cols]
    assert all(abs(math.fsum(mine[c]) / math.fsum(tau_terms[c]) - 1) > 1e-6 for c in left_out)   # there the two differ: the clamp


def test_reference_summary_on_a_hand_built_column(consts):
    """Levels and faces of the eight numbers on the opaque column, with thresholds taken between the reference's own values."""
    st, dz = lc.opaque_column()
    o = ref.profiles(consts, st, dz, ref.cfg(eta=0.7, c_mol=1e-31))
    cf, clear = ref.with_thresholds(o, ref.cfg(eta=0.7, c_mol=1e-31), 0.3)
    assert clear
    s, k = ref.summary(o, cf)
    nz = dz.size
    two_tau = 2.0 * o["tau_up"][0]
    assert (two_tau > 700).sum() > nz // 3 and (two_tau < 700).sum() > nz // 3    # opaque about halfway up
    assert not o["att_up"][0][two_tau > 700].view(np.uint64).any() and (o["att_up"][0][two_tau < 699] > 0).all()
    assert s[0, ref.TAU_PART] == pytest.approx(float(np.sum(o["ext"] * dz)), rel=1e-14) and s[0, ref.TAU_PART] > 700
    assert 0 <= k[0, 0] and s[0, ref.Z_BASE_UP] == 200.0 * k[0, 0] and s[0, ref.Z_LOST_UP] == 200.0 * (k[0, 1] + 1)
    assert s[0, ref.Z_TOP_DN] == 200.0 * (k[0, 2] + 1) and s[0, ref.Z_LOST_DN] == 200.0 * k[0, 3] and k[0, 2] == nz - 1
    assert s[0, ref.N_UP] == (o["att_up"] >= cf["beta_detect"]).sum() > 0 and s[0, ref.N_DN] > 0
    clear_air = ref.profiles(consts, lc.empty(1, 5), np.ones(5), ref.cfg(c_mol=0.0))
    s0, _ = ref.summary(clear_air, ref.cfg(c_mol=0.0))
    assert np.isnan(s0[0, 2:6]).all() and not s0[0, [0, 1, 6, 7]].any()
