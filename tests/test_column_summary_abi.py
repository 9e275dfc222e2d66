"""The per-column summary (include/kidmp_summary.h, kid_amd/summary.py) without a GPU: the four symbols exist in the built
library and in the new header, kid_amd/summary.py declares them as the header has them, the macros and enum values are
right, a missing context is refused, the Python wrappers turn wrong arguments away before the library is called, and the
numpy reference of the GPU tests gives the known answers of hand-built columns."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import column_summary_ref as ref
import refl_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_summary.h")
SYMBOLS = ("kidmp_column_summary_device", "kidmp32_column_summary_device", "kidmp_column_summary_host",
           "kidmp32_column_summary_host")
ENUM = ("WVP", "CWP", "RWP", "IWP", "SWP", "GWP", "TAU_C", "DBZ_MAX", "Z_DBZ_MAX", "Z_ECHO_TOP", "DBZ_SFC", "Z_CLOUD_BASE",
        "Z_CLOUD_TOP", "N_CLOUD", "Z_FREEZE")

SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "size_t": (C.c_size_t,), "double": (C.c_double,),
           "float": (C.c_float,), "int": (C.c_int, C.c_int32)}


def _code():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _prototypes():
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of the header (the method of
    test_level_stats_abi.py)."""
    text = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", " ", _code(), flags=re.M)
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


def test_macros_and_enum_values():
    import kid_amd
    code = _code()
    assert re.search(r"#define KIDMP_SUMMARY_N\s+16\b", code)
    body = re.search(r"enum\s*\{(.*?)\}\s*;", code, re.S).group(1)
    names = [" ".join(x.split()) for x in body.split(",")]
    assert names[0] == "KIDMP_SUM_WVP = 0"                                     # the rest count up from it
    assert [names[0].split()[0]] + names[1:] == ["KIDMP_SUM_" + n for n in ENUM]
    assert kid_amd.SUMMARY_NAMES == tuple(n.lower() for n in ENUM) == ref.NAMES
    assert kid_amd.SUMMARY_INPUTS == ("t", "p", "qv", "qc", "nc", "qi", "qr", "nr", "qs", "qg") == ref.INPUTS
    assert re.search(r"NULL cfg means \{ 18\.0, 1\.0e-5, 273\.15 \}", open(HEADER).read())
    import kid_amd.summary as ks
    assert ks.DEFAULT_CFG == ref.DEFAULT_CFG == (18.0, 1.0e-5, 273.15) and ks.SUMMARY_N == ref.N == 16


def test_the_python_declarations_match_the_header():
    import kid_amd.summary as ks
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
    body = re.search(r"typedef struct kidmp_summary_cfg \{(.*?)\} kidmp_summary_cfg;", _code(), re.S).group(1)
    members = [m.strip() for m in body.replace("double", "").replace(";", "").split(",")]
    assert members == [n for n, _ in ks._SummaryCfg._fields_] and all(t is C.c_double for _, t in ks._SummaryCfg._fields_)


def test_the_other_mirrors_do_not_declare_them():
    import kid_amd.stats as st
    import kid_amd.thompson as th
    assert not set(SYMBOLS) & set(th._declarations()) and not set(SYMBOLS) & set(st._declarations())


def test_entries_refuse_a_missing_context():
    from kid_amd.summary import library
    L = library()
    args = [None, 4, 120] + [None] * 11 + [0, None, None]
    assert L.kidmp_column_summary_host(*args) == -5                              # KIDMP_ESTATE
    assert L.kidmp32_column_summary_host(*args) == -5
    assert L.kidmp_column_summary_device(*args, None) == -5
    assert L.kidmp32_column_summary_device(*args, None) == -5


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


def _host_state(dtype=np.float64):
    return {k: np.zeros((N, NZ), dtype=dtype) for k in ref.INPUTS}


def _host_cases():
    good, dz = _host_state, np.ones(NZ)
    return [
        ("not a dict", [np.zeros((N, NZ))], dz, {}),
        ("torch for numpy", {k: __import__("torch").zeros(N, NZ, dtype=__import__("torch").float64) for k in ref.INPUTS}, dz, {}),
        ("float16", _host_state(np.float16), dz.astype(np.float16), {}),
        ("one-dimensional", {k: np.zeros(NZ) for k in ref.INPUTS}, dz, {}),
        ("nz = 1", {k: np.zeros((N, 1)) for k in ref.INPUTS}, np.ones(1), {}),
        ("nz = 257", {k: np.zeros((N, 257)) for k in ref.INPUTS}, np.ones(257), {}),
        ("qr missing", {k: v for k, v in good().items() if k != "qr"}, dz, {}),
        ("mixed dtypes", dict(good(), qc=np.zeros((N, NZ), dtype=np.float32)), dz, {}),
        ("shapes differ", dict(good(), qr=np.zeros((N, NZ + 1))), dz, {}),
        ("not contiguous", dict(good(), p=np.zeros((NZ, N)).T), dz, {}),
        ("dz dtype", good(), dz.astype(np.float32), {}),
        ("dz length", good(), np.ones(NZ + 1), {}),
        ("dz shape", good(), np.ones((N + 1, NZ)), {}),
        ("dz a list", good(), [1.0] * NZ, {}),
        ("dz strided", good(), np.ones((N, 2 * NZ))[:, ::2], {}),
        ("cfg of two", good(), dz, dict(cfg=(18.0, 1e-5))),
        ("cfg with a NaN", good(), dz, dict(cfg=(np.nan, 1e-5, 273.15))),
        ("cfg infinite", good(), dz, dict(cfg={"dbz_echo": np.inf})),
        ("cfg unknown key", good(), dz, dict(cfg={"echo": 18.0})),
        ("cfg a string", good(), dz, dict(cfg="default")),
    ]


@pytest.mark.parametrize("case", _host_cases(), ids=lambda c: c[0])
def test_host_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import column_summary_host
    _, st, dz, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="column_summary_host"):
        column_summary_host(_bare(), st, dz, **kw)
    with pytest.raises(th.KidmpError, match="column_summary_host"):
        _bare().column_summary_host(st, dz, **kw)


def _device_cases():
    """Host tensors throughout: each case is wrong in one way and, being host memory, on the wrong device as well."""
    import torch
    good = lambda dt=torch.float64: {k: torch.zeros(N, NZ, dtype=dt) for k in ref.INPUTS}   # noqa: E731
    dz = torch.ones(NZ, dtype=torch.float64)
    return [
        ("host memory", good(), dz, {}),
        ("numpy for torch", _host_state(), np.ones(NZ), {}),
        ("float16", good(torch.float16), dz.to(torch.float16), {}),
        ("nz = 257", {k: torch.zeros(N, 257, dtype=torch.float64) for k in ref.INPUTS}, torch.ones(257, dtype=torch.float64), {}),
        ("t missing", {k: v for k, v in good().items() if k != "t"}, dz, {}),
        ("dz numpy", good(), np.ones(NZ), {}),
        ("dz shape", good(), torch.ones(NZ + 1, dtype=torch.float64), {}),
        ("cfg with a NaN", good(), dz, dict(cfg=(18.0, float("nan"), 273.15))),
        ("out numpy", good(), dz, dict(out=np.zeros((N, 16)))),
    ]


@pytest.mark.parametrize("case", _device_cases(), ids=lambda c: c[0])
def test_device_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import column_summary
    _, st, dz, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="column_summary"):
        column_summary(_bare(), st, dz, **kw)
    with pytest.raises(th.KidmpError, match="column_summary"):
        _bare().column_summary(st, dz, **kw)


# ---- the numpy reference on hand-built columns with known answers ----
def _hand_state(nz=40):
    st = {k: np.zeros((1, nz)) for k in ref.INPUTS}
    st["t"][:], st["p"][:], st["qv"][:] = 285.0, 9.0e4, 5.0e-3
    return st


def test_reference_cloud_layer_in_levels_10_to_19():
    nz = 40
    st = _hand_state(nz)
    st["qc"][0, 10:20] = 5.0e-4
    dz = 20.0 * 1.05 ** np.arange(nz)                                            # uneven
    dbz = np.full((1, nz), ro.EMPTY_DBZ)
    re = np.where(st["qc"] > 0, 10.0e-6, ref.RE_QC_PRESET)
    out, mag, k = ref.summary(st, dz, dbz, re, re != ref.RE_QC_PRESET)
    rho = 0.622 * 9.0e4 / (287.04 * 285.0 * (5.0e-3 + 0.622))
    assert out[0, ref.Z_CLOUD_BASE] == pytest.approx(dz[:10].sum(), rel=1e-14)
    assert out[0, ref.Z_CLOUD_TOP] == pytest.approx(dz[:20].sum(), rel=1e-14)
    assert out[0, ref.N_CLOUD] == 10.0
    assert out[0, ref.CWP] == pytest.approx(rho * 5.0e-4 * dz[10:20].sum(), rel=1e-13)
    assert out[0, ref.WVP] == pytest.approx(rho * 5.0e-3 * dz.sum(), rel=1e-13)
    assert out[0, ref.TAU_C] == pytest.approx(1.5 * out[0, ref.CWP] / (1000.0 * 10.0e-6), rel=1e-13)
    assert mag[0, ref.CWP] == out[0, ref.CWP] and mag[0, ref.Z_FREEZE] == pytest.approx(dz.sum(), rel=1e-14)
    assert list(out[0, [ref.RWP, ref.IWP, ref.SWP, ref.GWP]]) == [0.0] * 4
    assert np.isnan(out[0, ref.Z_FREEZE]) and list(k[0]) == [0, -1, 10, 19, -1]   # 285 K everywhere


def test_reference_empty_column():
    nz = 40
    st = _hand_state(nz)
    dz = np.full(nz, 25.0)
    dbz = np.full((1, nz), ro.EMPTY_DBZ)
    re = np.full((1, nz), ref.RE_QC_PRESET)
    out, _, k = ref.summary(st, dz, dbz, re, re != ref.RE_QC_PRESET)
    assert np.isnan(out[0, [ref.Z_ECHO_TOP, ref.Z_CLOUD_BASE, ref.Z_CLOUD_TOP]]).all()
    assert out[0, ref.DBZ_MAX] == ro.EMPTY_DBZ == out[0, ref.DBZ_SFC]
    assert out[0, ref.Z_DBZ_MAX] == 12.5 and out[0, ref.N_CLOUD] == 0.0 and out[0, ref.TAU_C] == 0.0
    assert not ref.undecidable(dbz)[0]                                           # empty: level 0 by convention


def test_reference_echo_top_and_freezing_level():
    nz = 40
    st = _hand_state(nz)
    st["t"][0] = 290.0 - 1.0 * np.arange(nz)                                     # 273.15 K is crossed between levels 16 and 17
    dz = np.full(nz, 100.0)
    dbz = np.full((1, nz), ro.EMPTY_DBZ)
    dbz[0, 3:9] = [20.0, 35.0, 41.0, 41.0, 18.0, 17.9]
    re = np.full((1, nz), ref.RE_QC_PRESET)
    out, _, k = ref.summary(st, dz, dbz, re, re != ref.RE_QC_PRESET)
    assert list(k[0]) == [5, 7, -1, -1, 17]                                      # the lowest of the two 41s; 18.0 >= 18
    assert out[0, ref.Z_DBZ_MAX] == 550.0 and out[0, ref.Z_ECHO_TOP] == 800.0 and out[0, ref.Z_FREEZE] == 1750.0
    assert ref.undecidable(dbz)[0]                                               # a tie at the top and a level on the threshold
