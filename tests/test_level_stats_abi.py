"""The per-level ensemble statistics (include/kidmp_stats.h, kid_amd/stats.py) without a GPU: the five symbols exist in the
built library and in the new header and kid_amd/stats.py declares them as the header has them; the workspace and chunk
functions need no context; a missing context is refused; kidmp_stats_merge against numpy and exact arithmetic; and the
Python wrapper turns wrong arguments away before the library is called."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import level_stats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_stats.h")
SYMBOLS = ("kidmp_level_stats_device", "kidmp32_level_stats_device", "kidmp_stats_workspace_bytes", "kidmp_stats_chunks",
           "kidmp_stats_merge")
MAX_NZ = 256

SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "size_t": (C.c_size_t,), "double": (C.c_double,),
           "float": (C.c_float,), "int": (C.c_int, C.c_int32)}


def _prototypes():
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of the header (the method of
    test_mirror_matches_header.py)."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", " ", text, flags=re.M)
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
    hdr = open(HEADER).read()
    assert '#include "kidmp.h"' in hdr
    for macro, value in (("MAX_FIELDS", 16), ("MAX_GROUPS", 64), ("MAX_BINS", 64), ("NMOM", 5)):
        assert re.search(r"#define KIDMP_STATS_%s\s+%d\b" % (macro, value), hdr), macro


def test_the_python_declarations_match_the_header():
    import kid_amd.stats as ks
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
    # the request structure: the members of the header, in its order, pointers where it has pointers
    body = re.search(r"typedef struct kidmp_stats_request \{(.*?)\} kidmp_stats_request;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    members = [m.strip() for m in body.split(";") if m.strip()]
    assert [re.findall(r"\w+", m)[-1] for m in members] == [n for n, _ in ks._StatsRequest._fields_]
    for m, (n, t) in zip(members, ks._StatsRequest._fields_):
        assert _is_pointer(t) if "*" in m else t in SCALARS[m.split()[0]], m


def test_the_mirror_of_kidmp_h_does_not_declare_them():
    import kid_amd.thompson as th
    assert not set(SYMBOLS) & set(th._declarations())


def test_workspace_and_chunks_need_no_context():
    from kid_amd.stats import library
    L = library()
    chunks, nbytes = L.kidmp_stats_chunks, L.kidmp_stats_workspace_bytes
    assert chunks(0) == 0 and chunks(-1) == 0 and chunks(-2 ** 40) == 0
    assert [chunks(n) for n in (1, 2, 255, 256, 257, 10 ** 5, 2 ** 39)] == [1, 2, 255, 256, 256, 256, 256]
    prev = 0
    for ncol in range(0, 900, 7):                                # monotone in ncol
        assert chunks(ncol) >= prev
        assert nbytes(ncol, 37, 3, 2, 8) >= nbytes(max(ncol - 7, 0), 37, 3, 2, 8)
        prev = chunks(ncol)
    # chunks x cells x levels x (5 doubles + nbin+3 32-bit counts), rounded up to 256
    assert nbytes(10 ** 5, 120, 16, 64, 64) == 256 * (64 * 16) * 120 * (5 * 8 + 67 * 4)
    assert nbytes(10 ** 5, 120, 1, 1, 0) == 256 * 120 * 40
    assert nbytes(3, 2, 1, 1, 1) == (3 * 2 * (40 + 16) + 255) // 256 * 256
    assert nbytes(0, 120, 1, 1, 0) == 0
    for bad in ((-1, 120, 1, 1, 0), (10, 1, 1, 1, 0), (10, MAX_NZ + 1, 1, 1, 0), (10, 120, 0, 1, 0), (10, 120, 17, 1, 0),
                (10, 120, 1, 0, 0), (10, 120, 1, 65, 0), (10, 120, 1, 1, -1), (10, 120, 1, 1, 65), (2 ** 39 + 1, 120, 1, 1, 0)):
        assert nbytes(*bad) == 0, bad
    from kid_amd import stats_chunks, stats_workspace_bytes
    assert stats_chunks(1000) == 256 and stats_workspace_bytes(1000, 120, 2, 3, 19) == nbytes(1000, 120, 2, 3, 19)


def test_entries_refuse_a_missing_context():
    from kid_amd.stats import _StatsRequest, library
    L = library()
    req = _StatsRequest()
    assert L.kidmp_level_stats_device(None, 4, 120, C.byref(req), None, None, None, 0, None) == -5       # KIDMP_ESTATE
    assert L.kidmp32_level_stats_device(None, 4, 120, C.byref(req), None, None, None, 0, None) == -5


# ---- kidmp_stats_merge against numpy ----
NCOL, NZ, NBIN = 1000, 3, 12
CUTS = (0, 1, 499, 1000)


@pytest.fixture(scope="module")
def dataset():
    rng = np.random.default_rng(20250611)
    dbz = rng.uniform(-35.3, 60.0, (NCOL, NZ))
    temp = 250.0 + 10.0 * rng.standard_normal((NCOL, NZ))
    shifted = rng.integers(-50, 51, (NCOL, NZ)).astype(np.float64) + 2.0 ** 30
    edges = np.stack([np.linspace(-35.0, 60.0, NBIN + 1), np.linspace(220.0, 280.0, NBIN + 1),
                      2.0 ** 30 + np.linspace(-48.0, 48.0, NBIN + 1)])
    dbz[5, 0], dbz[600, 0], dbz[7, 1], dbz[700, 1], dbz[0, 2] = np.nan, np.inf, -np.inf, edges[0, 3], -35.0
    group = rng.integers(-1, 4, NCOL).astype(np.int32)             # ids -1 and 3 are outside [0, 3)
    return [dbz, temp, shifted], group, edges, [-35.0, -np.inf, -np.inf]


def _merge(L, ncell, mom_a, hist_a, mom_b, hist_b):
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    a, h = mom_a.copy(), hist_a.copy()
    assert L.kidmp_stats_merge(ncell, NZ, NBIN, a.ctypes.data_as(dp), h.ctypes.data_as(lp), mom_b.ctypes.data_as(dp),
                               hist_b.ctypes.data_as(lp)) == 0
    return a, h


@pytest.mark.parametrize("cut", CUTS)
def test_merge_of_two_parts_against_the_whole(dataset, cut):
    from kid_amd.stats import library
    L = library()
    fields, group, edges, floors = dataset
    parts = [ref.reference([x[s] for x in fields], group[s], 3, edges, floors) for s in (slice(0, cut), slice(cut, NCOL))]
    mom, hist = _merge(L, 9, *parts[0], *parts[1])
    worst = ref.check(mom, hist, fields, group, 3, edges, floors)
    print("cut %d: worst mean error %.3g, worst M2 error %.3g of the bounds" % ((cut,) + worst))
    for a, b in ((0, 1), (1, 0)):                                # an empty side is the identity, bit for bit
        if parts[b][0][:, :, 0, :].sum() == 0:
            m, h = _merge(L, 9, *parts[a], *parts[b])
            assert np.array_equal(m.view(np.uint64), parts[a][0].view(np.uint64)) and np.array_equal(h, parts[a][1])
    assert (cut in (0, NCOL)) == any(p[0][:, :, 0, :].sum() == 0 for p in parts)


def test_merge_refuses_bad_arguments():
    from kid_amd.stats import library
    L = library()
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    mom, hist = np.zeros((1, 5, 2)), np.zeros((1, 2, 4), dtype=np.int64)
    m, h = mom.ctypes.data_as(dp), hist.ctypes.data_as(lp)
    assert L.kidmp_stats_merge(1, 2, 1, m, h, m, h) == 0
    assert L.kidmp_stats_merge(1, 2, 0, m, None, m, None) == 0
    for bad in ((1, 2, 1, None, h, m, h), (1, 2, 1, m, None, m, h), (1, 2, 1, m, h, m, None), (-1, 2, 1, m, h, m, h),
                (1, 0, 1, m, h, m, h), (1, 2, 65, m, h, m, h), (1, 2, -1, m, h, m, h)):
        assert L.kidmp_stats_merge(*bad) == -1, bad


def test_result_object_merges_and_takes_percentiles_on_host_tensors(dataset):
    import torch
    from kid_amd import LevelStats
    fields, group, edges, floors = dataset
    names = ("dbz", "t", "shifted")
    parts = [LevelStats(names, *[torch.from_numpy(a) for a in ref.reference([x[s] for x in fields], group[s], 3, edges, floors)],
                        edges) for s in (slice(0, 499), slice(499, NCOL))]
    whole = parts[0].merge(parts[1])
    ref.check(whole.mom.numpy(), whole.hist.numpy(), fields, group, 3, edges, floors)
    assert whole.names == names and whole.index("t") == 1
    assert np.allclose(whole.variance().numpy(), whole.m2.numpy() / whole.count.numpy())
    # the median of the T-like field from 5-K bins: within a bin of numpy's, and inside the bin that holds it
    med = whole.percentile(50.0).numpy()
    for g in range(3):
        for k in range(NZ):
            assert abs(med[g, 1, k] - np.median(fields[1][group == g, k])) < 5.0
    assert np.all(np.diff(np.stack([whole.percentile(q).numpy() for q in (0, 10, 50, 90, 100)]), axis=0) >= 0.0)
    with pytest.raises(Exception, match="merge"):
        parts[0].merge(LevelStats(names[:2], parts[1].mom[:, :2], parts[1].hist[:, :2], edges[:2]))


# ---- the wrapper refuses wrong input before the library is reached ----
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


def _wrapper_cases():
    """(name, fields, keyword arguments): each wrong in one way (and, being host tensors, on the wrong device)."""
    import torch
    n, nz = 6, 40
    good = lambda dt=torch.float64: torch.zeros(n, nz, dtype=dt)                     # noqa: E731
    e = np.linspace(0.0, 1.0, 6)
    return [
        ("host memory", {"a": good()}, {}),
        ("not a dict", [good()], {}),
        ("no field", {}, {}),
        ("17 fields", {"f%d" % i: good() for i in range(17)}, {}),
        ("numpy for a tensor", {"a": np.zeros((n, nz))}, {}),
        ("float16", {"a": good(torch.float16)}, {}),
        ("mixed dtypes", {"a": good(), "b": good(torch.float32)}, {}),
        ("one-dimensional", {"a": torch.zeros(nz, dtype=torch.float64)}, {}),
        ("shapes differ", {"a": good(), "b": torch.zeros(n, nz + 1, dtype=torch.float64)}, {}),
        ("nz = 1", {"a": torch.zeros(n, 1, dtype=torch.float64)}, {}),
        ("nz = 257", {"a": torch.zeros(n, 257, dtype=torch.float64)}, {}),
        ("levels strided", {"a": torch.zeros(n, 2 * nz, dtype=torch.float64)[:, ::2]}, {}),
        ("transposed", {"a": torch.zeros(nz, n, dtype=torch.float64).t()}, {}),
        ("rows overlap", {"a": torch.zeros(n + nz, dtype=torch.float64).as_strided((n, nz), (1, 1))}, {}),
        ("ngroup = 0", {"a": good()}, dict(ngroup=0)),
        ("ngroup = 65", {"a": good()}, dict(ngroup=65)),
        ("ngroup a float", {"a": good()}, dict(ngroup=2.0)),
        ("group dtype", {"a": good()}, dict(group=torch.zeros(n, dtype=torch.int64), ngroup=2)),
        ("group length", {"a": good()}, dict(group=torch.zeros(n + 1, dtype=torch.int32), ngroup=2)),
        ("group numpy", {"a": good()}, dict(group=np.zeros(n, dtype=np.int32), ngroup=2)),
        ("edges not a dict", {"a": good()}, dict(edges=e)),
        ("edges for an unknown field", {"a": good()}, dict(edges={"b": e})),
        ("edges missing for a field", {"a": good(), "b": good()}, dict(edges={"a": e})),
        ("edges descending", {"a": good()}, dict(edges={"a": e[::-1]})),
        ("edges repeat", {"a": good()}, dict(edges={"a": np.array([0.0, 1.0, 1.0, 2.0])})),
        ("edges with a NaN", {"a": good()}, dict(edges={"a": np.array([0.0, np.nan, 2.0])})),
        ("one edge", {"a": good()}, dict(edges={"a": np.array([0.0])})),
        ("65 bins", {"a": good()}, dict(edges={"a": np.arange(66.0)})),
        ("edges two-dimensional", {"a": good()}, dict(edges={"a": np.zeros((2, 3))})),
        ("edges of two lengths", {"a": good(), "b": good()}, dict(edges={"a": e, "b": e[:-1]})),
        ("floor not a dict", {"a": good()}, dict(floor=-35.0)),
        ("floor of an unknown field", {"a": good()}, dict(floor={"b": 0.0})),
        ("floor not a number", {"a": good()}, dict(floor={"a": "low"})),
        ("work on the host", {"a": good()}, dict(work=torch.zeros(1 << 20, dtype=torch.uint8))),
    ]


@pytest.mark.parametrize("case", _wrapper_cases(), ids=lambda c: c[0])
def test_wrapper_rejects_bad_arguments_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    from kid_amd import level_stats
    _, fields, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="level_stats") as err:
        level_stats(_bare(), fields, **kw)
    # the tensors are judged for what they are before for where they live: only these two cases end at the device check
    assert ("must be a CUDA tensor" in str(err.value)) == (case[0] in ("host memory", "work on the host")), str(err.value)
    with pytest.raises(th.KidmpError, match="level_stats"):
        _bare().level_stats(fields, **kw)
