"""The range-height scan (include/kidmp_scan.h, kid_amd/scan.py) without a GPU: the entries exist in the built library and
in the header, kid_amd/scan.py declares them as the header has them, the header compiles as C99 and C++11, a missing
context is refused, rhi_rays gives the stated rows, the wrapper refuses wrong input before the library is reached, and the
geometry of kid_amd/csrc/kidmp_scan_geom.h -- the classification that guards every gather of the kernel -- runs as a host
program of its own, with and without ASan + UBSan, and equals tests/scan_ref.py's (i, k, h) to the bit on the covering
cases of tests/scan_cases.py.  Nothing is loaded into Python under a sanitizer.
"""
import ctypes as C
import importlib
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import scan_cases as cases
import scan_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp_scan.h")
CSRC = os.path.join(ROOT, "kid_amd", "csrc")
SYMBOLS = ("kidmp_scan_device", "kidmp32_scan_device")
SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "double": (C.c_double,), "float": (C.c_float,), "int": (C.c_int, C.c_int32),
           "void": (None,)}
EINVAL, ESTATE = -1, -5


def _ks():
    return importlib.import_module("kid_amd.scan")             # kid_amd.scan, the attribute, is the function


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
    assert '#include "kidmp.h"' in open(HEADER).read()
    assert "project's own" in open(HEADER).read().lower() and "unpinned" in open(HEADER).read()


def test_the_python_declarations_match_the_header():
    import kid_amd
    ks = _ks()
    declared = ks.declare(_Stub()).entries
    protos = _prototypes()
    assert sorted(declared) == sorted(protos) == sorted(ks._declarations())
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
    for struct, elem in (("kidmp_scan_out", "double"), ("kidmp32_scan_out", "float")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _code(), re.S).group(1)
        assert body.split()[0] == elem
        members = [m.strip().lstrip("*") for m in re.sub(r"\b(%s|int32_t)\b" % elem, "", body).replace(";", ",").split(",") if m.strip()]
        assert tuple(members) == ks.SCAN_NAMES == kid_amd.SCAN_NAMES == ref.NAMES
        assert re.search(r"int32_t \*cell;", body)
    assert [n for n, _ in ks._ScanOut._fields_] == list(ks.SCAN_NAMES) and all(t is C.c_void_p for _, t in ks._ScanOut._fields_)
    cfg = re.search(r"typedef struct kidmp_scan_cfg \{(.*?)\} kidmp_scan_cfg;", _code(), re.S).group(1)
    fields = []
    for decl in cfg.split(";"):
        if decl.strip():
            t, names = decl.split(None, 1)
            fields += [(n.strip(), {"double": C.c_double, "int32_t": C.c_int32}[t]) for n in names.split(",")]
    assert fields == list(ks._ScanCfg._fields_)
    assert [n for n, _ in fields] == ["r0", "dr", "ngate", "nsub", "half_inv_ae", "periodic", "missing"]
    raw = open(HEADER).read()
    assert int(re.search(r"#define KIDMP_SCAN_MAX_GATES (\d+)", raw).group(1)) == ks.SCAN_MAX_GATES == 1024
    assert int(re.search(r"#define KIDMP_SCAN_MAX_SUB (\d+)", raw).group(1)) == ks.SCAN_MAX_SUB == 9
    assert kid_amd.scan is ks.scan and kid_amd.rhi_rays is ks.rhi_rays and kid_amd.ScanCfg is ks.ScanCfg
    assert callable(kid_amd.ThompsonMP.scan)


def test_only_the_scan_mirror_declares_them():
    import kid_amd.mie as km
    import kid_amd.slab as sl
    import kid_amd.thompson as th
    for other in (th, km, sl):
        assert not set(SYMBOLS) & set(other._declarations())


@pytest.mark.parametrize("compiler, flags", [("gcc", ["-std=c99", "-x", "c"]), ("g++", ["-std=c++11", "-x", "c++"])])
def test_header_compiles_strictly(tmp_path, compiler, flags):
    cc = shutil.which(compiler)
    assert cc, compiler
    src = tmp_path / ("use" + (".c" if compiler == "gcc" else ".cpp"))
    src.write_text('#include "kidmp_scan.h"\n'
                   "int use(kidmp_ctx *c, const double *a, const float *b, kidmp_scan_cfg *f, kidmp_scan_out *o, kidmp32_scan_out *p)\n"
                   "{ f->ngate = KIDMP_SCAN_MAX_GATES; f->nsub = KIDMP_SCAN_MAX_SUB; f->r0 = 0.0; f->dr = 60.0; f->half_inv_ae = 0.0;\n"
                   "  f->periodic = 1; f->missing = -999.0; o->cell = p->cell;\n"
                   "  if (kidmp_scan_device(c, 1, 8, 16, 100.0, a, a, a, a, 0, a, a, 4, f, o, 0)) return 1;\n"
                   "  return kidmp32_scan_device(c, 1, 8, 16, 100.0, b, b, b, b, 1, a, a, 4, f, p, 0); }\n")
    subprocess.run([cc] + flags + ["-pedantic-errors", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "use.o")], check=True)


def test_entries_refuse_a_missing_context():
    ks = _ks()
    L = ks.library()
    o, c = ks._ScanOut(), ks._ScanCfg(0.0, 60.0, 8, 1, 0.0, 0, float("nan"))
    args = [None, 1, 8, 16, 100.0, None, None, None, None, 0, None, None, 4, C.byref(c), C.byref(o), None]
    assert L.kidmp_scan_device(*args) == ESTATE and L.kidmp32_scan_device(*args) == ESTATE
    assert L.kidmp_last_error(None)


def test_rhi_rays_gives_the_stated_rows():
    from kid_amd import KidmpError, rhi_rays
    r = rhi_rays(1, 250.0, 12.5, [0.5, 30.0, 90.0, 150.0, 180.0, 0.0])
    assert r.shape == (6, 6) and r.dtype == np.float64 and r.flags.c_contiguous
    assert (r[:, 0] == 1.0).all() and (r[:, 1] == 250.0).all() and (r[:, 2] == 12.5).all() and (r[:, 5] == 1.0).all()
    assert (r[2, 3], r[2, 4]) == (0.0, 1.0) and (r[4, 3], r[4, 4]) == (-1.0, 0.0) and (r[5, 3], r[5, 4]) == (1.0, 0.0)
    for row, el in zip(r, (0.5, 30.0)):
        assert row[3] == np.cos(np.deg2rad(el)) and row[4] == np.sin(np.deg2rad(el))
    assert r[3, 3] < 0.0 < r[3, 4]
    assert rhi_rays(0, 0.0, 0.0, 45.0).shape == (1, 6)
    for nsub in (2, 3, 5, 9):
        bw = 1.2
        b = rhi_rays(0, 0.0, 0.0, [10.0, 90.0], bw, nsub).reshape(2, nsub, 6)
        delta = bw * (2.0 * np.arange(nsub) / (nsub - 1) - 1.0)
        w = np.exp(-8.0 * math.log(2.0) * (delta / bw) ** 2)
        w = w / w.sum()
        assert np.array_equal(b[0, :, 5], w) and np.array_equal(b[1, :, 5], w) and abs(b[0, :, 5].sum() - 1.0) < 4e-16
        assert np.array_equal(b[0, :, 3], np.cos(np.deg2rad(10.0 + delta))) and np.array_equal(b[0, :, 4], np.sin(np.deg2rad(10.0 + delta)))
        assert delta[0] == -bw and delta[-1] == bw and np.allclose(np.diff(delta), 2.0 * bw / (nsub - 1), rtol=1e-14)
        if nsub % 2:
            assert (b[1, nsub // 2, 3], b[1, nsub // 2, 4]) == (0.0, 1.0)      # the centre sub-ray of the vertical beam
            assert b[0, nsub // 2, 5] == b[0, :, 5].max()
    for kw in (dict(nsub=0), dict(nsub=10), dict(nsub=2.5), dict(nsub=3), dict(nsub=3, beamwidth_deg=-1.0), dict(beamwidth_deg=float("nan"))):
        with pytest.raises(KidmpError, match="rhi_rays"):
            rhi_rays(0, 0.0, 0.0, [1.0], **kw)
    with pytest.raises(KidmpError, match="rhi_rays"):
        rhi_rays(0, 0.0, 0.0, [1.0, float("inf")])
    with pytest.raises(KidmpError, match="rhi_rays"):
        rhi_rays(-1, 0.0, 0.0, [1.0])


def _write_cases(path, cs):
    h = lambda v: float(v).hex()   # noqa: E731
    with open(path, "w") as f:
        f.write("%d\n" % len(cs))
        for c in cs:
            f.write("%d %d %d %d %d %d %s %s %s %s\n" % (c["nz"], c["nx"], c["nslab"], c["ngate"], c["periodic"], len(c["rays"]), h(c["r0"]),
                                                         h(c["dr"]), h(c["dx"]), h(c["half_inv_ae"])))
            f.write(" ".join(h(z) for z in c["zf"]) + "\n")
            for row in c["rays"]:
                f.write(" ".join(h(w) for w in row) + "\n")


def test_geometry_under_sanitizers_equals_the_reference(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    # the sanitizers' runtimes are linked statically: the program is instrumented by itself and runs in the environment as it is
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else ["-static-libsan"]
    common = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
              os.path.join(ROOT, "tests", "native", "scan_geom_check.cpp")]
    san, plain = tmp_path / "scan_san", tmp_path / "scan_plain"
    subprocess.run(common + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + static
                   + ["-o", str(san)], check=True)
    subprocess.run(common + ["-o", str(plain)], check=True)
    cs = cases.covering()
    _write_cases(tmp_path / "cases.txt", cs)
    a = subprocess.run([str(san), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    b = subprocess.run([str(plain), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert a.returncode == 0 and a.stdout.strip().endswith("scan ok") and "runtime error" not in a.stderr and "Sanitizer" not in a.stderr, \
        a.stdout[-2000:] + a.stderr
    assert b.returncode == 0 and a.stdout == b.stdout
    lines = iter(b.stdout.splitlines())
    seen = dict(inside=0, outside=0, wrapped=0, negative=0)
    for n, c in enumerate(cs):
        assert next(lines) == "c %d" % n
        valid, inside, i, k, h = cases.reference(c)
        for r in range(len(c["rays"])):
            assert next(lines) == "r %d" % valid[r], (c["name"], r)
            for g in range(c["ngate"]):
                tag, gi, gk, gin, gh = next(lines).split()
                gh = float.fromhex(gh) if "n" not in gh else float(gh)      # nan, -nan, inf
                assert tag == "g" and (int(gi), int(gk), int(gin)) == (i[r, g], k[r, g], inside[r, g]), (c["name"], r, g)
                assert (math.isnan(gh) and math.isnan(h[r, g])) or ref.bits(np.float64(gh))[()] == ref.bits(h[r, g])[()], (c["name"], r, g)
        seen["inside"] += int(inside.sum())
        seen["outside"] += int((~inside).sum())
    assert next(lines) == "scan ok"
    assert seen["inside"] > 10000 and seen["outside"] > 10000
    # the face case by hand: gate g sits on face 2g + 1 and belongs to level 2g + 1; x0 = 2 dx belongs to cell 2, x0 = 0 to
    # cell 0, x0 = nx dx to no cell; the beam leaves through the top after 20 gates
    face = cs[-1]
    valid, inside, i, k, h = cases.reference(face)
    assert face["name"] == "on-the-face" and valid.all()
    assert np.array_equal(k[0, :20], 2 * np.arange(20) + 1) and (k[0, 20:] == -1).all() and (i[0, :20] == 2).all()
    assert (i[1, :20] == 0).all() and not inside[2].any() and np.array_equal(h[0], 125.0 + 250.0 * np.arange(24))


def test_the_reference_wraps_negative_positions():
    """At 150 degrees x is negative: floor and the periodic wrap act on negative numbers, and without the wrap the beam is
    outside from the first gate that crosses x = 0."""
    c = cases.case(64, 7, 130, 1, 0)
    valid, inside, i, k, h = cases.reference(c)
    back = 3                                                       # slab 0 at 150 degrees
    x = c["rays"][back, 1] + (c["r0"] + (np.arange(130) + 0.5) * c["dr"]) * c["rays"][back, 3]
    assert (x < 0).sum() > 50 and inside[back][(x < 0) & (h[back] < c["zf"][-1])].all()
    assert np.array_equal(i[back][inside[back]], np.mod(np.floor(x / c["dx"]).astype(np.int64), 7)[inside[back]])
    c0 = cases.case(64, 7, 130, 0, 0)
    assert not cases.reference(c0)[1][back][x < 0].any() and cases.reference(c0)[1][back][x >= 0].all()


# ---- the wrapper refuses wrong input before the library is reached ----
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called")


def test_wrapper_rejects_bad_arguments_before_the_library(monkeypatch):
    import torch
    import kid_amd.thompson as th
    from kid_amd import ScanCfg, ThompsonMP
    m = ThompsonMP.__new__(ThompsonMP)                      # no kidmp_init: there is no device here
    m._h, m.device, m.iiwarm = None, 0, False
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    f = {"dbz": torch.zeros(16, 12, dtype=torch.float64)}   # host memory: refused at the first tensor at the latest
    zf, rays = torch.zeros(13, dtype=torch.float64), torch.zeros(4, 6, dtype=torch.float64)
    good = ScanCfg(dr=60.0, ngate=32)
    nan, inf = float("nan"), float("inf")
    calls = [dict(fields=[f["dbz"]]), dict(fields={"dbz": np.zeros((16, 12))}), dict(fields=dict(f, qr=f["dbz"])), dict(nx=0), dict(nx=5),
             dict(nx=4.0), dict(dx=0.0), dict(dx=inf), dict(dx="wide"), dict(cfg=None), dict(cfg=ScanCfg(ngate=0)), dict(cfg=ScanCfg(ngate=1025)),
             dict(cfg=ScanCfg(nsub=10)), dict(cfg=ScanCfg(nsub=0)), dict(cfg=ScanCfg(dr=0.0)), dict(cfg=ScanCfg(dr=nan)), dict(cfg=ScanCfg(r0=-1.0)),
             dict(cfg=ScanCfg(half_inv_ae=inf)), dict(cfg=ScanCfg(ngate=2.5)), dict(want=()), dict(want=("dbz", "dbz")), dict(want=("zdr",)),
             dict(want=3), dict()]
    for kw in calls:
        args = dict(fields=f, zf=zf, rays=rays, dx=100.0, nx=4, cfg=good, want=("dbz",))
        args.update(kw)
        with pytest.raises(th.KidmpError, match="scan"):
            m.scan(**args)
