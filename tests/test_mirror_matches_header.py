"""The ctypes declarations of the Python mirror (kid_amd/thompson.py, load_library) against the prototypes of
include/kidmp.h: the same entries, the same number of arguments, the same scalar types.  A disagreement would otherwise
show only as a fault on the GPU.  No library and no device: a stub stands where the shared object would be loaded."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kidmp.h")

SCALARS = {"int64_t": (C.c_int64,), "int32_t": (C.c_int32,), "size_t": (C.c_size_t,), "double": (C.c_double,),
           "float": (C.c_float,), "int": (C.c_int, C.c_int32)}


def _prototypes():
    """name -> (return type, [parameter, ...]) of every `type kidmp[32]_name(params);` of the header."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[^\n]*(\\\n[^\n]*)*", " ", text, flags=re.M)         # preprocessor lines
    out = {}
    for ret, name, params in re.findall(r"([\w \t\n\*]+?)\b(kidmp(?:32)?_\w+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        out[name] = (" ".join(ret.split()), [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    return out


class _Entry:
    restype = "never set"
    argtypes = None


class _Stub:
    """What ctypes.CDLL would return, remembering every entry the mirror reaches for."""

    def __init__(self, path):
        self._name = path
        self.entries = {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self.entries.setdefault(name, _Entry())


@pytest.fixture(scope="module")
def declared():
    try:
        import torch  # noqa: F401      (load_library imports it, and it loads libraries of its own through ctypes.CDLL)
    except ImportError:
        pass
    import kid_amd.thompson as th
    saved, cdll = th._lib, th.C.CDLL
    th._lib, th.C.CDLL = None, _Stub
    try:
        return th.load_library(HEADER).entries              # any file that exists: the stub does not open it
    finally:
        th._lib, th.C.CDLL = saved, cdll


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_the_header_has_the_prototypes_this_test_was_written_for():
    assert len(_prototypes()) == 67


def test_every_prototype_is_declared_with_its_argument_count_and_types(declared):
    wrong = []
    for name, (ret, params) in sorted(_prototypes().items()):
        e = declared.get(name)
        if e is None or e.argtypes is None:
            wrong.append("%s: not declared" % name)
            continue
        if len(e.argtypes) != len(params):
            wrong.append("%s: %d arguments declared, the header has %d" % (name, len(e.argtypes), len(params)))
            continue
        for i, (p, t) in enumerate(zip(params, e.argtypes)):
            if "*" in p:
                ok = _is_pointer(t)
            else:
                ctype = re.sub(r"\bconst\b", "", p).split()[0]
                ok = t in SCALARS[ctype]
            if not ok:
                wrong.append("%s: argument %d is `%s`, declared %s" % (name, i, p, getattr(t, "__name__", t)))
        if "*" in ret:
            ok = e.restype in (C.c_void_p, C.c_char_p)
        elif ret == "void":
            ok = e.restype is None
        else:
            ok = e.restype in SCALARS[ret]
        if not ok:
            wrong.append("%s: returns `%s`, declared %s" % (name, ret, getattr(e.restype, "__name__", e.restype)))
    assert not wrong, "\n".join(wrong)


def test_nothing_is_declared_that_the_header_lacks(declared):
    assert sorted(set(declared) - set(_prototypes())) == []
