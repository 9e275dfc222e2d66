"""The KiD adapter entries (kidmp[32]_kid_interface_*, kidmp[32]_kid_workspace_*) without a GPU: the eight symbols exist in
the built library and in include/kidmp.h, the workspace arithmetic needs no context, a missing context is refused, and the
Python wrappers turn wrong arrays away before the library is called."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = [pre + name for pre in ("kidmp", "kidmp32")
           for name in ("_kid_workspace_bytes", "_kid_workspace_offset", "_kid_interface_device", "_kid_interface_host")]
MAX_NZ = 256                                                 # KIDMP_MAX_NZ


def test_symbols_are_exported_and_declared():
    lib = os.path.join(ROOT, "kid_amd", "libkidmp.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(lib)
    hdr = open(os.path.join(ROOT, "include", "kidmp.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b(int|size_t)\s+%s\(" % name, hdr), name
    assert re.search(r"typedef struct kidmp_kid_fields\s*\{ double \*theta, \*qv, \*qc, \*qr, \*nr, \*qi, \*ni, \*qs, \*qg; \}", hdr)
    assert re.search(r"typedef struct kidmp32_kid_fields\s*\{ float  \*theta, \*qv, \*qc, \*qr, \*nr, \*qi, \*ni, \*qs, \*qg; \}", hdr)
    assert "#define KIDMP_MAX_NZ      %d" % MAX_NZ in hdr


def _stride(ncol, nz, size):
    return (ncol * nz * size + 255) // 256 * 256


@pytest.mark.parametrize("pre,size", [("kidmp", 8), ("kidmp32", 4)])
def test_workspace_bytes_and_offsets(pre, size):
    from kid_amd.thompson import load_library
    L = load_library()
    nbytes, offset = getattr(L, pre + "_kid_workspace_bytes"), getattr(L, pre + "_kid_workspace_offset")
    for ncol, nz in ((1, 2), (3, 37), (301, 120), (1023, 200), (7, MAX_NZ), (100000, 120), (5, 1)):
        assert nbytes(ncol, nz) == 15 * _stride(ncol, nz, size), (ncol, nz)
        assert nbytes(ncol, nz) % 256 == 0
        for v in range(15):
            assert offset(ncol, nz, v) == v * _stride(ncol, nz, size), (ncol, nz, v)
    assert nbytes(0, 120) == 0
    prev = 0
    for ncol in range(0, 600, 7):                            # monotone in ncol
        assert nbytes(ncol, 37) >= prev
        prev = nbytes(ncol, 37)
    for ncol, nz in ((-1, 120), (10, 0), (10, -3), (10, MAX_NZ + 1)):
        assert nbytes(ncol, nz) == 0, (ncol, nz)
        assert offset(ncol, nz, 3) == 0, (ncol, nz)
    assert offset(10, 120, -1) == 0 and offset(10, 120, 15) == 0


def test_python_workspace_bytes_agree():
    import torch
    from kid_amd import ThompsonMP
    assert ThompsonMP.kid_workspace_bytes(301, 120, np.float64) == 15 * _stride(301, 120, 8)
    assert ThompsonMP.kid_workspace_bytes(301, 37, torch.float32) == 15 * _stride(301, 37, 4)


def test_entries_refuse_a_missing_context():
    """No device is needed to be told that there is no context."""
    from kid_amd.thompson import load_library
    L = load_library()
    head = [None, 4, 120, 10.0, 1.0e5, 0.2856] + [None] * 10
    assert L.kidmp_kid_interface_device(*head, None, 0, None) == -5            # KIDMP_ESTATE
    assert L.kidmp_kid_interface_host(*head) == -5
    assert L.kidmp32_kid_interface_device(*head, 0, None, 0, None) == -5
    assert L.kidmp32_kid_interface_host(*head, 0) == -5


class _NoLibrary:
    """Stands where the library would: the wrapper must raise before it reaches for it."""

    def __getattr__(self, name):
        raise AssertionError("the library was called")


def _bare(iiwarm=True):
    from kid_amd import ThompsonMP
    m = ThompsonMP.__new__(ThompsonMP)                      # no kidmp_init: there is no device here
    m._h = None
    m.device = 0
    m.iiwarm = iiwarm
    return m


NCOL, NZ = 6, 40
WARM = ("theta", "qv", "qc", "qr", "nr")
FROZEN = ("qi", "ni", "qs", "qg")


def _good(dtype=np.float64, keys=WARM):
    st = {k: np.zeros((NCOL, NZ), dtype=dtype) for k in keys}
    return st, np.ones((NCOL, NZ), dtype=dtype), np.full(NZ, 25.0, dtype=dtype)


def _host_cases():
    """(name, iiwarm, state, exner, dz, keyword arguments) -- each wrong in exactly one way."""
    out = []
    st, ex, dz = _good()
    out.append(("dtype of a member", True, dict(st, qc=st["qc"].astype(np.float32)), ex, dz, {}))
    out.append(("shape of a member", True, dict(st, qr=np.zeros((NCOL, NZ + 1))), ex, dz, {}))
    out.append(("stride of a member", True, dict(st, nr=np.zeros((NCOL, 2 * NZ))[:, ::2]), ex, dz, {}))
    out.append(("Fortran order", True, dict(st, qv=np.asfortranarray(np.zeros((NCOL, NZ)))), ex, dz, {}))
    out.append(("missing member", True, {k: v for k, v in st.items() if k != "nr"}, ex, dz, {}))
    out.append(("unknown member", True, dict(st, qh=np.zeros((NCOL, NZ))), ex, dz, {}))
    out.append(("list for an array", True, dict(st, qc=[[0.0] * NZ] * NCOL), ex, dz, {}))
    out.append(("theta one-dimensional", True, dict(st, theta=np.zeros(NZ)), ex, dz, {}))
    out.append(("integer theta", True, dict(st, theta=np.zeros((NCOL, NZ), dtype=np.int64)), ex, dz, {}))
    out.append(("state not a dict", True, [st["theta"]], ex, dz, {}))
    out.append(("exner shape", True, st, ex[:-1], dz, {}))
    out.append(("exner dtype", True, st, ex.astype(np.float32), dz, {}))
    out.append(("dz two-dimensional", True, st, ex, np.full((NCOL, NZ), 25.0), {}))
    out.append(("dz length", True, st, ex, dz[:-1], {}))
    out.append(("adv member dtype", True, st, ex, dz, dict(adv={"theta": np.zeros((NCOL, NZ), dtype=np.float32)})))
    out.append(("div member shape", True, st, ex, dz, dict(div={"qv": np.zeros((NCOL + 1, NZ))})))
    out.append(("adv not a dict", True, st, ex, dz, dict(adv=np.zeros((NCOL, NZ)))))
    out.append(("arith with float64", True, st, ex, dz, dict(arith="p32n")))
    out.append(("mixed phase without qi", False, st, ex, dz, {}))
    st32, ex32, dz32 = _good(np.float32)
    out.append(("unknown arith", True, st32, ex32, dz32, dict(arith="bf16")))
    return out


@pytest.mark.parametrize("case", _host_cases(), ids=lambda c: c[0])
def test_host_wrapper_rejects_bad_arrays_before_the_library(case, monkeypatch):
    import kid_amd.thompson as th
    _, iiwarm, st, ex, dz, kw = case
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="kid_interface_host"):
        _bare(iiwarm).kid_interface_host(st, 10.0, 1.0e5, 0.2856, ex, dz, **kw)


def test_host_wrapper_ignores_frozen_members_in_a_warm_context(monkeypatch):
    """In an iiwarm context the frozen members are not looked at: a wrong one does not stop the call before the library."""
    import kid_amd.thompson as th
    st, ex, dz = _good()
    st["qi"] = np.zeros(3, dtype=np.float32)
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(AssertionError, match="the library was called"):
        _bare(True).kid_interface_host(st, 10.0, 1.0e5, 0.2856, ex, dz)


def test_device_wrapper_rejects_bad_tensors_before_the_library(monkeypatch):
    """Host tensors stand for 'wrong device' here; dtype, shape and stride are judged before the device is."""
    import torch
    import kid_amd.thompson as th
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    st = {k: torch.zeros(NCOL, NZ, dtype=torch.float64) for k in WARM}
    ex, dz = torch.ones(NCOL, NZ, dtype=torch.float64), torch.full((NZ,), 25.0, dtype=torch.float64)
    bad = [
        (st, ex, dz, {}),                                                                    # host memory
        (dict(st, theta=torch.zeros(NCOL, NZ, dtype=torch.float16)), ex, dz, {}),
        (dict(st, theta=torch.zeros(NZ, dtype=torch.float64)), ex, dz, {}),
        (dict(st, theta=np.zeros((NCOL, NZ))), ex, dz, {}),                                  # numpy where a tensor belongs
        ({k: v for k, v in st.items() if k != "qc"}, ex, dz, {}),
        (st, ex, dz, dict(arith="f32")),
        (st, ex, dz, dict(adv=[ex])),
    ]
    for s, e, d, kw in bad:
        with pytest.raises(th.KidmpError, match="kid_interface"):
            _bare().kid_interface(s, 10.0, 1.0e5, 0.2856, e, d, **kw)
