"""The per-column droplet number (kidmp_set_column_nc) without a GPU: the two entries exist in the built library and in
include/kidmp.h, and the Python wrapper turns wrong shapes and dtypes away before the library is called."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_declared():
    lib = os.path.join(ROOT, "kid_amd", "libkidmp.so")
    assert os.path.exists(lib), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = C.CDLL(lib)
    hdr = open(os.path.join(ROOT, "include", "kidmp.h")).read()
    for name in ("kidmp_set_column_nc", "kidmp_column_nc_count"):
        assert hasattr(L, name), name
    assert re.search(r"\bint\s+kidmp_set_column_nc\(kidmp_ctx \*ctx, int64_t ncol, const double \*set_nc\);", hdr)
    assert re.search(r"\bint64_t\s+kidmp_column_nc_count\(const kidmp_ctx \*ctx\);", hdr)


def test_entries_refuse_a_missing_context():
    """No device is needed to be told that there is no context."""
    from kid_amd.thompson import load_library
    L = load_library()
    v = np.array([100.0])
    assert L.kidmp_set_column_nc(None, 1, v.ctypes.data) == -5           # KIDMP_ESTATE
    assert L.kidmp_column_nc_count(None) == 0


class _NoLibrary:
    """Stands where the context handle would: the wrapper must raise before it reaches for it."""

    def __getattr__(self, name):
        raise AssertionError("the library was called")


def _bare():
    from kid_amd import ThompsonMP
    m = ThompsonMP.__new__(ThompsonMP)                      # no kidmp_init: there is no device here
    m._h = None
    m.device = 0
    return m


@pytest.mark.parametrize("bad", [
    np.array([100.0, 300.0], dtype=np.float32),             # dtype
    np.array([100, 300]),                                    # integers
    np.full((4, 2), 100.0),                                  # two-dimensional
    np.array(100.0),                                         # zero-dimensional
    np.empty(0),                                             # empty: unbinding is None
    np.full(8, 100.0)[::2],                                  # not contiguous
    [100.0, 300.0],                                          # neither an array nor a tensor
    100.0,
])
def test_wrapper_rejects_wrong_shapes_and_dtypes_before_the_library(bad, monkeypatch):
    import kid_amd.thompson as th
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    with pytest.raises(th.KidmpError, match="set_column_nc"):
        _bare().set_column_nc(bad)


def test_wrapper_rejects_wrong_tensors_before_the_library(monkeypatch):
    import torch
    import kid_amd.thompson as th
    monkeypatch.setattr(th, "load_library", lambda *a: _NoLibrary())
    for bad in (torch.full((4,), 100.0, dtype=torch.float32), torch.full((2, 2), 100.0, dtype=torch.float64),
                torch.empty(0, dtype=torch.float64), torch.full((8,), 100.0, dtype=torch.float64)[::2],
                torch.tensor([100, 300])):
        with pytest.raises(th.KidmpError, match="set_column_nc"):
            _bare().set_column_nc(bad)


def test_wrapper_hands_a_good_array_to_the_library():
    import kid_amd.thompson as th
    v = np.array([25.0, 100.0, 300.0])
    assert th.column_nc_pointer(v) == (v.ctypes.data, 3)
    import torch
    t = torch.tensor([25.0, 1000.0], dtype=torch.float64)
    assert th.column_nc_pointer(t, device=0) == (t.data_ptr(), 2)
