"""Per-column summaries on the device (include/kidmp_summary.h): water paths, liquid cloud optical depth, composite
reflectivity, echo-top, cloud-base, cloud-top and freezing heights -- 16 doubles per column from one read of its
profiles, without a download and without writing a profile.

The four entries of kidmp_summary.h are declared here, on the object load_library() returned, the first time one of
them is needed: include/kidmp.h and its mirror in thompson.py stay what they are.  There is no fallback: without the
library or the device a call raises KidmpError.
"""
import ctypes as C
import math

import numpy as np

from . import thompson as _th
from .thompson import KidmpError

SUMMARY_N = 16                                                  # KIDMP_SUMMARY_N
SUMMARY_NAMES = ("wvp", "cwp", "rwp", "iwp", "swp", "gwp", "tau_c", "dbz_max", "z_dbz_max", "z_echo_top", "dbz_sfc",
                 "z_cloud_base", "z_cloud_top", "n_cloud", "z_freeze")          # slot s is KIDMP_SUM_<NAME>
SUMMARY_INPUTS = ("t", "p", "qv", "qc", "nc", "qi", "qr", "nr", "qs", "qg")
_OPTIONAL = ("nc", "qi", "qs", "qg")                           # whether one may be left out is the library's to say
DEFAULT_CFG = (18.0, 1.0e-5, 273.15)                           # dbz_echo, q_cloud, t_freeze of a NULL cfg


class _SummaryCfg(C.Structure):
    """kidmp_summary_cfg."""
    _fields_ = [("dbz_echo", C.c_double), ("q_cloud", C.c_double), ("t_freeze", C.c_double)]


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_summary.h."""
    i32, i64, vp, rc = C.c_int32, C.c_int64, C.c_void_p, C.c_int
    host = [vp, i64, i32] + [vp] * 11 + [i64, C.POINTER(_SummaryCfg), vp]
    return {
        "kidmp_column_summary_device": (rc, host + [vp]),
        "kidmp32_column_summary_device": (rc, host + [vp]),
        "kidmp_column_summary_host": (rc, host),
        "kidmp32_column_summary_host": (rc, host),
    }


def declare(L):
    """Declare the entries of kidmp_summary.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the summary entries declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _refuse(who, msg):
    raise KidmpError("%s: %s" % (who, msg))


def _cfg(who, cfg):
    """None, or the kidmp_summary_cfg of a dict {dbz_echo, q_cloud, t_freeze} / a sequence of the three (finite numbers)."""
    if cfg is None:
        return None
    try:
        if isinstance(cfg, dict):
            if set(cfg) - {"dbz_echo", "q_cloud", "t_freeze"}:
                raise ValueError
            v = [float(cfg.get(k, d)) for k, d in zip(("dbz_echo", "q_cloud", "t_freeze"), DEFAULT_CFG)]
        else:
            v = [float(x) for x in cfg]
    except (TypeError, ValueError):
        _refuse(who, "cfg must be None, a dict with the keys dbz_echo, q_cloud, t_freeze, or three numbers")
    if len(v) != 3 or not all(math.isfinite(x) for x in v):
        _refuse(who, "cfg must hold three finite numbers (dbz_echo, q_cloud, t_freeze)")
    return _SummaryCfg(*v)


def _dz_stride(who, shape, ncol, nz):
    if tuple(shape) == (nz,):
        return 0
    if tuple(shape) == (ncol, nz):
        return nz
    _refuse(who, "dz must be [nz] = [%d] or [ncol, nz] = [%d, %d], got %s" % (nz, ncol, nz, list(shape)))


def column_summary(model, st, dz, cfg=None, out=None, stream=None):
    """The per-column summary of a device-resident state (kidmp[32]_column_summary_device): one launch.

    st      dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load), keys SUMMARY_INPUTS; nc
            may be missing (or None) unless the context is aerosol-aware, qi and qs + qg in an iiwarm context
    dz      layer depths in m (positive), [nz] for all columns or [ncol, nz], of the state's dtype
    cfg     None = (18 dBZ, 1e-5 kg/kg, 273.15 K), or a dict {dbz_echo, q_cloud, t_freeze} / three numbers
    out     float64 CUDA tensor [ncol, 16] to write into, None = made here
    Returns [ncol, 16] float64: column SUMMARY_NAMES.index(name) is that number, column 15 is reserved (+0.0); NaN where
    the level a slot asks for does not exist.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    who = "column_summary"
    if not isinstance(st, dict) or not isinstance(st.get("t"), torch.Tensor):
        _refuse(who, "the state must be a dict of torch tensors with the keys %s" % (SUMMARY_INPUTS,))
    q = st["t"]
    if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 tensors [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = int(q.shape[0]), int(q.shape[1])

    def check(a, k):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        model._want(a, q.dtype, (ncol, nz), who + ": ", k)

    ptrs = _th._pointers(st, SUMMARY_INPUTS, _OPTIONAL, check, torch.Tensor.data_ptr)
    if not isinstance(dz, torch.Tensor):
        _refuse(who, "dz must be a torch tensor, got %s" % type(dz).__name__)
    stride = _dz_stride(who, dz.shape, ncol, nz)
    model._want(dz, q.dtype, tuple(dz.shape), who + ": ", "dz")
    c = _cfg(who, cfg)
    if out is None:
        out = torch.empty((ncol, SUMMARY_N), dtype=torch.float64, device=q.device)
    elif not isinstance(out, torch.Tensor):
        _refuse(who, "out must be a torch tensor, got %s" % type(out).__name__)
    model._want(out, torch.float64, (ncol, SUMMARY_N), who + ": ", "out")
    L = library()
    fn = L.kidmp_column_summary_device if q.dtype == torch.float64 else L.kidmp32_column_summary_device
    rc = fn(model._h, ncol, nz, *ptrs, dz.data_ptr(), stride, C.byref(c) if c is not None else None, out.data_ptr(),
            _th._stream(stream, q))
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, L.kidmp_last_error(model._h).decode()))
    return out


def column_summary_host(model, st, dz, cfg=None):
    """column_summary on numpy arrays [ncol, nz] (float64 or float32; dz [nz] or [ncol, nz] of the same dtype): chunks of
    columns through the context's staging memory (kidmp[32]_column_summary_host).  Returns numpy [ncol, 16] float64, bit
    for bit what column_summary gives."""
    who = "column_summary_host"
    if not isinstance(st, dict) or not isinstance(st.get("t"), np.ndarray):
        _refuse(who, "the state must be a dict of numpy arrays with the keys %s" % (SUMMARY_INPUTS,))
    q = st["t"]
    if q.dtype not in (np.float64, np.float32) or q.ndim != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 arrays [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = q.shape

    def check(a, k, shape=(ncol, nz)):
        if not (isinstance(a, np.ndarray) and a.dtype == q.dtype and a.flags.c_contiguous and a.shape == shape):
            _refuse(who, "%s must be a contiguous %s array %s" % (k, q.dtype.name, list(shape)))

    ptrs = _th._pointers(st, SUMMARY_INPUTS, _OPTIONAL, check, lambda a: a.ctypes.data)
    if not isinstance(dz, np.ndarray):
        _refuse(who, "dz must be a numpy array, got %s" % type(dz).__name__)
    stride = _dz_stride(who, dz.shape, ncol, nz)
    check(dz, "dz", dz.shape)
    c = _cfg(who, cfg)
    out = np.empty((ncol, SUMMARY_N), dtype=np.float64)
    L = library()
    fn = L.kidmp_column_summary_host if q.dtype == np.float64 else L.kidmp32_column_summary_host
    rc = fn(model._h, ncol, nz, *ptrs, dz.ctypes.data, stride, C.byref(c) if c is not None else None, out.ctypes.data)
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, L.kidmp_last_error(model._h).decode()))
    return out
