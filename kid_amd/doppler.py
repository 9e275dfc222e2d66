"""The Doppler moments of a vertically pointing radar on the device (include/kidmp_doppler.h): reflectivity, mean Doppler
velocity and spectrum width of every level, with the per-species reflectivities and reflectivity-weighted fall speeds
they are formed from -- one launch per call.

The four entries of kidmp_doppler.h are declared here, on the object load_library() returned, the first time one of them
is needed: include/kidmp.h and its mirror in thompson.py stay what they are.  There is no fallback: without the library
or the device a call raises KidmpError.
"""
import ctypes as C

import numpy as np

from . import thompson as _th
from .thompson import KidmpError

DOPPLER_NAMES = ("dbz", "vd", "sw", "vz_r", "vz_s", "vz_g", "dbz_r", "dbz_s", "dbz_g")   # kidmp_doppler_out
DOPPLER_INPUTS = ("t", "p", "qv", "qr", "nr", "qs", "qg")
_OPTIONAL = ("qs", "qg")                                      # left out (or None) = zero, in any context


class _DopplerOut(C.Structure):
    """kidmp_doppler_out / kidmp32_doppler_out: nine pointers."""
    _fields_ = [(n, C.c_void_p) for n in DOPPLER_NAMES]


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_doppler.h."""
    i32, i64, vp, rc = C.c_int32, C.c_int64, C.c_void_p, C.c_int
    host = [vp, i64, i32] + [vp] * 8 + [C.POINTER(_DopplerOut)]
    return {
        "kidmp_doppler_moments_device": (rc, host + [vp]),
        "kidmp32_doppler_moments_device": (rc, host + [vp]),
        "kidmp_doppler_moments_host": (rc, host),
        "kidmp32_doppler_moments_host": (rc, host),
    }


def declare(L):
    """Declare the entries of kidmp_doppler.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the Doppler entries declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _refuse(who, msg):
    raise KidmpError("%s: %s" % (who, msg))


def _wanted(who, want):
    if isinstance(want, str):
        want = (want,)
    try:
        want = tuple(want)
    except TypeError:
        _refuse(who, "want must be a name or a sequence of names out of %s" % (DOPPLER_NAMES,))
    for n in want:
        if n not in DOPPLER_NAMES:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, DOPPLER_NAMES))
    if len(set(want)) != len(want):
        _refuse(who, "want names an output twice")
    if not want:
        _refuse(who, "nothing requested: want is empty")
    return want


def _call(fn, model, ncol, nz, ptrs, w, out, *stream):
    o = _DopplerOut(**out)
    rc = fn(model._h, ncol, nz, *ptrs, w, C.byref(o), *stream)
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, library().kidmp_last_error(model._h).decode()))


def doppler_moments(model, st, w=None, want=DOPPLER_NAMES, stream=None):
    """Radar moments of a device-resident state (kidmp[32]_doppler_moments_device): one launch.

    st      dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load), keys DOPPLER_INPUTS; qs
            and qg may be missing (or None): zero
    w       None = still air, or the vertical air velocity [ncol, nz] in m s-1, positive upward
    want    the profiles to form, names out of DOPPLER_NAMES; one that is not named costs no store
    Returns a dict name -> [ncol, nz] tensor of the state's dtype: dbz* in dBZ; vd, sw, vz_* in m s-1, positive downward;
    a level without rain, snow and graupel has vd = sw = 0.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    who = "doppler_moments"
    if not isinstance(st, dict) or not isinstance(st.get("t"), torch.Tensor):
        _refuse(who, "the state must be a dict of torch tensors with the keys %s" % (DOPPLER_INPUTS,))
    q = st["t"]
    if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 tensors [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = int(q.shape[0]), int(q.shape[1])
    want = _wanted(who, want)

    def check(a, k):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        model._want(a, q.dtype, (ncol, nz), who + ": ", k)

    ptrs = _th._pointers(st, DOPPLER_INPUTS, _OPTIONAL, check, torch.Tensor.data_ptr)
    if w is not None:
        check(w, "w")
    res = {n: torch.empty((ncol, nz), dtype=q.dtype, device=q.device) for n in want}
    L = library()
    fn = L.kidmp_doppler_moments_device if q.dtype == torch.float64 else L.kidmp32_doppler_moments_device
    _call(fn, model, ncol, nz, ptrs, w.data_ptr() if w is not None else None, {n: res[n].data_ptr() for n in want}, _th._stream(stream, q))
    return res


def doppler_moments_host(model, st, w=None, want=DOPPLER_NAMES):
    """doppler_moments on numpy arrays [ncol, nz] (float64 or float32; w of the same dtype): chunks of columns through the
    context's staging memory (kidmp[32]_doppler_moments_host); only the profiles in `want` come back over PCIe.  Returns
    numpy arrays, bit for bit what doppler_moments gives."""
    who = "doppler_moments_host"
    if not isinstance(st, dict) or not isinstance(st.get("t"), np.ndarray):
        _refuse(who, "the state must be a dict of numpy arrays with the keys %s" % (DOPPLER_INPUTS,))
    q = st["t"]
    if q.dtype not in (np.float64, np.float32) or q.ndim != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 arrays [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = q.shape
    want = _wanted(who, want)

    def check(a, k):
        if not (isinstance(a, np.ndarray) and a.dtype == q.dtype and a.flags.c_contiguous and a.shape == (ncol, nz)):
            _refuse(who, "%s must be a contiguous %s array %s" % (k, q.dtype.name, [ncol, nz]))

    ptrs = _th._pointers(st, DOPPLER_INPUTS, _OPTIONAL, check, lambda a: a.ctypes.data)
    if w is not None:
        check(w, "w")
    res = {n: np.empty((ncol, nz), dtype=q.dtype) for n in want}
    L = library()
    fn = L.kidmp_doppler_moments_host if q.dtype == np.float64 else L.kidmp32_doppler_moments_host
    _call(fn, model, ncol, nz, ptrs, w.ctypes.data if w is not None else None, {n: res[n].ctypes.data for n in want})
    return res
