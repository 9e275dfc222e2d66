"""Block-O fall speeds and precipitation-flux profiles on the device (include/kidmp_fall.h): the mass- and number-weighted
fall speeds of rain, ice, snow and graupel at every level, the sedimentation fluxes v * rho q per species and in total
(the real `total_ppt_level`), and the CFL substep counts those speeds imply for a given dt -- one launch per call.

The four entries of kidmp_fall.h are declared here, on the object load_library() returned, the first time one of them is
needed: include/kidmp.h and its mirror in thompson.py stay what they are.  There is no fallback: without the library or
the device a call raises KidmpError.
"""
import ctypes as C

import numpy as np

from . import thompson as _th
from .thompson import KidmpError

FALL_NAMES = ("vt_r", "vt_nr", "vt_i", "vt_ni", "vt_s", "vt_g", "flux_r", "flux_i", "flux_s", "flux_g", "flux_total")   # kidmp_fall_out
FALL_INPUTS = ("t", "p", "qv", "qr", "nr", "qi", "ni", "qs", "qg")
_OPTIONAL = ("qi", "ni", "qs", "qg")                           # whether one may be left out is the library's to say


class _FallOut(C.Structure):
    """kidmp_fall_out / kidmp32_fall_out: eleven pointers."""
    _fields_ = [(n, C.c_void_p) for n in FALL_NAMES]


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_fall.h."""
    i32, i64, vp, rc = C.c_int32, C.c_int64, C.c_void_p, C.c_int
    host = [vp, i64, i32] + [vp] * 11 + [i64, C.c_double, C.POINTER(_FallOut), vp]
    return {
        "kidmp_fall_speeds_device": (rc, host + [vp]),
        "kidmp32_fall_speeds_device": (rc, host + [vp]),
        "kidmp_fall_speeds_host": (rc, host),
        "kidmp32_fall_speeds_host": (rc, host),
    }


def declare(L):
    """Declare the entries of kidmp_fall.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the fall-speed entries declared."""
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
        _refuse(who, "want must be a name or a sequence of names out of %s" % (FALL_NAMES,))
    for n in want:
        if n not in FALL_NAMES:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, FALL_NAMES))
    if len(set(want)) != len(want):
        _refuse(who, "want names an output twice")
    return want


def _dz_dt(who, dz, dt, ncol, nz, want):
    """(stride, dt) of a request for nstep, or None when dz and dt are both left out."""
    if dz is None and dt is None:
        if not want:
            _refuse(who, "nothing requested: want is empty and dz, dt are not given")
        return None
    if dz is None or dt is None:
        _refuse(who, "nstep needs both dz and dt")
    try:
        dt = float(dt)
    except (TypeError, ValueError):
        _refuse(who, "dt must be a number")
    if not dt > 0.0:
        _refuse(who, "dt must be > 0")
    if tuple(dz.shape) == (nz,):
        return 0, dt
    if tuple(dz.shape) == (ncol, nz):
        return nz, dt
    _refuse(who, "dz must be [nz] = [%d] or [ncol, nz] = [%d, %d], got %s" % (nz, ncol, nz, list(dz.shape)))


def _call(who, fn, model, ncol, nz, ptrs, boost, dz, stride_dt, out, nstep, *stream):
    o = _FallOut(**out)
    stride, dt = stride_dt if stride_dt is not None else (0, 0.0)
    rc = fn(model._h, ncol, nz, *ptrs, boost, dz, stride, dt, C.byref(o), nstep, *stream)
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, library().kidmp_last_error(model._h).decode()))


def fall_speeds(model, st, boost=None, dz=None, dt=None, want=FALL_NAMES, stream=None):
    """Fall speeds and sedimentation fluxes of a device-resident state (kidmp[32]_fall_speeds_device): one launch.

    st      dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load), keys FALL_INPUTS; qi, ni,
            qs and qg may be missing (or None) in an iiwarm context
    boost   None = the vts_boost of a level without riming (1.0 where T < T_0, 1.5 elsewhere), or a tensor [ncol, nz]
    dz, dt  both given: the result also holds `nstep`, int32 [ncol, 4] (rain, ice, snow, graupel); dz in m (positive),
            [nz] for all columns or [ncol, nz], of the state's dtype; dt in s
    want    the profiles to form, names out of FALL_NAMES; one that is not named costs no store
    Returns a dict name -> [ncol, nz] tensor of the state's dtype (m s-1; kg m-2 s-1).  Asynchronous on `stream`
    (default: torch's current stream)."""
    import torch
    who = "fall_speeds"
    if not isinstance(st, dict) or not isinstance(st.get("t"), torch.Tensor):
        _refuse(who, "the state must be a dict of torch tensors with the keys %s" % (FALL_INPUTS,))
    q = st["t"]
    if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 tensors [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = int(q.shape[0]), int(q.shape[1])
    want = _wanted(who, want)

    def check(a, k):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        model._want(a, q.dtype, (ncol, nz), who + ": ", k)

    ptrs = _th._pointers(st, FALL_INPUTS, _OPTIONAL, check, torch.Tensor.data_ptr)
    if boost is not None:
        check(boost, "boost")
    if dz is not None and not isinstance(dz, torch.Tensor):
        _refuse(who, "dz must be a torch tensor, got %s" % type(dz).__name__)
    sd = _dz_dt(who, dz, dt, ncol, nz, want)
    if sd is not None:
        model._want(dz, q.dtype, tuple(dz.shape), who + ": ", "dz")
    res = {n: torch.empty((ncol, nz), dtype=q.dtype, device=q.device) for n in want}
    if sd is not None:
        res["nstep"] = torch.empty((ncol, 4), dtype=torch.int32, device=q.device)
    L = library()
    fn = L.kidmp_fall_speeds_device if q.dtype == torch.float64 else L.kidmp32_fall_speeds_device
    _call(who, fn, model, ncol, nz, ptrs, boost.data_ptr() if boost is not None else None, dz.data_ptr() if sd is not None else None, sd,
          {n: res[n].data_ptr() for n in want}, res["nstep"].data_ptr() if sd is not None else None, _th._stream(stream, q))
    return res


def fall_speeds_host(model, st, boost=None, dz=None, dt=None, want=FALL_NAMES):
    """fall_speeds on numpy arrays [ncol, nz] (float64 or float32; boost and dz of the same dtype): chunks of columns
    through the context's staging memory (kidmp[32]_fall_speeds_host); only the profiles in `want` cross PCIe.  Returns
    numpy arrays, bit for bit what fall_speeds gives."""
    who = "fall_speeds_host"
    if not isinstance(st, dict) or not isinstance(st.get("t"), np.ndarray):
        _refuse(who, "the state must be a dict of numpy arrays with the keys %s" % (FALL_INPUTS,))
    q = st["t"]
    if q.dtype not in (np.float64, np.float32) or q.ndim != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 arrays [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = q.shape
    want = _wanted(who, want)

    def check(a, k, shape=(ncol, nz)):
        if not (isinstance(a, np.ndarray) and a.dtype == q.dtype and a.flags.c_contiguous and a.shape == shape):
            _refuse(who, "%s must be a contiguous %s array %s" % (k, q.dtype.name, list(shape)))

    ptrs = _th._pointers(st, FALL_INPUTS, _OPTIONAL, check, lambda a: a.ctypes.data)
    if boost is not None:
        check(boost, "boost")
    if dz is not None and not isinstance(dz, np.ndarray):
        _refuse(who, "dz must be a numpy array, got %s" % type(dz).__name__)
    sd = _dz_dt(who, dz, dt, ncol, nz, want)
    if sd is not None:
        check(dz, "dz", dz.shape)
    res = {n: np.empty((ncol, nz), dtype=q.dtype) for n in want}
    if sd is not None:
        res["nstep"] = np.empty((ncol, 4), dtype=np.int32)
    L = library()
    fn = L.kidmp_fall_speeds_host if q.dtype == np.float64 else L.kidmp32_fall_speeds_host
    _call(who, fn, model, ncol, nz, ptrs, boost.ctypes.data if boost is not None else None, dz.ctypes.data if sd is not None else None, sd,
          {n: res[n].ctypes.data for n in want}, res["nstep"].ctypes.data if sd is not None else None)
    return res
