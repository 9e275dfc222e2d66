"""The Doppler spectrum of a vertically pointing radar on the device (include/kidmp_dspectrum.h): per level the
reflectivity of rain, snow and graupel as a function of radial velocity, on a uniform velocity grid, from the load, the
size distributions and the fall-speed laws of doppler_moments -- one launch per call.

Turbulent or beam broadening is a one-dimensional convolution along the bin axis (axis 1 of a spectrum), which the
caller applies; the spectra here are the quiet-air ones shifted by the vertical air velocity.  kid_amd.specproc's
spectrum_process applies it on the device, with a noise floor, detection and the moments, in one launch.

The four entries of kidmp_dspectrum.h are declared here, on the object load_library() returned, the first time one of
them is needed: include/kidmp.h and its mirror in thompson.py stay what they are.  There is no fallback: without the
library or the device a call raises KidmpError.
"""
import ctypes as C
import math

import numpy as np

from . import thompson as _th
from .thompson import KidmpError

DSPECTRUM_NAMES = ("total", "rain", "snow", "graupel", "below", "above")   # kidmp_dspectrum_out
DSPECTRUM_SPECIES = ("r", "s", "g")                             # rain, snow, graupel: kidmp_dspectrum_grids
DSPECTRUM_INPUTS = ("t", "p", "qv", "qr", "nr", "qs", "qg")
DSPECTRUM_MAX_NV = 256                                          # KIDMP_DSPECTRUM_MAX_NV
DSPECTRUM_MAX_BINS = 256                                        # KIDMP_DSPECTRUM_MAX_BINS
_OPTIONAL = ("qs", "qg")                                        # left out (or None) = zero, in any context
_PROFILES = ("below", "above")                                  # [ncol, nz]; the others are [ncol, nv, nz]
_NSPEC = len(DSPECTRUM_SPECIES)


class _DSpectrumOut(C.Structure):
    """kidmp_dspectrum_out / kidmp32_dspectrum_out: six pointers."""
    _fields_ = [(n, C.c_void_p) for n in DSPECTRUM_NAMES]


class _DSpectrumGrids(C.Structure):
    """kidmp_dspectrum_grids: D, dD and nb by species."""
    _fields_ = [("D", C.c_void_p * _NSPEC), ("dD", C.c_void_p * _NSPEC), ("nb", C.c_int32 * _NSPEC)]


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_dspectrum.h."""
    i32, i64, vp, rc, f64 = C.c_int32, C.c_int64, C.c_void_p, C.c_int, C.c_double
    host = [vp, i64, i32] + [vp] * 8 + [f64, f64, i32, C.POINTER(_DSpectrumGrids), C.POINTER(_DSpectrumOut)]
    return {
        "kidmp_doppler_spectrum_device": (rc, host + [vp]),
        "kidmp32_doppler_spectrum_device": (rc, host + [vp]),
        "kidmp_doppler_spectrum_host": (rc, host),
        "kidmp32_doppler_spectrum_host": (rc, host),
    }


def declare(L):
    """Declare the entries of kidmp_dspectrum.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the Doppler-spectrum entries declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _refuse(who, msg):
    raise KidmpError("%s: %s" % (who, msg))


def velocity_grid(v0, dv, nv):
    """The centres of the nv velocity bins, v0 + j*dv in m s-1 (positive downward): a float64 numpy array."""
    _grid("velocity_grid", v0, dv, nv)
    return float(v0) + float(dv) * np.arange(int(nv), dtype=np.float64)


def _grid(who, v0, dv, nv):
    try:
        v0, dv = float(v0), float(dv)
    except (TypeError, ValueError):
        _refuse(who, "v0 and dv must be numbers")
    if isinstance(nv, bool) or not isinstance(nv, (int, np.integer)) or not 1 <= nv <= DSPECTRUM_MAX_NV:
        _refuse(who, "nv must be an integer in [1, %d]" % DSPECTRUM_MAX_NV)
    if not (math.isfinite(dv) and dv > 0.0 and math.isfinite(1.0 / dv)):
        _refuse(who, "dv must be finite and above 0")
    if not math.isfinite(v0):
        _refuse(who, "v0 must be finite")
    return v0, dv, int(nv)


def _wanted(who, want):
    if isinstance(want, str):
        want = (want,)
    try:
        want = tuple(want)
    except TypeError:
        _refuse(who, "want must be a name or a sequence of names out of %s" % (DSPECTRUM_NAMES,))
    for n in want:
        if n not in DSPECTRUM_NAMES:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, DSPECTRUM_NAMES))
    if len(set(want)) != len(want):
        _refuse(who, "want names an output twice")
    if not want:
        _refuse(who, "nothing requested: want is empty")
    return want


def _grid_sizes(who, grids, is_array, check):
    """species -> nb of every grid the caller gave, each judged by check(a, name, nb)."""
    if grids is None:
        grids = {}
    if not isinstance(grids, dict):
        _refuse(who, "grids must be a dict species -> (D, dD)")
    nb = {}
    for x, g in grids.items():
        if x not in DSPECTRUM_SPECIES:
            _refuse(who, "unknown species %r in grids: out of %s" % (x, DSPECTRUM_SPECIES))
        if g is None:
            continue
        if not (isinstance(g, (tuple, list)) and len(g) == 2 and is_array(g[0]) and is_array(g[1])):
            _refuse(who, "grids[%r] must be a pair (D, dD) of arrays" % x)
        D, dD = g
        if len(D.shape) != 1 or not 1 <= D.shape[0] <= DSPECTRUM_MAX_BINS:
            _refuse(who, "grids[%r]: D must be one-dimensional with 1 to %d bins" % (x, DSPECTRUM_MAX_BINS))
        nb[x] = int(D.shape[0])
        check(D, "grids[%r] D" % x, nb[x])
        check(dD, "grids[%r] dD" % x, nb[x])
    return nb


def _call(fn, model, ncol, nz, ptrs, w, v0, dv, nv, grids, nb, addr, res, *stream):
    o = _DSpectrumOut(**{n: addr(a) for n, a in res.items()})
    g = _DSpectrumGrids()
    for i, x in enumerate(DSPECTRUM_SPECIES):
        if x in nb:
            g.D[i], g.dD[i], g.nb[i] = addr(grids[x][0]), addr(grids[x][1]), nb[x]
    rc = fn(model._h, ncol, nz, *ptrs, w, v0, dv, nv, C.byref(g), C.byref(o), *stream)
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, library().kidmp_last_error(model._h).decode()))


def _results(who, want, out, shapes, check, fresh):
    if out is not None and not isinstance(out, dict):
        _refuse(who, "out must be a dict name -> array")
    res = {}
    for n in want:
        if out is not None and out.get(n) is not None:
            check(out[n], "out[%r]" % n, shapes[n])
            res[n] = out[n]
        else:
            res[n] = fresh(shapes[n])
    return res


def doppler_spectrum(model, st, v0, dv, nv, w=None, grids=None, want=("total",), out=None, stream=None):
    """The Doppler spectrum of a device-resident state (kidmp[32]_doppler_spectrum_device): one launch.

    st      dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load), keys DSPECTRUM_INPUTS; qs
            and qg may be missing (or None): zero
    v0, dv, nv  the velocity grid: nv (1..DSPECTRUM_MAX_NV) bins of width dv > 0 m s-1, v0 the centre of bin 0
            (velocity_grid gives the centres); velocities are positive downward
    w       None = still air, or the vertical air velocity [ncol, nz] in m s-1, positive upward
    grids   None, or a dict species ("r", "s", "g") -> (D, dD): float64 CUDA tensors [nb], 1 <= nb <= DSPECTRUM_MAX_BINS,
            bin diameters and widths in m; a species without an entry is put on the scheme's own 100 bins
    want    names out of DSPECTRUM_NAMES: "total", "rain", "snow", "graupel" are spectra [ncol, nv, nz] in m6 m-3 per
            bin (10*log10(1e18 * sum over bins) is dBZ); "below" and "above" [ncol, nz] hold what `total` puts outside
            the grid.  What is not named costs nothing.
    out     None, or a dict name -> tensor of the result's shape and dtype to write into instead of a fresh one
    Turbulent or beam broadening is a 1-D convolution along the bin axis (axis 1), which the caller applies
    (spectrum_process does it on the device).
    Returns a dict name -> tensor of the state's dtype.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    who = "doppler_spectrum"
    if not isinstance(st, dict) or not isinstance(st.get("t"), torch.Tensor):
        _refuse(who, "the state must be a dict of torch tensors with the keys %s" % (DSPECTRUM_INPUTS,))
    q = st["t"]
    if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 tensors [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = int(q.shape[0]), int(q.shape[1])
    v0, dv, nv = _grid(who, v0, dv, nv)
    want = _wanted(who, want)

    def check(a, k, shape=(ncol, nz), dtype=q.dtype):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        model._want(a, dtype, shape, who + ": ", k)

    ptrs = _th._pointers(st, DSPECTRUM_INPUTS, _OPTIONAL, check, torch.Tensor.data_ptr)
    if w is not None:
        check(w, "w")
    nb = _grid_sizes(who, grids, lambda a: isinstance(a, torch.Tensor), lambda a, k, n: check(a, k, (n,), torch.float64))
    shapes = {n: (ncol, nz) if n in _PROFILES else (ncol, nv, nz) for n in want}
    res = _results(who, want, out, shapes, check, lambda s: torch.empty(s, dtype=q.dtype, device=q.device))
    L = library()
    fn = L.kidmp_doppler_spectrum_device if q.dtype == torch.float64 else L.kidmp32_doppler_spectrum_device
    _call(fn, model, ncol, nz, ptrs, w.data_ptr() if w is not None else None, v0, dv, nv, grids, nb, torch.Tensor.data_ptr, res,
          _th._stream(stream, q))
    return res


def doppler_spectrum_host(model, st, v0, dv, nv, w=None, grids=None, want=("total",), out=None):
    """doppler_spectrum on numpy arrays [ncol, nz] (float64 or float32; w of the same dtype; grids float64 numpy arrays):
    chunks of columns through the context's staging memory (kidmp[32]_doppler_spectrum_host), sized so that the staging
    stays under 256 MiB; only what `want` names comes back over PCIe.  Returns numpy arrays, bit for bit what
    doppler_spectrum gives."""
    who = "doppler_spectrum_host"
    if not isinstance(st, dict) or not isinstance(st.get("t"), np.ndarray):
        _refuse(who, "the state must be a dict of numpy arrays with the keys %s" % (DSPECTRUM_INPUTS,))
    q = st["t"]
    if q.dtype not in (np.float64, np.float32) or q.ndim != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 arrays [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = q.shape
    v0, dv, nv = _grid(who, v0, dv, nv)
    want = _wanted(who, want)

    def check(a, k, shape=(ncol, nz), dtype=q.dtype):
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and a.shape == tuple(shape)):
            _refuse(who, "%s must be a contiguous %s array %s" % (k, np.dtype(dtype).name, list(shape)))

    addr = lambda a: a.ctypes.data   # noqa: E731
    ptrs = _th._pointers(st, DSPECTRUM_INPUTS, _OPTIONAL, check, addr)
    if w is not None:
        check(w, "w")
    nb = _grid_sizes(who, grids, lambda a: isinstance(a, np.ndarray), lambda a, k, n: check(a, k, (n,), np.float64))
    shapes = {n: (ncol, nz) if n in _PROFILES else (ncol, nv, nz) for n in want}
    res = _results(who, want, out, shapes, check, lambda s: np.empty(s, dtype=q.dtype))
    L = library()
    fn = L.kidmp_doppler_spectrum_host if q.dtype == np.float64 else L.kidmp32_doppler_spectrum_host
    _call(fn, model, ncol, nz, ptrs, w.ctypes.data if w is not None else None, v0, dv, nv, grids, nb, addr, res)
    return res
