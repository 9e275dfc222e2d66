"""The scheme's size distributions on diameter bins (include/kidmp_spectra.h): per level the slope and intercept of cloud
water, cloud ice, rain, snow and graupel as mp_thompson loads the state, and the number of particles per m3 of air in
every bin of a diameter grid -- the scheme's own 100 bins per species or the caller's -- in one launch per call.

The five entries of kidmp_spectra.h are declared here, on the object load_library() returned, the first time one of them
is needed: include/kidmp.h and its mirror in thompson.py stay what they are.  There is no fallback: without the library or
the device a call raises KidmpError.
"""
import ctypes as C

import numpy as np

from . import thompson as _th
from .thompson import KidmpError

SPECTRA_SPECIES = ("c", "i", "r", "s", "g")                    # cloud water, cloud ice, rain, snow, graupel: kidmp_spectra_bins
SPECTRA_PARAMS = ("lam_c", "n0_c", "nu_c", "lam_i", "n0_i", "lam_r", "n0_r", "smob", "smoc", "lam_g", "n0_g")   # kidmp_spectra_out
SPECTRA_INPUTS = ("t", "p", "qv", "qc", "nc", "qi", "ni", "qr", "nr", "qs", "qg")
SPECTRA_MAX_BINS = 256                                         # KIDMP_SPECTRA_MAX_BINS
SPECTRA_DEFAULT_BINS = 100                                     # KIDMP_SPECTRA_DEFAULT_BINS
_OPTIONAL = ("nc", "qi", "ni", "qs", "qg")                     # whether one may be left out is the library's to say
_NSPEC = len(SPECTRA_SPECIES)


class _SpectraOut(C.Structure):
    """kidmp_spectra_out / kidmp32_spectra_out: eleven pointers."""
    _fields_ = [(n, C.c_void_p) for n in SPECTRA_PARAMS]


class _SpectraBins(C.Structure):
    """kidmp_spectra_bins / kidmp32_spectra_bins: five pointers."""
    _fields_ = [("n_" + x, C.c_void_p) for x in SPECTRA_SPECIES]


class _SpectraGrids(C.Structure):
    """kidmp_spectra_grids: D, dD and nb by species."""
    _fields_ = [("D", C.c_void_p * _NSPEC), ("dD", C.c_void_p * _NSPEC), ("nb", C.c_int32 * _NSPEC)]


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_spectra.h."""
    i32, i64, vp, rc = C.c_int32, C.c_int64, C.c_void_p, C.c_int
    host = [vp, i64, i32] + [vp] * 11 + [C.POINTER(_SpectraOut), C.POINTER(_SpectraBins), C.POINTER(_SpectraGrids)]
    return {
        "kidmp_spectra_default_grid": (rc, [vp, i32, vp, vp, i32]),
        "kidmp_size_spectra_device": (rc, host + [vp]),
        "kidmp32_size_spectra_device": (rc, host + [vp]),
        "kidmp_size_spectra_host": (rc, host),
        "kidmp32_size_spectra_host": (rc, host),
    }


def declare(L):
    """Declare the entries of kidmp_spectra.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the size-spectra entries declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _refuse(who, msg):
    raise KidmpError("%s: %s" % (who, msg))


def _wanted(who, want):
    names = SPECTRA_SPECIES + SPECTRA_PARAMS
    if isinstance(want, str):
        want = (want,)
    try:
        want = tuple(want)
    except TypeError:
        _refuse(who, "want must be a name or a sequence of names out of %s" % (names,))
    for n in want:
        if n not in names:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, names))
    if len(set(want)) != len(want):
        _refuse(who, "want names an output twice")
    if not want:
        _refuse(who, "nothing requested: want is empty")
    return want


def _grid_sizes(who, grids, want, is_array, check):
    """species -> nb of every wanted spectrum; the caller's grids are judged by check(a, name, nb)."""
    if grids is None:
        grids = {}
    if not isinstance(grids, dict):
        _refuse(who, "grids must be a dict species -> (D, dD)")
    for x in grids:
        if x not in SPECTRA_SPECIES:
            _refuse(who, "unknown species %r in grids: out of %s" % (x, SPECTRA_SPECIES))
    nb = {}
    for x in SPECTRA_SPECIES:
        if x not in want:
            continue
        nb[x] = SPECTRA_DEFAULT_BINS
        g = grids.get(x)
        if g is None:
            continue
        if not (isinstance(g, (tuple, list)) and len(g) == 2 and is_array(g[0]) and is_array(g[1])):
            _refuse(who, "grids[%r] must be a pair (D, dD) of arrays" % x)
        D, dD = g
        if len(D.shape) != 1 or not 1 <= D.shape[0] <= SPECTRA_MAX_BINS:
            _refuse(who, "grids[%r]: D must be one-dimensional with 1 to %d bins" % (x, SPECTRA_MAX_BINS))
        nb[x] = int(D.shape[0])
        check(D, "grids[%r] D" % x, nb[x])
        check(dD, "grids[%r] dD" % x, nb[x])
    return nb


def _shapes(want, nb, ncol, nz):
    return {n: (ncol, nb[n], nz) if n in SPECTRA_SPECIES else (ncol, nz) for n in want}


def _call(who, fn, model, ncol, nz, ptrs, want, addr, res, grids, nb, *stream):
    par = _SpectraOut(**{n: addr(res[n]) for n in want if n in SPECTRA_PARAMS})
    bins = _SpectraBins(**{"n_" + x: addr(res[x]) for x in want if x in SPECTRA_SPECIES})
    g = _SpectraGrids()
    for i, x in enumerate(SPECTRA_SPECIES):
        pair = (grids or {}).get(x) if x in nb else None
        if pair is not None:
            g.D[i], g.dD[i], g.nb[i] = addr(pair[0]), addr(pair[1]), nb[x]
    rc = fn(model._h, ncol, nz, *ptrs, C.byref(par), C.byref(bins), C.byref(g), *stream)
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, library().kidmp_last_error(model._h).decode()))


def default_grid(model, species):
    """The scheme's own bins of `species` (one of SPECTRA_SPECIES; M:605-657): (D, dD), float64 numpy arrays in m."""
    who = "default_grid"
    if species not in SPECTRA_SPECIES:
        _refuse(who, "unknown species %r: out of %s" % (species, SPECTRA_SPECIES))
    L = library()
    x = SPECTRA_SPECIES.index(species)
    nb = L.kidmp_spectra_default_grid(model._h, x, None, None, 0)
    if nb < 0:
        raise KidmpError("kidmp error %d: %s" % (nb, L.kidmp_last_error(model._h).decode()))
    D, dD = np.empty(nb), np.empty(nb)
    rc = L.kidmp_spectra_default_grid(model._h, x, D.ctypes.data, dD.ctypes.data, nb)
    if rc != nb:
        raise KidmpError("kidmp error %d: %s" % (rc, L.kidmp_last_error(model._h).decode()))
    return D, dD


def size_spectra(model, st, want=SPECTRA_SPECIES, grids=None, out=None, stream=None):
    """Size distributions of a device-resident state (kidmp[32]_size_spectra_device): one launch.

    st      dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load), keys SPECTRA_INPUTS; nc may
            be missing (or None) unless the context is aerosol-aware, qi, ni, qs and qg in an iiwarm context or when no
            frozen output is wanted
    want    names out of SPECTRA_SPECIES (the spectrum, [ncol, nb, nz]: particles per m3 of air in each bin) and
            SPECTRA_PARAMS (a parameter profile, [ncol, nz]); what is not named costs nothing
    grids   None, or a dict species -> (D, dD): float64 CUDA tensors [nb], 1 <= nb <= SPECTRA_MAX_BINS, bin diameters and
            widths in m; a species without an entry is put on the scheme's own SPECTRA_DEFAULT_BINS bins (default_grid)
    out     None, or a dict name -> tensor of the result's shape and dtype to write into instead of a fresh one
    Returns a dict name -> tensor of the state's dtype.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    who = "size_spectra"
    if not isinstance(st, dict) or not isinstance(st.get("t"), torch.Tensor):
        _refuse(who, "the state must be a dict of torch tensors with the keys %s" % (SPECTRA_INPUTS,))
    q = st["t"]
    if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 tensors [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = int(q.shape[0]), int(q.shape[1])
    want = _wanted(who, want)

    def check(a, k, shape=(ncol, nz), dtype=q.dtype):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        model._want(a, dtype, shape, who + ": ", k)

    ptrs = _th._pointers(st, SPECTRA_INPUTS, _OPTIONAL, check, torch.Tensor.data_ptr)
    nb = _grid_sizes(who, grids, want, lambda a: isinstance(a, torch.Tensor), lambda a, k, n: check(a, k, (n,), torch.float64))
    shapes = _shapes(want, nb, ncol, nz)
    if out is not None and not isinstance(out, dict):
        _refuse(who, "out must be a dict name -> tensor")
    res = {}
    for n in want:
        if out is not None and out.get(n) is not None:
            check(out[n], "out[%r]" % n, shapes[n])
            res[n] = out[n]
        else:
            res[n] = torch.empty(shapes[n], dtype=q.dtype, device=q.device)
    L = library()
    fn = L.kidmp_size_spectra_device if q.dtype == torch.float64 else L.kidmp32_size_spectra_device
    _call(who, fn, model, ncol, nz, ptrs, want, torch.Tensor.data_ptr, res, grids, nb, _th._stream(stream, q))
    return res


def size_spectra_host(model, st, want=SPECTRA_SPECIES, grids=None, out=None):
    """size_spectra on numpy arrays [ncol, nz] (float64 or float32; grids float64 numpy arrays): chunks of columns through
    the context's staging memory (kidmp[32]_size_spectra_host); only what `want` names crosses PCIe.  Returns numpy
    arrays, bit for bit what size_spectra gives."""
    who = "size_spectra_host"
    if not isinstance(st, dict) or not isinstance(st.get("t"), np.ndarray):
        _refuse(who, "the state must be a dict of numpy arrays with the keys %s" % (SPECTRA_INPUTS,))
    q = st["t"]
    if q.dtype not in (np.float64, np.float32) or q.ndim != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 arrays [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = q.shape
    want = _wanted(who, want)

    def check(a, k, shape=(ncol, nz), dtype=q.dtype):
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and a.shape == tuple(shape)):
            _refuse(who, "%s must be a contiguous %s array %s" % (k, np.dtype(dtype).name, list(shape)))

    addr = lambda a: a.ctypes.data   # noqa: E731
    ptrs = _th._pointers(st, SPECTRA_INPUTS, _OPTIONAL, check, addr)
    nb = _grid_sizes(who, grids, want, lambda a: isinstance(a, np.ndarray), lambda a, k, n: check(a, k, (n,), np.float64))
    shapes = _shapes(want, nb, ncol, nz)
    if out is not None and not isinstance(out, dict):
        _refuse(who, "out must be a dict name -> array")
    res = {}
    for n in want:
        if out is not None and out.get(n) is not None:
            check(out[n], "out[%r]" % n, shapes[n])
            res[n] = out[n]
        else:
            res[n] = np.empty(shapes[n], dtype=q.dtype)
    L = library()
    fn = L.kidmp_size_spectra_host if q.dtype == np.float64 else L.kidmp32_size_spectra_host
    _call(who, fn, model, ncol, nz, ptrs, want, addr, res, grids, nb)
    return res
