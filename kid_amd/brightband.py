"""The radar bright band on the device (include/kidmp_brightband.h): calc_refl10cm with melting snow and graupel below
the melting level -- the reference's own melting level and melt fractions, and a Maxwell-Garnett / Rayleigh model of the
wet particle integrated over the scheme's size distributions -- one launch per call.

The definitions are the project's own; parity with another radar simulator is unpinned.

The entries of kidmp_brightband.h are declared here, on the object load_library() returned, the first time one of them
is needed: include/kidmp.h and its mirror in thompson.py stay what they are.  There is no fallback: without the library
or the device a call raises KidmpError.
"""
import ctypes as C
import math

import numpy as np

from . import thompson as _th
from .thompson import KidmpError

BRIGHTBAND_NAMES = ("dbz", "dbz_s", "dbz_g", "enh_s", "enh_g", "fmelt_s", "fmelt_g", "k0")   # kidmp_brightband_out
BRIGHTBAND_SPECIES = ("s", "g")                                 # snow, graupel: kidmp_brightband_grids
BRIGHTBAND_INPUTS = ("t", "p", "qv", "qr", "nr", "qs", "qg")
BRIGHTBAND_MAX_BINS = 256                                       # KIDMP_BB_MAX_BINS
WATER_MATRIX, ICE_MATRIX = 0, 1                                 # KIDMP_BB_WATER_MATRIX, KIDMP_BB_ICE_MATRIX
_OPTIONAL = ("qs", "qg")                                        # left out (or None) = zero, in any context
_NSPEC = len(BRIGHTBAND_SPECIES)
_CFG_KEYS = ("eps_w", "eps_i", "rho_w", "rho_i", "kw2", "topology")


class _BrightBandCfg(C.Structure):
    """kidmp_brightband_cfg."""
    _fields_ = [("eps_w_re", C.c_double), ("eps_w_im", C.c_double), ("eps_i", C.c_double), ("rho_w", C.c_double),
                ("rho_i", C.c_double), ("kw2", C.c_double), ("topology", C.c_int32)]


class _BrightBandOut(C.Structure):
    """kidmp_brightband_out / kidmp32_brightband_out: seven profile pointers and k0."""
    _fields_ = [(n, C.c_void_p) for n in BRIGHTBAND_NAMES]


class _BrightBandGrids(C.Structure):
    """kidmp_brightband_grids: D, dD and nb by species."""
    _fields_ = [("D", C.c_void_p * _NSPEC), ("dD", C.c_void_p * _NSPEC), ("nb", C.c_int32 * _NSPEC)]


def default_eps_i():
    """(1 + 2k)/(1 - k) with k = sqrt(0.176): the real permittivity of ice whose |K_i|**2 is the scheme's 0.176."""
    k = math.sqrt(0.176)
    return (1.0 + 2.0 * k) / (1.0 - k)


class BrightBandCfg:
    """The configuration of the operator; what is not given keeps the value of a NULL cfg: eps_w the complex relative
    permittivity of water (10 cm, 0 C), eps_i the real one of ice, rho_w and rho_i the densities (kg m-3), kw2 the
    normalisation the carrier reflectivity holds, topology WATER_MATRIX or ICE_MATRIX."""

    def __init__(self, eps_w=complex(79.5, 24.9), eps_i=None, rho_w=1000.0, rho_i=900.0, kw2=0.93, topology=WATER_MATRIX):
        self.eps_w, self.eps_i = eps_w, default_eps_i() if eps_i is None else eps_i
        self.rho_w, self.rho_i, self.kw2, self.topology = rho_w, rho_i, kw2, topology

    def as_dict(self):
        return {k: getattr(self, k) for k in _CFG_KEYS}


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_brightband.h."""
    i32, i64, vp, rc = C.c_int32, C.c_int64, C.c_void_p, C.c_int
    host = [vp, i64, i32] + [vp] * 7 + [C.POINTER(_BrightBandCfg), C.POINTER(_BrightBandGrids), C.POINTER(_BrightBandOut)]
    return {
        "kidmp_bright_band_device": (rc, host + [vp]),
        "kidmp32_bright_band_device": (rc, host + [vp]),
        "kidmp_bright_band_host": (rc, host),
        "kidmp32_bright_band_host": (rc, host),
        "kidmp_brightband_defaults": (None, [C.POINTER(_BrightBandCfg)]),
    }


def declare(L):
    """Declare the entries of kidmp_brightband.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the bright-band entries declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _refuse(who, msg):
    raise KidmpError("%s: %s" % (who, msg))


def _config(who, cfg):
    """The ctypes configuration of a BrightBandCfg (None: NULL, the library's defaults), refused here where the library
    would refuse it."""
    if cfg is None:
        return None
    if not isinstance(cfg, BrightBandCfg):
        _refuse(who, "cfg must be a BrightBandCfg or None")
    try:
        ew = complex(cfg.eps_w)
        vals = dict(eps_i=float(cfg.eps_i), rho_w=float(cfg.rho_w), rho_i=float(cfg.rho_i), kw2=float(cfg.kw2))
    except (TypeError, ValueError):
        _refuse(who, "the members of cfg must be numbers")
    if not all(math.isfinite(v) for v in (ew.real, ew.imag) + tuple(vals.values())):
        _refuse(who, "the members of cfg must be finite")
    for k in ("rho_w", "rho_i", "kw2"):
        if not vals[k] > 0.0:
            _refuse(who, "cfg.%s must be above 0" % k)
    if isinstance(cfg.topology, bool) or cfg.topology not in (WATER_MATRIX, ICE_MATRIX):
        _refuse(who, "cfg.topology must be WATER_MATRIX or ICE_MATRIX")
    return _BrightBandCfg(ew.real, ew.imag, vals["eps_i"], vals["rho_w"], vals["rho_i"], vals["kw2"], int(cfg.topology))


def _wanted(who, want):
    if isinstance(want, str):
        want = (want,)
    try:
        want = tuple(want)
    except TypeError:
        _refuse(who, "want must be a name or a sequence of names out of %s" % (BRIGHTBAND_NAMES,))
    for n in want:
        if n not in BRIGHTBAND_NAMES:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, BRIGHTBAND_NAMES))
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
        if x not in BRIGHTBAND_SPECIES:
            _refuse(who, "unknown species %r in grids: out of %s" % (x, BRIGHTBAND_SPECIES))
        if g is None:
            continue
        if not (isinstance(g, (tuple, list)) and len(g) == 2 and is_array(g[0]) and is_array(g[1])):
            _refuse(who, "grids[%r] must be a pair (D, dD) of arrays" % x)
        D, dD = g
        if len(D.shape) != 1 or not 1 <= D.shape[0] <= BRIGHTBAND_MAX_BINS:
            _refuse(who, "grids[%r]: D must be one-dimensional with 1 to %d bins" % (x, BRIGHTBAND_MAX_BINS))
        nb[x] = int(D.shape[0])
        check(D, "grids[%r] D" % x, nb[x])
        check(dD, "grids[%r] dD" % x, nb[x])
    return nb


def _call(fn, model, ncol, nz, ptrs, cfg, grids, nb, addr, res, *stream):
    o = _BrightBandOut(**{n: addr(a) for n, a in res.items()})
    g = _BrightBandGrids()
    for i, x in enumerate(BRIGHTBAND_SPECIES):
        if x in nb:
            g.D[i], g.dD[i], g.nb[i] = addr(grids[x][0]), addr(grids[x][1]), nb[x]
    rc = fn(model._h, ncol, nz, *ptrs, C.byref(cfg) if cfg is not None else None, C.byref(g), C.byref(o), *stream)
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, library().kidmp_last_error(model._h).decode()))


def _results(who, want, out, shapes, dtypes, check, fresh):
    if out is not None and not isinstance(out, dict):
        _refuse(who, "out must be a dict name -> array")
    res = {}
    for n in want:
        if out is not None and out.get(n) is not None:
            check(out[n], "out[%r]" % n, shapes[n], dtypes[n])
            res[n] = out[n]
        else:
            res[n] = fresh(shapes[n], dtypes[n])
    return res


def bright_band(model, st, cfg=None, grids=None, want=("dbz",), out=None, stream=None):
    """The reflectivity with its melting layer of a device-resident state (kidmp[32]_bright_band_device): one launch.

    st      dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load), keys BRIGHTBAND_INPUTS; qs
            and qg may be missing (or None): zero
    cfg     None = the defaults, or a BrightBandCfg
    grids   None, or a dict species ("s", "g") -> (D, dD): float64 CUDA tensors [nb], 1 <= nb <= BRIGHTBAND_MAX_BINS, bin
            diameters and widths in m; a species without an entry is put on the scheme's own 100 bins
    want    names out of BRIGHTBAND_NAMES: "dbz", "dbz_s", "dbz_g" in dBZ, "enh_s", "enh_g" the linear enhancement of
            snow's and graupel's reflectivity (exactly 1.0 where dry), "fmelt_s", "fmelt_g" the melt fractions, all
            [ncol, nz]; "k0" the melting level, int32 [ncol], -1 where the column has none
    out     None, or a dict name -> tensor of the result's shape and dtype to write into instead of a fresh one
    Returns a dict name -> tensor.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    who = "bright_band"
    if not isinstance(st, dict) or not isinstance(st.get("t"), torch.Tensor):
        _refuse(who, "the state must be a dict of torch tensors with the keys %s" % (BRIGHTBAND_INPUTS,))
    q = st["t"]
    if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 tensors [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = int(q.shape[0]), int(q.shape[1])
    want = _wanted(who, want)
    ccfg = _config(who, cfg)

    def check(a, k, shape=(ncol, nz), dtype=q.dtype):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        model._want(a, dtype, shape, who + ": ", k)

    ptrs = _th._pointers(st, BRIGHTBAND_INPUTS, _OPTIONAL, check, torch.Tensor.data_ptr)
    nb = _grid_sizes(who, grids, lambda a: isinstance(a, torch.Tensor), lambda a, k, n: check(a, k, (n,), torch.float64))
    shapes = {n: (ncol,) if n == "k0" else (ncol, nz) for n in want}
    dtypes = {n: torch.int32 if n == "k0" else q.dtype for n in want}
    res = _results(who, want, out, shapes, dtypes, check, lambda s, d: torch.empty(s, dtype=d, device=q.device))
    L = library()
    fn = L.kidmp_bright_band_device if q.dtype == torch.float64 else L.kidmp32_bright_band_device
    _call(fn, model, ncol, nz, ptrs, ccfg, grids, nb, torch.Tensor.data_ptr, res, _th._stream(stream, q))
    return res


def bright_band_host(model, st, cfg=None, grids=None, want=("dbz",), out=None):
    """bright_band on numpy arrays [ncol, nz] (float64 or float32; grids float64 numpy arrays): chunks of columns through
    the context's staging memory (kidmp[32]_bright_band_host); only what `want` names comes back over PCIe.  Returns
    numpy arrays, bit for bit what bright_band gives."""
    who = "bright_band_host"
    if not isinstance(st, dict) or not isinstance(st.get("t"), np.ndarray):
        _refuse(who, "the state must be a dict of numpy arrays with the keys %s" % (BRIGHTBAND_INPUTS,))
    q = st["t"]
    if q.dtype not in (np.float64, np.float32) or q.ndim != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 arrays [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = q.shape
    want = _wanted(who, want)
    ccfg = _config(who, cfg)

    def check(a, k, shape=(ncol, nz), dtype=q.dtype):
        if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and a.shape == tuple(shape)):
            _refuse(who, "%s must be a contiguous %s array %s" % (k, np.dtype(dtype).name, list(shape)))

    addr = lambda a: a.ctypes.data   # noqa: E731
    ptrs = _th._pointers(st, BRIGHTBAND_INPUTS, _OPTIONAL, check, addr)
    nb = _grid_sizes(who, grids, lambda a: isinstance(a, np.ndarray), lambda a, k, n: check(a, k, (n,), np.float64))
    shapes = {n: (ncol,) if n == "k0" else (ncol, nz) for n in want}
    dtypes = {n: np.int32 if n == "k0" else q.dtype for n in want}
    res = _results(who, want, out, shapes, dtypes, check, lambda s, d: np.empty(s, dtype=d))
    L = library()
    fn = L.kidmp_bright_band_host if q.dtype == np.float64 else L.kidmp32_bright_band_host
    _call(fn, model, ncol, nz, ptrs, ccfg, grids, nb, addr, res)
    return res
