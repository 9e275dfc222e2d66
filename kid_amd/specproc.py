"""Doppler-spectrum processing on the device (include/kidmp_specproc.h): turbulent and beam broadening of a spectrum
[ncol, nv, nz] by a Gaussian whose width differs per level, a noise floor, detection and the moments of what is detected
(reflectivity, mean velocity, width, skewness, kurtosis, the edges and the number of detected bins), in one launch per call
(spectrum_process).  It serves the spectra of doppler_spectrum and any other spectrum on a uniform velocity grid.

The definitions are the project's own and parity with an instrument simulator is unpinned.  Not modelled: random noise
realisations, spectral averaging, peak separation, aliasing or folding, non-uniform grids.

The entries of kidmp_specproc.h are declared here, on the object load_library() returned, the first time one of them is
needed.  There is no fallback: without the library or the device a call raises KidmpError.
"""
import ctypes as C
import math

from . import thompson as _th
from .dspectrum import _grid
from .thompson import KidmpError

SPECPROC_NAMES = ("spec", "lost_below", "lost_above", "dbz", "vm", "sw", "skew", "kurt", "v_lo", "v_hi", "nbins")   # kidmp_specproc_out
SPECPROC_MAX_NV = 256                                           # KIDMP_SPECPROC_MAX_NV
SPECPROC_MAX_HALF = 256                                         # KIDMP_SPECPROC_MAX_HALF
_MOMENTS = SPECPROC_NAMES[3:]


class _SpecCfg(C.Structure):
    """kidmp_specproc_cfg."""
    _fields_ = [("cut", C.c_double), ("snr_min", C.c_double), ("add_noise", C.c_int32)]


class _SpecOut(C.Structure):
    """kidmp_specproc_out / kidmp32_specproc_out: ten value pointers and nbins."""
    _fields_ = [(n, C.c_void_p) for n in SPECPROC_NAMES]


class SpecCfg:
    """The configuration of spectrum_process: the broadening window reaches `cut` standard deviations (at most
    SPECPROC_MAX_HALF bins) to either side; bin j is detected where its signal exceeds snr_min times the level's noise;
    add_noise adds the level's noise to every bin of the returned spectrum."""

    def __init__(self, cut=4.0, snr_min=1.0, add_noise=False):
        self.cut, self.snr_min, self.add_noise = cut, snr_min, add_noise


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_specproc.h."""
    i32, i64, vp, rc, d = C.c_int32, C.c_int64, C.c_void_p, C.c_int, C.c_double
    entry = [vp, i64, i32, vp, d, d, i32, vp, i32, vp, i32, C.POINTER(_SpecCfg), C.POINTER(_SpecOut), vp]
    return {"kidmp_spectrum_process_device": (rc, entry), "kidmp32_spectrum_process_device": (rc, entry)}


def declare(L):
    """Declare the entries of kidmp_specproc.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the entries of kidmp_specproc.h declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _refuse(who, msg):
    raise KidmpError("%s: %s" % (who, msg))


def _config(who, cfg):
    """The kidmp_specproc_cfg of a SpecCfg (None: the defaults), refused here where the library would refuse it."""
    if cfg is None:
        cfg = SpecCfg()
    if not isinstance(cfg, SpecCfg):
        _refuse(who, "cfg must be a SpecCfg")
    try:
        cut, snr_min = float(cfg.cut), float(cfg.snr_min)
    except (TypeError, ValueError):
        _refuse(who, "the members of cfg must be numbers")
    if not (cut > 0.0 and math.isfinite(cut)):
        _refuse(who, "cfg: cut must be finite and above 0")
    if not (snr_min >= 0.0 and math.isfinite(snr_min)):
        _refuse(who, "cfg: snr_min must be finite and not below 0")
    return _SpecCfg(cut, snr_min, 1 if cfg.add_noise else 0)


def _wanted(who, want):
    if isinstance(want, str):
        want = (want,)
    try:
        want = tuple(want)
    except TypeError:
        _refuse(who, "want must be a name or a sequence of names out of %s" % (SPECPROC_NAMES,))
    for n in want:
        if n not in SPECPROC_NAMES:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, SPECPROC_NAMES))
    if len(set(want)) != len(want):
        _refuse(who, "want names an output twice")
    if not want:
        _refuse(who, "nothing requested: want is empty")
    return want


def spectrum_process(model, spec, v0, dv, sigma=None, noise=None, cfg=None, want=_MOMENTS, out=None, stream=None):
    """Broadening, noise floor, detection and moments of device-resident spectra (kidmp[32]_spectrum_process_device): one
    launch, no allocation beyond the results, no synchronisation.

    spec    CUDA tensor [ncol, nv, nz], float64 or float32 (widened on load), m6 m-3 per bin: doppler_spectrum's `total`
            or any other spectrum on the grid v0 + j*dv (1 <= nv <= SPECPROC_MAX_NV, velocities positive downward)
    sigma   None = no broadening, or the standard deviation of the broadening in m s-1, [nz] (shared by the columns) or
            [ncol, nz], of spec's dtype; a value that is not above 0 leaves its level as it is
    noise   None = 0, or the mean noise per velocity bin in the units of spec, [nz] or [ncol, nz]
    cfg     None = SpecCfg(), or a SpecCfg
    want    names out of SPECPROC_NAMES: spec the broadened spectrum [ncol, nv, nz] (plus the noise with add_noise);
            lost_below, lost_above what the broadening carried off the grid; dbz, vm, sw, skew, kurt the moments over the
            detected bins; v_lo, v_hi the centres of the first and last detected bin; nbins (int32) their number; all
            [ncol, nz].  What is not named costs no store: the default is the moments without the spectrum.
    out     None, or the dict an earlier call returned (or name -> tensor of the result's shape and dtype): rewritten in
            place, nothing is allocated
    Returns a dict name -> tensor.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    who = "spectrum_process"
    if not isinstance(spec, torch.Tensor) or spec.dtype not in (torch.float64, torch.float32) or spec.dim() != 3 \
            or not 2 <= spec.shape[2] <= _th.MAX_NZ:
        _refuse(who, "spec must be a float64 or float32 CUDA tensor [ncol, nv, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nv, nz = (int(n) for n in spec.shape)
    if not 1 <= nv <= SPECPROC_MAX_NV:
        _refuse(who, "nv must be in [1, %d], got %d" % (SPECPROC_MAX_NV, nv))
    v0, dv, nv = _grid(who, v0, dv, nv)
    c_cfg = _config(who, cfg)
    want = _wanted(who, want)

    def check(a, k, shape, dtype=spec.dtype):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        model._want(a, dtype, shape, who + ": ", k)

    check(spec, "spec", (ncol, nv, nz))
    stride = {}
    for k, a in (("sigma", sigma), ("noise", noise)):
        stride[k] = 0
        if a is not None:
            per_column = isinstance(a, torch.Tensor) and a.dim() == 2
            check(a, k, (ncol, nz) if per_column else (nz,))
            stride[k] = nz if per_column else 0
    if out is not None and not isinstance(out, dict):
        _refuse(who, "out must be a dict name -> tensor")
    res = {}
    for n in want:
        shape = (ncol, nv, nz) if n == "spec" else (ncol, nz)
        dtype = torch.int32 if n == "nbins" else spec.dtype
        if out is not None and out.get(n) is not None:
            check(out[n], "out[%r]" % n, shape, dtype)
            res[n] = out[n]
        else:
            res[n] = torch.empty(shape, dtype=dtype, device=spec.device)
    o = _SpecOut(**{n: a.data_ptr() for n, a in res.items()})
    L = library()
    fn = L.kidmp_spectrum_process_device if spec.dtype == torch.float64 else L.kidmp32_spectrum_process_device
    rc = fn(model._h, ncol, nz, spec.data_ptr(), v0, dv, nv, None if sigma is None else sigma.data_ptr(), stride["sigma"],
            None if noise is None else noise.data_ptr(), stride["noise"], C.byref(c_cfg), C.byref(o), _th._stream(stream, spec))
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, L.kidmp_last_error(model._h).decode()))
    return res
