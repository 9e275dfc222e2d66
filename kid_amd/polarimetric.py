"""A polarimetric radar operator on the device (include/kidmp_polarimetric.h): differential reflectivity Z_DR, specific
differential phase K_DP and the co-polar correlation rho_hv of oblate spheroids in the Rayleigh-Gans approximation -- a
table of seven numbers per diameter bin built once on the host (PolTable), folded into the scheme's size distributions in
one launch per call (polarimetric).

The particle models, the canting moments and the definitions are the project's own; parity with an instrument simulator is
unpinned, and the defaults of PolCfg are illustrative, not values of record.  The table takes the wavelength, the
permittivities and the densities from a kid_amd.mie.MieCfg (kw2 is not read).

The entries of kidmp_polarimetric.h are declared here, on the object load_library() returned, the first time one of them
is needed.  There is no fallback: without the library a call raises KidmpError; pol_spheroid and pol_bins need the library
but no device.
"""
import ctypes as C
import math

import numpy as np

from . import mie as _mie
from . import thompson as _th
from .mie import MIE_MAX_BINS, MIE_SPECIES, MieCfg, _MieCfg, _MieGrids
from .thompson import KidmpError

POL_NAMES = ("dbz_h", "zdr", "kdp", "rhohv", "dbz_h_r", "dbz_h_s", "dbz_h_g", "zdr_r", "zdr_s", "zdr_g", "kdp_r", "kdp_s",
             "kdp_g")                                           # kidmp_pol_out
POL_ROWS = ("s_h", "s_v", "c_re", "c_im", "s_0", "k", "mass")   # the rows of a table, KIDMP_POL_NROWS
POL_SCALARS = ("s_h/s_0", "s_v/s_0", "c_re/s_0", "c_im/s_0", "k/mass")   # of a uniform species, KIDMP_POL_NSCALARS
POL_INPUTS = ("t", "p", "qv", "qr", "nr", "qs", "qg")
_OPTIONAL = ("qs", "qg")                                        # left out (or None) = zero, in any context
_NSPEC = len(MIE_SPECIES)


class _PolCfg(C.Structure):
    """kidmp_pol_cfg."""
    _fields_ = [("axis_r", C.c_double * 5), ("axis_r_min", C.c_double), ("axis_s", C.c_double), ("axis_g", C.c_double),
                ("sigma", C.c_double * _NSPEC), ("force_quadrature", C.c_int32)]


class _PolOut(C.Structure):
    """kidmp_pol_out / kidmp32_pol_out: thirteen profile pointers."""
    _fields_ = [(n, C.c_void_p) for n in POL_NAMES]


class PolCfg:
    """The shapes and orientations of a table; what is not given keeps the value kidmp_pol_defaults writes.  These defaults
    are illustrative, not values of record.

    axis_r            five coefficients of rain's axis ratio in d = D*1e3 (mm): clamp(c0 + d (c1 + d (c2 + d (c3 + d c4))),
                      axis_r_min, 1); default Brandes et al. (2002)
    axis_s, axis_g    the constant axis ratios of snow and graupel, in (0, 1]
    sigma             the widths of the canting-angle distributions of rain, snow and graupel in radians, >= 0
    force_quadrature  True: no species is taken as uniform, every one walks its bins"""

    def __init__(self, axis_r=(0.9951, 0.02510, -0.03644, 0.005303, -0.0002492), axis_r_min=0.2, axis_s=0.75, axis_g=0.8,
                 sigma=(math.radians(10.0), math.radians(40.0), math.radians(40.0)), force_quadrature=False):
        self.axis_r, self.axis_r_min, self.axis_s, self.axis_g = tuple(axis_r), axis_r_min, axis_s, axis_g
        self.sigma, self.force_quadrature = tuple(sigma), bool(force_quadrature)


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_polarimetric.h."""
    i32, i64, vp, rc, dbl = C.c_int32, C.c_int64, C.c_void_p, C.c_int, C.c_double
    pm, pp = C.POINTER(_MieCfg), C.POINTER(_PolCfg)
    host = [vp, vp, i64, i32] + [vp] * 7 + [C.POINTER(_PolOut)]
    return {
        "kidmp_pol_defaults": (None, [pp]),
        "kidmp_pol_spheroid": (rc, [dbl, dbl, dbl, dbl, vp]),
        "kidmp_pol_bins": (rc, [pm, pp, i32, i32, vp, vp]),
        "kidmp_pol_table_create": (rc, [vp, pm, pp, C.POINTER(_MieGrids), C.POINTER(vp)]),
        "kidmp_pol_table_destroy": (None, [vp]),
        "kidmp_pol_table_get": (rc, [vp, i32, C.POINTER(i32), vp, vp, vp, pm, pp, C.POINTER(i32), vp]),
        "kidmp_polarimetric_device": (rc, host + [vp]),
        "kidmp32_polarimetric_device": (rc, host + [vp]),
        "kidmp_polarimetric_host": (rc, host),
        "kidmp32_polarimetric_host": (rc, host),
    }


def declare(L):
    """Declare the entries of kidmp_polarimetric.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the entries of kidmp_polarimetric.h declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _refuse(who, msg):
    raise KidmpError("%s: %s" % (who, msg))


def _raise(rc, handle=None):
    raise KidmpError("kidmp error %d: %s" % (rc, library().kidmp_last_error(handle).decode()))


def _pol_config(who, cfg):
    """The kidmp_pol_cfg of a PolCfg (None: the defaults), refused here where the library would refuse it."""
    if cfg is None:
        cfg = PolCfg()
    if not isinstance(cfg, PolCfg):
        _refuse(who, "pol_cfg must be a PolCfg or None")
    try:
        axis_r, sigma = [float(v) for v in cfg.axis_r], [float(v) for v in cfg.sigma]
        rmin, rs, rg = float(cfg.axis_r_min), float(cfg.axis_s), float(cfg.axis_g)
    except (TypeError, ValueError):
        _refuse(who, "the members of pol_cfg must be numbers")
    if len(axis_r) != 5 or len(sigma) != _NSPEC:
        _refuse(who, "pol_cfg: axis_r takes five coefficients and sigma one width per species %s" % (MIE_SPECIES,))
    if not all(math.isfinite(v) for v in axis_r + sigma + [rmin, rs, rg]):
        _refuse(who, "the members of pol_cfg must be finite")
    if not all(0.0 < v <= 1.0 for v in (rmin, rs, rg)):
        _refuse(who, "pol_cfg: axis_r_min, axis_s and axis_g must be in (0, 1]")
    if any(v < 0.0 for v in sigma):
        _refuse(who, "pol_cfg: sigma must not be below 0")
    return _PolCfg((C.c_double * 5)(*axis_r), rmin, rs, rg, (C.c_double * _NSPEC)(*sigma), 1 if cfg.force_quadrature else 0)


def pol_spheroid(eps, ratio, sigma):
    """The rows POL_ROWS of an oblate spheroid of unit equal-volume diameter, permittivity eps (complex, Im >= 0), axis
    ratio in (0, 1] and canting width sigma (radians): float64 [7], the mass +0.0 (kidmp_pol_spheroid): host code, no
    device."""
    eps = complex(eps)
    rows = np.empty(len(POL_ROWS), dtype=np.float64)
    rc = library().kidmp_pol_spheroid(eps.real, eps.imag, float(ratio), float(sigma), rows.ctypes.data)
    if rc < 0:
        _raise(rc)
    return rows


def pol_bins(mie_cfg, pol_cfg, species, D):
    """The seven rows POL_ROWS of `species` ("r", "s", "g") on the diameters D (m), float64 [7, nb] (kidmp_pol_bins): host
    code, no device."""
    who = "pol_bins"
    c = _mie._config(who, mie_cfg)
    p = _pol_config(who, pol_cfg)
    x = _mie._species(who, species)
    D = np.ascontiguousarray(D, dtype=np.float64)
    if D.ndim != 1 or D.shape[0] < 1:
        _refuse(who, "D must be one-dimensional with at least one diameter")
    rows = np.empty((len(POL_ROWS), D.shape[0]), dtype=np.float64)
    rc = library().kidmp_pol_bins(C.byref(c), C.byref(p), x, D.shape[0], D.ctypes.data, rows.ctypes.data)
    if rc < 0:
        _raise(rc)
    return rows


class PolTable:
    """The rows of rain, snow and graupel for one configuration, on the device of `model` (kidmp_pol_table_create).

    mie_cfg None = kidmp_mie_defaults (10 cm), or a MieCfg: wavelength, permittivities, densities
    pol_cfg None = kidmp_pol_defaults, or a PolCfg: axis ratios, canting widths, force_quadrature
    grids   None, or a dict species ("r", "s", "g") -> (D, dD): float64 numpy arrays [nb], 1 <= nb <= MIE_MAX_BINS, bin
            diameters and widths in m; a species without an entry is put on the scheme's own 100 bins
    The handle is freed by close(), on leaving a `with` block, or when the object is collected; free it before the model."""

    def __init__(self, model, mie_cfg=None, pol_cfg=None, grids=None):
        who = "PolTable"
        self._t = None
        self.model = model
        c = _mie._config(who, mie_cfg)
        p = _pol_config(who, pol_cfg)
        if grids is None:
            grids = {}
        if not isinstance(grids, dict):
            _refuse(who, "grids must be a dict species -> (D, dD)")
        g = _MieGrids()
        keep = []
        for x, pair in grids.items():
            i = _mie._species(who, x)
            if pair is None:
                continue
            if not (isinstance(pair, (tuple, list)) and len(pair) == 2 and all(isinstance(a, np.ndarray) for a in pair)):
                _refuse(who, "grids[%r] must be a pair (D, dD) of numpy arrays" % x)
            D, dD = pair
            if D.ndim != 1 or not 1 <= D.shape[0] <= MIE_MAX_BINS:
                _refuse(who, "grids[%r]: D must be one-dimensional with 1 to %d bins" % (x, MIE_MAX_BINS))
            for a, k in ((D, "D"), (dD, "dD")):
                if not (a.dtype == np.float64 and a.flags.c_contiguous and a.shape == D.shape):
                    _refuse(who, "grids[%r] %s must be a contiguous float64 array [%d]" % (x, k, D.shape[0]))
            keep += [D, dD]
            g.D[i], g.dD[i], g.nb[i] = D.ctypes.data, dD.ctypes.data, D.shape[0]
        h = C.c_void_p()
        rc = library().kidmp_pol_table_create(model._h, C.byref(c), C.byref(p), C.byref(g), C.byref(h))
        if rc < 0:
            _raise(rc, model._h)
        self._t = h

    def _get(self, who, x, *args):
        if self._t is None:
            _refuse(who, "the table is closed")
        rc = library().kidmp_pol_table_get(self._t, x, *args)
        if rc < 0:
            _raise(rc, self.model._h)

    def get(self, species):
        """(D, dD, rows, uniform, scalars) of a species as the device holds them: float64 [nb], [nb], [7, nb], whether the
        kernel takes the species as uniform, and its five POL_SCALARS (kidmp_pol_table_get)."""
        who = "PolTable.get"
        x = _mie._species(who, species)
        nb, uni = C.c_int32(), C.c_int32()
        self._get(who, x, C.byref(nb), None, None, None, None, None, None, None)
        D, dD, rows = np.empty(nb.value), np.empty(nb.value), np.empty((len(POL_ROWS), nb.value))
        scal = np.empty(len(POL_SCALARS))
        self._get(who, x, C.byref(nb), D.ctypes.data, dD.ctypes.data, rows.ctypes.data, None, None, C.byref(uni), scal.ctypes.data)
        return D, dD, rows, bool(uni.value), scal

    @property
    def cfg(self):
        """The configuration the table was built with, as a pair (MieCfg, PolCfg)."""
        c, p, nb = _MieCfg(), _PolCfg(), C.c_int32()
        self._get("PolTable.cfg", 0, C.byref(nb), None, None, None, C.byref(c), C.byref(p), None, None)
        return (MieCfg(c.wavelength, complex(c.eps_w_re, c.eps_w_im), complex(c.eps_i_re, c.eps_i_im), c.rho_w, c.rho_i, c.kw2),
                PolCfg(tuple(p.axis_r), p.axis_r_min, p.axis_s, p.axis_g, tuple(p.sigma), bool(p.force_quadrature)))

    def close(self):
        if self._t is not None:
            library().kidmp_pol_table_destroy(self._t)
            self._t = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:                                   # interpreter shutdown: the library may be gone
            pass


def _wanted(who, want):
    if isinstance(want, str):
        want = (want,)
    try:
        want = tuple(want)
    except TypeError:
        _refuse(who, "want must be a name or a sequence of names out of %s" % (POL_NAMES,))
    for n in want:
        if n not in POL_NAMES:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, POL_NAMES))
    if len(set(want)) != len(want):
        _refuse(who, "want names an output twice")
    if not want:
        _refuse(who, "nothing requested: want is empty")
    return want


def _table(who, model, table):
    if not isinstance(table, PolTable) or table._t is None:
        _refuse(who, "table must be an open PolTable")
    if table.model is not model:
        _refuse(who, "the table belongs to another context")
    return table._t


def _call(fn, model, table, ncol, nz, ptrs, addr, res, *stream):
    o = _PolOut(**{n: addr(a) for n, a in res.items()})
    rc = fn(model._h, table, ncol, nz, *ptrs, C.byref(o), *stream)
    if rc < 0:
        _raise(rc, model._h)


def polarimetric(model, table, st, want=("dbz_h", "zdr", "kdp", "rhohv"), out=None, stream=None):
    """The polarimetric radar of a device-resident state (kidmp[32]_polarimetric_device): one launch.

    table   a PolTable of this model
    st      dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load), keys POL_INPUTS; qs and qg
            may be missing (or None): zero
    want    names out of POL_NAMES: dbz_h the reflectivity at horizontal polarisation in dBZ, zdr the differential
            reflectivity in dB, kdp the specific differential phase in degrees per km, rhohv the co-polar correlation;
            dbz_h_x, zdr_x, kdp_x those of rain, snow and graupel alone; all [ncol, nz]
    out     None, or a dict name -> tensor of the result's shape and dtype to write into instead of a fresh one
    Returns a dict name -> tensor.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    who = "polarimetric"
    if not isinstance(st, dict) or not isinstance(st.get("t"), torch.Tensor):
        _refuse(who, "the state must be a dict of torch tensors with the keys %s" % (POL_INPUTS,))
    q = st["t"]
    if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 tensors [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = int(q.shape[0]), int(q.shape[1])
    want = _wanted(who, want)
    h = _table(who, model, table)

    def check(a, k, shape=(ncol, nz)):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        model._want(a, q.dtype, shape, who + ": ", k)

    ptrs = _th._pointers(st, POL_INPUTS, _OPTIONAL, check, torch.Tensor.data_ptr)
    shapes = {n: (ncol, nz) for n in want}
    res = _mie._results(who, want, out, shapes, q.dtype, check, lambda s, d: torch.empty(s, dtype=d, device=q.device))
    L = library()
    fn = L.kidmp_polarimetric_device if q.dtype == torch.float64 else L.kidmp32_polarimetric_device
    _call(fn, model, h, ncol, nz, ptrs, torch.Tensor.data_ptr, res, _th._stream(stream, q))
    return res


def polarimetric_host(model, table, st, want=("dbz_h", "zdr", "kdp", "rhohv"), out=None):
    """polarimetric on numpy arrays [ncol, nz] (float64 or float32): chunks of columns through the context's staging
    memory (kidmp[32]_polarimetric_host); only what `want` names comes back over PCIe.  Returns numpy arrays, bit for bit
    what polarimetric gives."""
    who = "polarimetric_host"
    if not isinstance(st, dict) or not isinstance(st.get("t"), np.ndarray):
        _refuse(who, "the state must be a dict of numpy arrays with the keys %s" % (POL_INPUTS,))
    q = st["t"]
    if q.dtype not in (np.float64, np.float32) or q.ndim != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 arrays [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = q.shape
    want = _wanted(who, want)
    h = _table(who, model, table)

    def check(a, k, shape=(ncol, nz)):
        if not (isinstance(a, np.ndarray) and a.dtype == q.dtype and a.flags.c_contiguous and a.shape == tuple(shape)):
            _refuse(who, "%s must be a contiguous %s array %s" % (k, q.dtype.name, list(shape)))

    addr = lambda a: a.ctypes.data   # noqa: E731
    ptrs = _th._pointers(st, POL_INPUTS, _OPTIONAL, check, addr)
    shapes = {n: (ncol, nz) for n in want}
    res = _mie._results(who, want, out, shapes, q.dtype, check, lambda s, d: np.empty(s, dtype=d))
    L = library()
    fn = L.kidmp_polarimetric_host if q.dtype == np.float64 else L.kidmp32_polarimetric_host
    _call(fn, model, h, ncol, nz, ptrs, addr, res)
    return res
