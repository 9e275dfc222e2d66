"""A cloud-radar operator on the device (include/kidmp_mie.h): Lorenz-Mie reflectivity, extinction, path-integrated
attenuation and mean Doppler velocity at a chosen wavelength -- a table of five numbers per diameter bin built once on the
host (MieTable), folded into the scheme's size distributions in one launch per call (mie_radar).

The particle models and the definitions are the project's own; parity with an instrument simulator is unpinned.  The
library holds no permittivities but the 10-cm ones of the bright band: a cloud-radar user passes the wavelength and the
permittivities of water and ice at that wavelength and temperature.

The entries of kidmp_mie.h are declared here, on the object load_library() returned, the first time one of them is
needed: include/kidmp.h and its mirror in thompson.py stay what they are.  There is no fallback: without the library a
call raises KidmpError; mie_sphere and mie_bins need the library but no device.
"""
import ctypes as C
import math

import numpy as np

from . import thompson as _th
from .thompson import KidmpError

MIE_NAMES = ("dbz", "dbz_up", "dbz_down", "dbz_r", "dbz_s", "dbz_g", "mie_r", "mie_s", "mie_g", "ext", "pia_up", "pia_down",
             "vd", "pia_total")                                 # kidmp_mie_out
MIE_SPECIES = ("r", "s", "g")                                   # rain, snow, graupel: kidmp_mie_grids
MIE_ROWS = ("s_mie", "s_ray", "s_ext", "mass", "v0")            # the rows of a table, KIDMP_MIE_NROWS
MIE_INPUTS = ("t", "p", "qv", "qc", "qr", "nr", "qs", "qg")
MIE_MAX_BINS = 256                                              # KIDMP_MIE_MAX_BINS
_OPTIONAL = ("qc", "qs", "qg")                                  # left out (or None) = zero, in any context
_PATH = ("dbz_up", "dbz_down", "pia_up", "pia_down", "pia_total")   # what needs dz
_NSPEC = len(MIE_SPECIES)


class _MieCfg(C.Structure):
    """kidmp_mie_cfg."""
    _fields_ = [(n, C.c_double) for n in ("wavelength", "eps_w_re", "eps_w_im", "eps_i_re", "eps_i_im", "rho_w", "rho_i", "kw2")]


class _MieOut(C.Structure):
    """kidmp_mie_out / kidmp32_mie_out: thirteen profile pointers and pia_total."""
    _fields_ = [(n, C.c_void_p) for n in MIE_NAMES]


class _MieGrids(C.Structure):
    """kidmp_mie_grids: D, dD and nb by species."""
    _fields_ = [("D", C.c_void_p * _NSPEC), ("dD", C.c_void_p * _NSPEC), ("nb", C.c_int32 * _NSPEC)]


def default_eps_i():
    """(1 + 2k)/(1 - k) with k = sqrt(0.176): the real permittivity of ice whose |K_i|**2 is the scheme's 0.176."""
    k = math.sqrt(0.176)
    return (1.0 + 2.0 * k) / (1.0 - k)


class MieCfg:
    """The configuration of a table; what is not given keeps the value kidmp_mie_defaults writes: wavelength in m, eps_w and
    eps_i the complex relative permittivities of water and ice (Im >= 0 marks absorption), rho_w and rho_i the densities
    (kg m-3), kw2 the normalisation of the reflectivity."""

    def __init__(self, wavelength=0.10, eps_w=complex(79.5, 24.9), eps_i=None, rho_w=1000.0, rho_i=900.0, kw2=0.93):
        self.wavelength, self.eps_w = wavelength, eps_w
        self.eps_i = complex(default_eps_i(), 0.0) if eps_i is None else eps_i
        self.rho_w, self.rho_i, self.kw2 = rho_w, rho_i, kw2


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_mie.h."""
    i32, i64, vp, rc, dbl = C.c_int32, C.c_int64, C.c_void_p, C.c_int, C.c_double
    pd = C.POINTER(C.c_double)
    host = [vp, vp, i64, i32] + [vp] * 8 + [vp, i64, vp, vp, i64, C.POINTER(_MieOut)]
    return {
        "kidmp_mie_defaults": (None, [C.POINTER(_MieCfg)]),
        "kidmp_mie_sphere": (rc, [dbl, dbl, dbl, pd, pd]),
        "kidmp_mie_bins": (rc, [C.POINTER(_MieCfg), i32, i32, vp, vp]),
        "kidmp_mie_table_create": (rc, [vp, C.POINTER(_MieCfg), C.POINTER(_MieGrids), C.POINTER(vp)]),
        "kidmp_mie_table_destroy": (None, [vp]),
        "kidmp_mie_table_get": (rc, [vp, i32, C.POINTER(i32), vp, vp, vp, C.POINTER(_MieCfg)]),
        "kidmp_mie_radar_device": (rc, host + [vp]),
        "kidmp32_mie_radar_device": (rc, host + [vp]),
        "kidmp_mie_radar_host": (rc, host),
        "kidmp32_mie_radar_host": (rc, host),
    }


def declare(L):
    """Declare the entries of kidmp_mie.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the entries of kidmp_mie.h declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _refuse(who, msg):
    raise KidmpError("%s: %s" % (who, msg))


def _config(who, cfg):
    """The kidmp_mie_cfg of a MieCfg (None: the defaults), refused here where the library would refuse it."""
    if cfg is None:
        cfg = MieCfg()
    if not isinstance(cfg, MieCfg):
        _refuse(who, "cfg must be a MieCfg or None")
    try:
        ew, ei = complex(cfg.eps_w), complex(cfg.eps_i)
        lam, rw, ri, kw2 = float(cfg.wavelength), float(cfg.rho_w), float(cfg.rho_i), float(cfg.kw2)
    except (TypeError, ValueError):
        _refuse(who, "the members of cfg must be numbers")
    vals = (lam, ew.real, ew.imag, ei.real, ei.imag, rw, ri, kw2)
    if not all(math.isfinite(v) for v in vals):
        _refuse(who, "the members of cfg must be finite")
    if not (lam > 0.0 and rw > 0.0 and ri > 0.0 and kw2 > 0.0):
        _refuse(who, "cfg: wavelength, rho_w, rho_i and kw2 must be above 0")
    if ew.imag < 0.0 or ei.imag < 0.0:
        _refuse(who, "cfg: Im(eps) must not be below 0")
    if (ew.imag == 0.0 and not ew.real > 0.0) or (ei.imag == 0.0 and not ei.real > 0.0):
        _refuse(who, "cfg: a real permittivity must be above 0")
    return _MieCfg(*vals)


def _raise(rc, handle=None):
    raise KidmpError("kidmp error %d: %s" % (rc, library().kidmp_last_error(handle).decode()))


def mie_sphere(x, m):
    """(Q_ext, Q_back) of a homogeneous sphere of size parameter x and complex refractive index m = n + ik, k >= 0, by the
    Lorenz-Mie series of the library (kidmp_mie_sphere): host code, no device."""
    m = complex(m)
    qe, qb = C.c_double(), C.c_double()
    rc = library().kidmp_mie_sphere(float(x), m.real, m.imag, C.byref(qe), C.byref(qb))
    if rc < 0:
        _raise(rc)
    return qe.value, qb.value


def _species(who, species):
    if species not in MIE_SPECIES:
        _refuse(who, "unknown species %r: out of %s" % (species, MIE_SPECIES))
    return MIE_SPECIES.index(species)


def mie_bins(cfg, species, D):
    """The five rows MIE_ROWS of `species` ("r", "s", "g") on the diameters D (m), float64 [5, nb] (kidmp_mie_bins): host
    code, no device."""
    who = "mie_bins"
    c = _config(who, cfg)
    x = _species(who, species)
    D = np.ascontiguousarray(D, dtype=np.float64)
    if D.ndim != 1 or D.shape[0] < 1:
        _refuse(who, "D must be one-dimensional with at least one diameter")
    rows = np.empty((len(MIE_ROWS), D.shape[0]), dtype=np.float64)
    rc = library().kidmp_mie_bins(C.byref(c), x, D.shape[0], D.ctypes.data, rows.ctypes.data)
    if rc < 0:
        _raise(rc)
    return rows


class MieTable:
    """The rows of rain, snow and graupel for one configuration, on the device of `model` (kidmp_mie_table_create).

    cfg     None = the defaults (10 cm), or a MieCfg
    grids   None, or a dict species ("r", "s", "g") -> (D, dD): float64 numpy arrays [nb], 1 <= nb <= MIE_MAX_BINS, bin
            diameters and widths in m; a species without an entry is put on the scheme's own 100 bins
    The handle is freed by close(), on leaving a `with` block, or when the object is collected; free it before the model."""

    def __init__(self, model, cfg=None, grids=None):
        who = "MieTable"
        self._t = None
        self.model = model
        c = _config(who, cfg)
        if grids is None:
            grids = {}
        if not isinstance(grids, dict):
            _refuse(who, "grids must be a dict species -> (D, dD)")
        g = _MieGrids()
        keep = []
        for x, pair in grids.items():
            i = _species(who, x)
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
        rc = library().kidmp_mie_table_create(model._h, C.byref(c), C.byref(g), C.byref(h))
        if rc < 0:
            _raise(rc, model._h)
        self._t = h

    def get(self, species):
        """(D, dD, rows) of a species as the device holds them: float64 [nb], [nb], [5, nb] (kidmp_mie_table_get)."""
        who = "MieTable.get"
        if self._t is None:
            _refuse(who, "the table is closed")
        x = _species(who, species)
        L = library()
        nb = C.c_int32()
        rc = L.kidmp_mie_table_get(self._t, x, C.byref(nb), None, None, None, None)
        if rc < 0:
            _raise(rc, self.model._h)
        D, dD, rows = np.empty(nb.value), np.empty(nb.value), np.empty((len(MIE_ROWS), nb.value))
        rc = L.kidmp_mie_table_get(self._t, x, C.byref(nb), D.ctypes.data, dD.ctypes.data, rows.ctypes.data, None)
        if rc < 0:
            _raise(rc, self.model._h)
        return D, dD, rows

    @property
    def cfg(self):
        """The configuration the table was built with, as a MieCfg."""
        if self._t is None:
            _refuse("MieTable.cfg", "the table is closed")
        c, nb = _MieCfg(), C.c_int32()
        rc = library().kidmp_mie_table_get(self._t, 0, C.byref(nb), None, None, None, C.byref(c))
        if rc < 0:
            _raise(rc, self.model._h)
        return MieCfg(c.wavelength, complex(c.eps_w_re, c.eps_w_im), complex(c.eps_i_re, c.eps_i_im), c.rho_w, c.rho_i, c.kw2)

    def close(self):
        if self._t is not None:
            library().kidmp_mie_table_destroy(self._t)
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
        _refuse(who, "want must be a name or a sequence of names out of %s" % (MIE_NAMES,))
    for n in want:
        if n not in MIE_NAMES:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, MIE_NAMES))
    if len(set(want)) != len(want):
        _refuse(who, "want names an output twice")
    if not want:
        _refuse(who, "nothing requested: want is empty")
    return want


def _table(who, model, table):
    if not isinstance(table, MieTable) or table._t is None:
        _refuse(who, "table must be an open MieTable")
    if table.model is not model:
        _refuse(who, "the table belongs to another context")
    return table._t


def _stride(who, a, name, shape, ncol, nz):
    if a is None:
        return 0
    if tuple(shape) == (nz,):
        return 0
    if tuple(shape) == (ncol, nz):
        return nz
    _refuse(who, "%s must be [nz] = [%d] or [ncol, nz] = [%d, %d], got %s" % (name, nz, ncol, nz, list(shape)))


def _call(fn, model, table, ncol, nz, ptrs, dz, dz_stride, w, k_gas, kg_stride, addr, res, *stream):
    o = _MieOut(**{n: addr(a) for n, a in res.items()})
    rc = fn(model._h, table, ncol, nz, *ptrs, dz, dz_stride, w, k_gas, kg_stride, C.byref(o), *stream)
    if rc < 0:
        _raise(rc, model._h)


def _results(who, want, out, shapes, dtype, check, fresh):
    if out is not None and not isinstance(out, dict):
        _refuse(who, "out must be a dict name -> array")
    res = {}
    for n in want:
        if out is not None and out.get(n) is not None:
            check(out[n], "out[%r]" % n, shapes[n])
            res[n] = out[n]
        else:
            res[n] = fresh(shapes[n], dtype)
    return res


def mie_radar(model, table, st, dz=None, w=None, k_gas=None, want=("dbz",), out=None, stream=None):
    """The cloud radar of a device-resident state (kidmp[32]_mie_radar_device): one launch.

    table   a MieTable of this model
    st      dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load), keys MIE_INPUTS; qc, qs and
            qg may be missing (or None): zero
    dz      layer depths in m, [nz] or [ncol, nz], of the state's dtype; needed for dbz_up, dbz_down, pia_up, pia_down and
            pia_total
    w       None (zero) or the vertical air velocity [ncol, nz], positive upwards; vd is positive downwards
    k_gas   None (zero) or the one-way gas extinction in 1/m, [nz] or [ncol, nz]
    want    names out of MIE_NAMES: dbz, dbz_r, dbz_s, dbz_g the Mie reflectivities in dBZ; dbz_up, dbz_down those a
            ground-based and a space-borne radar record behind the two-way attenuation pia_up, pia_down (dB); mie_r, mie_s,
            mie_g the linear ratios to the Rayleigh reflectivity (exactly 1.0 where the species is absent); ext the one-way
            extinction (1/m); vd the mean Doppler velocity; all [ncol, nz]; pia_total [ncol], the two-way attenuation of
            the whole column
    out     None, or a dict name -> tensor of the result's shape and dtype to write into instead of a fresh one
    Returns a dict name -> tensor.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    who = "mie_radar"
    if not isinstance(st, dict) or not isinstance(st.get("t"), torch.Tensor):
        _refuse(who, "the state must be a dict of torch tensors with the keys %s" % (MIE_INPUTS,))
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

    ptrs = _th._pointers(st, MIE_INPUTS, _OPTIONAL, check, torch.Tensor.data_ptr)
    for a, k in ((dz, "dz"), (w, "w"), (k_gas, "k_gas")):
        if a is not None and not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
    if dz is None and any(n in _PATH for n in want):
        _refuse(who, "dz is needed for %s" % (_PATH,))
    dz_stride = _stride(who, dz, "dz", () if dz is None else dz.shape, ncol, nz)
    kg_stride = _stride(who, k_gas, "k_gas", () if k_gas is None else k_gas.shape, ncol, nz)
    for a, k in ((dz, "dz"), (k_gas, "k_gas")):
        if a is not None:
            check(a, k, tuple(a.shape))
    if w is not None:
        check(w, "w")
    shapes = {n: (ncol,) if n == "pia_total" else (ncol, nz) for n in want}
    res = _results(who, want, out, shapes, q.dtype, check, lambda s, d: torch.empty(s, dtype=d, device=q.device))
    L = library()
    fn = L.kidmp_mie_radar_device if q.dtype == torch.float64 else L.kidmp32_mie_radar_device
    ptr = lambda a: None if a is None else a.data_ptr()   # noqa: E731
    _call(fn, model, h, ncol, nz, ptrs, ptr(dz), dz_stride, ptr(w), ptr(k_gas), kg_stride, torch.Tensor.data_ptr, res, _th._stream(stream, q))
    return res


def mie_radar_host(model, table, st, dz=None, w=None, k_gas=None, want=("dbz",), out=None):
    """mie_radar on numpy arrays [ncol, nz] (float64 or float32): chunks of columns through the context's staging memory
    (kidmp[32]_mie_radar_host); only what `want` names comes back over PCIe.  Returns numpy arrays, bit for bit what
    mie_radar gives."""
    who = "mie_radar_host"
    if not isinstance(st, dict) or not isinstance(st.get("t"), np.ndarray):
        _refuse(who, "the state must be a dict of numpy arrays with the keys %s" % (MIE_INPUTS,))
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
    ptrs = _th._pointers(st, MIE_INPUTS, _OPTIONAL, check, addr)
    for a, k in ((dz, "dz"), (w, "w"), (k_gas, "k_gas")):
        if a is not None and not isinstance(a, np.ndarray):
            _refuse(who, "%s must be a numpy array, got %s" % (k, type(a).__name__))
    if dz is None and any(n in _PATH for n in want):
        _refuse(who, "dz is needed for %s" % (_PATH,))
    dz_stride = _stride(who, dz, "dz", () if dz is None else dz.shape, ncol, nz)
    kg_stride = _stride(who, k_gas, "k_gas", () if k_gas is None else k_gas.shape, ncol, nz)
    for a, k in ((dz, "dz"), (k_gas, "k_gas")):
        if a is not None:
            check(a, k, a.shape)
    if w is not None:
        check(w, "w")
    shapes = {n: (ncol,) if n == "pia_total" else (ncol, nz) for n in want}
    res = _results(who, want, out, shapes, q.dtype, check, lambda s, d: np.empty(s, dtype=d))
    L = library()
    fn = L.kidmp_mie_radar_host if q.dtype == np.float64 else L.kidmp32_mie_radar_host
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    _call(fn, model, h, ncol, nz, ptrs, ptr(dz), dz_stride, ptr(w), ptr(k_gas), kg_stride, addr, res)
    return res
