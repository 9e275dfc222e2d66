"""A passive microwave radiometer on the device (include/kidmp_radiometer.h): two-stream brightness temperatures at a
chosen wavelength, looking up from the ground or down from orbit -- a table of three numbers per diameter bin built once
on the host (RadiometerTable), folded into the scheme's size distributions, turned into a two-stream layer per level and
added up by two wave scans in one launch per call (radiometer).

The particle models and the definitions are the project's own; parity with an instrument simulator is unpinned.  The
configuration of a table is the cloud radar's MieCfg (kw2 is not read); the caller passes the permittivities of water and
ice at the wavelength, and any gas absorption as the profile k_gas.

The entries of kidmp_radiometer.h are declared here, on the object load_library() returned, the first time one of them
is needed.  There is no fallback: without the library a call raises KidmpError; radiometer_sphere and radiometer_bins
need the library but no device.
"""
import ctypes as C
import math

import numpy as np

from . import thompson as _th
from .mie import MIE_INPUTS, MIE_MAX_BINS, MieCfg, _MieCfg, _MieGrids, _config, _refuse, _results, _species, _stride
from .thompson import KidmpError

RADIOMETER_NAMES = ("k_abs", "k_bsc", "refl", "trans", "tb_up", "tb_down", "tb_toa", "tb_ground", "tau_abs")   # kidmp_radiometer_out
RADIOMETER_SUMMARY_NAMES = ("tb_toa", "tb_ground", "tau_abs")   # [ncol]; the others are [ncol, nz]
RADIOMETER_ROWS = ("s_abs", "s_bsc", "mass")                    # the rows of a table, KIDMP_RADIOMETER_NROWS
RADIOMETER_INPUTS = MIE_INPUTS
_OPTIONAL = ("qc", "qs", "qg")                                  # left out (or None) = zero, in any context
_NO_DZ = ("k_abs", "k_bsc")                                     # what needs no dz


class _RadiometerCfg(C.Structure):
    """kidmp_radiometer_cfg."""
    _fields_ = [(n, C.c_double) for n in ("mu", "emissivity", "t_cosmic")]


class _RadiometerOut(C.Structure):
    """kidmp_radiometer_out / kidmp32_radiometer_out: six profile pointers and three per column."""
    _fields_ = [(n, C.c_void_p) for n in RADIOMETER_NAMES]


class RadiometerCfg:
    """What a call takes beside the table; what is not given keeps the value kidmp_radiometer_defaults writes: mu the
    cosine of the two streams in (0, 1], emissivity of the surface in [0, 1], t_cosmic the brightness temperature of
    space in K."""

    def __init__(self, mu=1.0, emissivity=1.0, t_cosmic=2.725):
        self.mu, self.emissivity, self.t_cosmic = mu, emissivity, t_cosmic


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_radiometer.h."""
    i32, i64, vp, rc, dbl = C.c_int32, C.c_int64, C.c_void_p, C.c_int, C.c_double
    pd = C.POINTER(C.c_double)
    host = [vp, vp, C.POINTER(_RadiometerCfg), i64, i32] + [vp] * 8 + [vp, i64, vp, i64, vp, C.POINTER(_RadiometerOut)]
    return {
        "kidmp_radiometer_defaults": (None, [C.POINTER(_RadiometerCfg)]),
        "kidmp_radiometer_sphere": (rc, [dbl, dbl, dbl, pd, pd, pd, pd]),
        "kidmp_radiometer_bins": (rc, [C.POINTER(_MieCfg), i32, i32, vp, vp]),
        "kidmp_radiometer_table_create": (rc, [vp, C.POINTER(_MieCfg), C.POINTER(_MieGrids), C.POINTER(vp)]),
        "kidmp_radiometer_table_destroy": (None, [vp]),
        "kidmp_radiometer_table_get": (rc, [vp, i32, C.POINTER(i32), vp, vp, vp, C.POINTER(_MieCfg)]),
        "kidmp_radiometer_device": (rc, host + [vp]),
        "kidmp32_radiometer_device": (rc, host + [vp]),
        "kidmp_radiometer_host": (rc, host),
        "kidmp32_radiometer_host": (rc, host),
    }


def declare(L):
    """Declare the entries of kidmp_radiometer.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the entries of kidmp_radiometer.h declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _raise(rc, handle=None):
    raise KidmpError("kidmp error %d: %s" % (rc, library().kidmp_last_error(handle).decode()))


def _rcfg(who, rcfg):
    """The kidmp_radiometer_cfg of a RadiometerCfg (None: the defaults), refused here where the library would refuse it."""
    if rcfg is None:
        rcfg = RadiometerCfg()
    if not isinstance(rcfg, RadiometerCfg):
        _refuse(who, "rcfg must be a RadiometerCfg or None")
    try:
        mu, em, tc = float(rcfg.mu), float(rcfg.emissivity), float(rcfg.t_cosmic)
    except (TypeError, ValueError):
        _refuse(who, "the members of rcfg must be numbers")
    if not 0.0 < mu <= 1.0:
        _refuse(who, "rcfg: mu must be in (0, 1]")
    if not 0.0 <= em <= 1.0:
        _refuse(who, "rcfg: emissivity must be in [0, 1]")
    if not (math.isfinite(tc) and tc >= 0.0):
        _refuse(who, "rcfg: t_cosmic must be finite and not below 0")
    return _RadiometerCfg(mu, em, tc)


def radiometer_sphere(x, m):
    """(Q_ext, Q_sca, Q_back, g) of a homogeneous sphere of size parameter x and complex refractive index m = n + ik,
    k >= 0, by the Lorenz-Mie series of the library (kidmp_radiometer_sphere): host code, no device."""
    m = complex(m)
    q = [C.c_double() for _ in range(4)]
    rc = library().kidmp_radiometer_sphere(float(x), m.real, m.imag, *[C.byref(v) for v in q])
    if rc < 0:
        _raise(rc)
    return tuple(v.value for v in q)


def radiometer_bins(cfg, species, D):
    """The three rows RADIOMETER_ROWS of `species` ("r", "s", "g") on the diameters D (m), float64 [3, nb]
    (kidmp_radiometer_bins): host code, no device."""
    who = "radiometer_bins"
    c = _config(who, cfg)
    x = _species(who, species)
    D = np.ascontiguousarray(D, dtype=np.float64)
    if D.ndim != 1 or D.shape[0] < 1:
        _refuse(who, "D must be one-dimensional with at least one diameter")
    rows = np.empty((len(RADIOMETER_ROWS), D.shape[0]), dtype=np.float64)
    rc = library().kidmp_radiometer_bins(C.byref(c), x, D.shape[0], D.ctypes.data, rows.ctypes.data)
    if rc < 0:
        _raise(rc)
    return rows


class RadiometerTable:
    """The rows of rain, snow and graupel for one configuration, on the device of `model` (kidmp_radiometer_table_create).

    cfg     None = the defaults (10 cm), or a MieCfg (kw2 is not read)
    grids   None, or a dict species ("r", "s", "g") -> (D, dD): float64 numpy arrays [nb], 1 <= nb <= MIE_MAX_BINS, bin
            diameters and widths in m; a species without an entry is put on the scheme's own 100 bins
    The handle is freed by close(), on leaving a `with` block, or when the object is collected; free it before the model."""

    def __init__(self, model, cfg=None, grids=None):
        who = "RadiometerTable"
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
        rc = library().kidmp_radiometer_table_create(model._h, C.byref(c), C.byref(g), C.byref(h))
        if rc < 0:
            _raise(rc, model._h)
        self._t = h

    def get(self, species):
        """(D, dD, rows) of a species as the device holds them: float64 [nb], [nb], [3, nb] (kidmp_radiometer_table_get)."""
        who = "RadiometerTable.get"
        if self._t is None:
            _refuse(who, "the table is closed")
        x = _species(who, species)
        L = library()
        nb = C.c_int32()
        rc = L.kidmp_radiometer_table_get(self._t, x, C.byref(nb), None, None, None, None)
        if rc < 0:
            _raise(rc, self.model._h)
        D, dD, rows = np.empty(nb.value), np.empty(nb.value), np.empty((len(RADIOMETER_ROWS), nb.value))
        rc = L.kidmp_radiometer_table_get(self._t, x, C.byref(nb), D.ctypes.data, dD.ctypes.data, rows.ctypes.data, None)
        if rc < 0:
            _raise(rc, self.model._h)
        return D, dD, rows

    @property
    def cfg(self):
        """The configuration the table was built with, as a MieCfg."""
        if self._t is None:
            _refuse("RadiometerTable.cfg", "the table is closed")
        c, nb = _MieCfg(), C.c_int32()
        rc = library().kidmp_radiometer_table_get(self._t, 0, C.byref(nb), None, None, None, C.byref(c))
        if rc < 0:
            _raise(rc, self.model._h)
        return MieCfg(c.wavelength, complex(c.eps_w_re, c.eps_w_im), complex(c.eps_i_re, c.eps_i_im), c.rho_w, c.rho_i, c.kw2)

    def close(self):
        if self._t is not None:
            library().kidmp_radiometer_table_destroy(self._t)
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
        _refuse(who, "want must be a name or a sequence of names out of %s" % (RADIOMETER_NAMES,))
    for n in want:
        if n not in RADIOMETER_NAMES:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, RADIOMETER_NAMES))
    if len(set(want)) != len(want):
        _refuse(who, "want names an output twice")
    if not want:
        _refuse(who, "nothing requested: want is empty")
    return want


def _table(who, model, table):
    if not isinstance(table, RadiometerTable) or table._t is None:
        _refuse(who, "table must be an open RadiometerTable")
    if table.model is not model:
        _refuse(who, "the table belongs to another context")
    return table._t


def _call(fn, model, table, rcfg, ncol, nz, ptrs, dz, dz_stride, k_gas, kg_stride, t_sfc, addr, res, *stream):
    o = _RadiometerOut(**{n: addr(a) for n, a in res.items()})
    rc = fn(model._h, table, C.byref(rcfg), ncol, nz, *ptrs, dz, dz_stride, k_gas, kg_stride, t_sfc, C.byref(o), *stream)
    if rc < 0:
        _raise(rc, model._h)


def _shapes(want, ncol, nz):
    return {n: (ncol,) if n in RADIOMETER_SUMMARY_NAMES else (ncol, nz) for n in want}


def radiometer(model, table, st, dz=None, k_gas=None, t_sfc=None, rcfg=None, want=("tb_toa",), out=None, stream=None):
    """The radiometer of a device-resident state (kidmp[32]_radiometer_device): one launch.

    table   a RadiometerTable of this model
    st      dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load), keys RADIOMETER_INPUTS; qc,
            qs and qg may be missing (or None): zero
    dz      layer depths in m, [nz] or [ncol, nz], of the state's dtype; needed for everything but k_abs and k_bsc
    k_gas   None (zero) or the gas absorption in 1/m, [nz] or [ncol, nz]
    t_sfc   None (the column's t at level 0) or the surface temperature [ncol]
    rcfg    None (mu = 1, emissivity = 1, t_cosmic = 2.725) or a RadiometerCfg
    want    names out of RADIOMETER_NAMES: k_abs, k_bsc the absorption and back-hemisphere scattering coefficients (1/m);
            refl, trans the layer's reflection and transmission; tb_up, tb_down the brightness temperatures (K) going up
            through the upper face and coming down through the lower face of each level; all [ncol, nz]; tb_toa what a
            satellite sees, tb_ground what a ground radiometer sees, tau_abs the absorption optical depth: [ncol]
    out     None, or a dict name -> tensor of the result's shape and dtype to write into instead of a fresh one
    Returns a dict name -> tensor.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    who = "radiometer"
    if not isinstance(st, dict) or not isinstance(st.get("t"), torch.Tensor):
        _refuse(who, "the state must be a dict of torch tensors with the keys %s" % (RADIOMETER_INPUTS,))
    q = st["t"]
    if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 tensors [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = int(q.shape[0]), int(q.shape[1])
    want = _wanted(who, want)
    h = _table(who, model, table)
    r = _rcfg(who, rcfg)

    def check(a, k, shape=(ncol, nz)):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        model._want(a, q.dtype, shape, who + ": ", k)

    ptrs = _th._pointers(st, RADIOMETER_INPUTS, _OPTIONAL, check, torch.Tensor.data_ptr)
    for a, k in ((dz, "dz"), (k_gas, "k_gas"), (t_sfc, "t_sfc")):
        if a is not None and not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
    if dz is None and any(n not in _NO_DZ for n in want):
        _refuse(who, "dz is needed for everything but %s" % (_NO_DZ,))
    dz_stride = _stride(who, dz, "dz", () if dz is None else dz.shape, ncol, nz)
    kg_stride = _stride(who, k_gas, "k_gas", () if k_gas is None else k_gas.shape, ncol, nz)
    for a, k in ((dz, "dz"), (k_gas, "k_gas")):
        if a is not None:
            check(a, k, tuple(a.shape))
    if t_sfc is not None:
        check(t_sfc, "t_sfc", (ncol,))
    res = _results(who, want, out, _shapes(want, ncol, nz), q.dtype, check, lambda s, d: torch.empty(s, dtype=d, device=q.device))
    L = library()
    fn = L.kidmp_radiometer_device if q.dtype == torch.float64 else L.kidmp32_radiometer_device
    ptr = lambda a: None if a is None else a.data_ptr()   # noqa: E731
    _call(fn, model, h, r, ncol, nz, ptrs, ptr(dz), dz_stride, ptr(k_gas), kg_stride, ptr(t_sfc), torch.Tensor.data_ptr, res, _th._stream(stream, q))
    return res


def radiometer_host(model, table, st, dz=None, k_gas=None, t_sfc=None, rcfg=None, want=("tb_toa",), out=None):
    """radiometer on numpy arrays [ncol, nz] (float64 or float32): chunks of columns through the context's staging memory
    (kidmp[32]_radiometer_host); only what `want` names comes back over PCIe.  Returns numpy arrays, bit for bit what
    radiometer gives."""
    who = "radiometer_host"
    if not isinstance(st, dict) or not isinstance(st.get("t"), np.ndarray):
        _refuse(who, "the state must be a dict of numpy arrays with the keys %s" % (RADIOMETER_INPUTS,))
    q = st["t"]
    if q.dtype not in (np.float64, np.float32) or q.ndim != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 arrays [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = q.shape
    want = _wanted(who, want)
    h = _table(who, model, table)
    r = _rcfg(who, rcfg)

    def check(a, k, shape=(ncol, nz)):
        if not (isinstance(a, np.ndarray) and a.dtype == q.dtype and a.flags.c_contiguous and a.shape == tuple(shape)):
            _refuse(who, "%s must be a contiguous %s array %s" % (k, q.dtype.name, list(shape)))

    addr = lambda a: a.ctypes.data   # noqa: E731
    ptrs = _th._pointers(st, RADIOMETER_INPUTS, _OPTIONAL, check, addr)
    for a, k in ((dz, "dz"), (k_gas, "k_gas"), (t_sfc, "t_sfc")):
        if a is not None and not isinstance(a, np.ndarray):
            _refuse(who, "%s must be a numpy array, got %s" % (k, type(a).__name__))
    if dz is None and any(n not in _NO_DZ for n in want):
        _refuse(who, "dz is needed for everything but %s" % (_NO_DZ,))
    dz_stride = _stride(who, dz, "dz", () if dz is None else dz.shape, ncol, nz)
    kg_stride = _stride(who, k_gas, "k_gas", () if k_gas is None else k_gas.shape, ncol, nz)
    for a, k in ((dz, "dz"), (k_gas, "k_gas")):
        if a is not None:
            check(a, k, a.shape)
    if t_sfc is not None:
        check(t_sfc, "t_sfc", (ncol,))
    res = _results(who, want, out, _shapes(want, ncol, nz), q.dtype, check, lambda s, d: np.empty(s, dtype=d))
    L = library()
    fn = L.kidmp_radiometer_host if q.dtype == np.float64 else L.kidmp32_radiometer_host
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    _call(fn, model, h, r, ncol, nz, ptrs, ptr(dz), dz_stride, ptr(k_gas), kg_stride, ptr(t_sfc), addr, res)
    return res
