"""Several channels of the radiometer or of the cloud radar in one launch (include/kidmp_multichannel.h).

A microwave imager has nine to thirteen channels, a dual-frequency radar two.  A channel set is a list of 1 to MAX_CHANNELS
existing RadiometerTable or MieTable objects of one model, all on the same diameter grids; radiometer_multi and
mie_radar_multi form the load and the size distributions once and fold every bin into the sums of all the channels.  Slab
c of every result holds the bits radiometer / mie_radar gives with tables[c] (and rcfgs[c], and channel c's k_gas),
whatever else is in the list; the same table may appear twice.

The entries of kidmp_multichannel.h are declared here, on the object load_library() returned, the first time one of them
is needed.  There is no fallback: without the library a call raises KidmpError.
"""
import ctypes as C

import numpy as np

from . import mie as _mie
from . import radiometer as _rad
from . import thompson as _th
from .mie import _refuse, _results

MAX_CHANNELS = 16                                               # KIDMP_MAX_CHANNELS
_KINDS = ("radiometer", "radar")                                # `which` of kidmp_multichannel_tile


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_multichannel.h."""
    i32, i64, vp, rc = C.c_int32, C.c_int64, C.c_void_p, C.c_int
    rad = [vp, C.POINTER(vp), i32, C.POINTER(_rad._RadiometerCfg), i64, i32] + [vp] * 8 + [vp, i64, vp, i64, i64, vp, C.POINTER(_rad._RadiometerOut)]
    radar = [vp, C.POINTER(vp), i32, i64, i32] + [vp] * 8 + [vp, i64, vp, vp, i64, i64, C.POINTER(_mie._MieOut)]
    return {
        "kidmp_multichannel_tile": (i32, [i32, i32]),
        "kidmp_radiometer_multi_device": (rc, rad + [vp]),
        "kidmp32_radiometer_multi_device": (rc, rad + [vp]),
        "kidmp_radiometer_multi_host": (rc, rad),
        "kidmp32_radiometer_multi_host": (rc, rad),
        "kidmp_mie_radar_multi_device": (rc, radar + [vp]),
        "kidmp32_mie_radar_multi_device": (rc, radar + [vp]),
        "kidmp_mie_radar_multi_host": (rc, radar),
        "kidmp32_mie_radar_multi_host": (rc, radar),
    }


def declare(L):
    """Declare the entries of kidmp_multichannel.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the entries of kidmp_multichannel.h declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def multichannel_tile(which, nz):
    """How many channels one pass of the kernel carries at nz levels (kidmp_multichannel_tile); which is "radiometer" (or 0)
    or "radar" (or 1).  Needs the library but no device."""
    who = "multichannel_tile"
    if which in _KINDS:
        which = _KINDS.index(which)
    if which not in (0, 1):
        _refuse(who, "which must be one of %s, or 0 or 1" % (_KINDS,))
    if not (isinstance(nz, (int, np.integer)) and 1 <= nz <= _th.MAX_NZ):
        _refuse(who, "nz must be an integer in [1, %d]" % _th.MAX_NZ)
    return int(library().kidmp_multichannel_tile(int(which), int(nz)))


def _handles(who, model, tables, one):
    """The array of handles of a channel set; `one` is radiometer._table or mie._table."""
    if isinstance(tables, (_rad.RadiometerTable, _mie.MieTable)) or not isinstance(tables, (list, tuple)):
        _refuse(who, "tables must be a list or tuple of tables")
    if not 1 <= len(tables) <= MAX_CHANNELS:
        _refuse(who, "the number of channels must be in [1, %d], got %d" % (MAX_CHANNELS, len(tables)))
    return (C.c_void_p * len(tables))(*[one(who, model, t) for t in tables])


def _rcfgs(who, rcfgs, nch):
    """The kidmp_radiometer_cfg array of None, one RadiometerCfg or a sequence of nch."""
    if rcfgs is None or isinstance(rcfgs, _rad.RadiometerCfg):
        rcfgs = [rcfgs] * nch
    if not isinstance(rcfgs, (list, tuple)) or len(rcfgs) != nch:
        _refuse(who, "rcfgs must be None, one RadiometerCfg or a sequence of %d" % nch)
    return (_rad._RadiometerCfg * nch)(*[_rad._rcfg(who, r) for r in rcfgs])


def _k_gas_strides(who, k_gas, nch, ncol, nz):
    """(column stride, channel stride) of k_gas [nz], [ncol, nz], [nch, nz] or [nch, ncol, nz]; a two-dimensional array
    whose first extent is ncol is [ncol, nz]."""
    if k_gas is None:
        return 0, 0
    shape = tuple(k_gas.shape)
    if shape == (nz,):
        return 0, 0
    if shape == (ncol, nz):
        return nz, 0
    if shape == (nch, nz):
        return 0, nz
    if shape == (nch, ncol, nz):
        return nz, ncol * nz
    _refuse(who, "k_gas must be [nz], [ncol, nz], [nch, nz] or [nch, ncol, nz] with nch = %d, ncol = %d, nz = %d, got %s"
            % (nch, ncol, nz, list(shape)))


class _Device:
    """What differs between the device entries (torch tensors) and the host entries (numpy arrays)."""

    def __init__(self, who, model, st, inputs):
        import torch
        self.who, self.model, self.kind, self.array = who, model, "torch tensor", torch.Tensor
        if not isinstance(st, dict) or not isinstance(st.get("t"), torch.Tensor):
            _refuse(who, "the state must be a dict of torch tensors with the keys %s" % (inputs,))
        q = st["t"]
        if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
            _refuse(who, "the state must be float64 or float32 tensors [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
        self.q, self.ncol, self.nz, self.wide = q, int(q.shape[0]), int(q.shape[1]), q.dtype == torch.float64
        self.addr = torch.Tensor.data_ptr
        self.fresh = lambda s, d: torch.empty(s, dtype=d, device=q.device)
        self.suffix = "device"

    def check(self, a, k, shape=None):
        if not isinstance(a, self.array):
            _refuse(self.who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        self.model._want(a, self.q.dtype, (self.ncol, self.nz) if shape is None else shape, self.who + ": ", k)

    def tail(self, stream):
        return (_th._stream(stream, self.q),)


class _Host:
    def __init__(self, who, model, st, inputs):
        self.who, self.model, self.kind, self.array = who, model, "numpy array", np.ndarray
        if not isinstance(st, dict) or not isinstance(st.get("t"), np.ndarray):
            _refuse(who, "the state must be a dict of numpy arrays with the keys %s" % (inputs,))
        q = st["t"]
        if q.dtype not in (np.float64, np.float32) or q.ndim != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
            _refuse(who, "the state must be float64 or float32 arrays [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
        self.q, self.ncol, self.nz, self.wide = q, int(q.shape[0]), int(q.shape[1]), q.dtype == np.float64
        self.addr = lambda a: a.ctypes.data
        self.fresh = lambda s, d: np.empty(s, dtype=d)
        self.suffix = "host"

    def check(self, a, k, shape=None):
        shape = (self.ncol, self.nz) if shape is None else tuple(shape)
        if not (isinstance(a, np.ndarray) and a.dtype == self.q.dtype and a.flags.c_contiguous and a.shape == shape):
            _refuse(self.who, "%s must be a contiguous %s array %s" % (k, self.q.dtype.name, list(shape)))

    def tail(self, stream):
        return ()


def _common(b, st, inputs, optional, extras, nch, dz_needed, dz_msg):
    """The checks the four entries share; returns (state pointers, ptr, dz stride, (k_gas column stride, channel stride))."""
    who, ncol, nz = b.who, b.ncol, b.nz
    ptrs = _th._pointers(st, inputs, optional, b.check, b.addr)
    for a, k in extras:
        if a is not None and not isinstance(a, b.array):
            _refuse(who, "%s must be a %s, got %s" % (k, b.kind, type(a).__name__))
    dz, k_gas = extras[0][0], extras[1][0]
    if dz is None and dz_needed:
        _refuse(who, dz_msg)
    dz_stride = _mie._stride(who, dz, "dz", () if dz is None else dz.shape, ncol, nz)
    kg = _k_gas_strides(who, k_gas, nch, ncol, nz)
    for a, k in extras[:2]:
        if a is not None:
            b.check(a, k, tuple(a.shape))
    return ptrs, (lambda a: None if a is None else b.addr(a)), dz_stride, kg


def _radiometer(b, model, tables, st, dz, k_gas, t_sfc, rcfgs, want, out, stream):
    who, ncol, nz = b.who, b.ncol, b.nz
    want = _rad._wanted(who, want)
    h = _handles(who, model, tables, _rad._table)
    nch = len(h)
    r = _rcfgs(who, rcfgs, nch)
    ptrs, ptr, dz_stride, (kg_col, kg_ch) = _common(b, st, _rad.RADIOMETER_INPUTS, _rad._OPTIONAL, ((dz, "dz"), (k_gas, "k_gas"), (t_sfc, "t_sfc")),
                                                    nch, any(n not in _rad._NO_DZ for n in want), "dz is needed for everything but %s" % (_rad._NO_DZ,))
    if t_sfc is not None:
        b.check(t_sfc, "t_sfc", (ncol,))
    shapes = {n: (nch, ncol) if n in _rad.RADIOMETER_SUMMARY_NAMES else (nch, ncol, nz) for n in want}
    res = _results(who, want, out, shapes, b.q.dtype, b.check, b.fresh)
    fn = getattr(library(), "%s_radiometer_multi_%s" % ("kidmp" if b.wide else "kidmp32", b.suffix))
    o = _rad._RadiometerOut(**{n: b.addr(a) for n, a in res.items()})
    rc = fn(model._h, h, nch, r, ncol, nz, *ptrs, ptr(dz), dz_stride, ptr(k_gas), kg_col, kg_ch, ptr(t_sfc), C.byref(o), *b.tail(stream))
    if rc < 0:
        _rad._raise(rc, model._h)
    return res


def _mie_radar(b, model, tables, st, dz, w, k_gas, want, out, stream):
    who, ncol, nz = b.who, b.ncol, b.nz
    want = _mie._wanted(who, want)
    h = _handles(who, model, tables, _mie._table)
    nch = len(h)
    ptrs, ptr, dz_stride, (kg_col, kg_ch) = _common(b, st, _mie.MIE_INPUTS, _mie._OPTIONAL, ((dz, "dz"), (k_gas, "k_gas"), (w, "w")), nch,
                                                    any(n in _mie._PATH for n in want), "dz is needed for %s" % (_mie._PATH,))
    if w is not None:
        b.check(w, "w")
    shapes = {n: (nch, ncol) if n == "pia_total" else (nch, ncol, nz) for n in want}
    res = _results(who, want, out, shapes, b.q.dtype, b.check, b.fresh)
    fn = getattr(library(), "%s_mie_radar_multi_%s" % ("kidmp" if b.wide else "kidmp32", b.suffix))
    o = _mie._MieOut(**{n: b.addr(a) for n, a in res.items()})
    rc = fn(model._h, h, nch, ncol, nz, *ptrs, ptr(dz), dz_stride, ptr(w), ptr(k_gas), kg_col, kg_ch, C.byref(o), *b.tail(stream))
    if rc < 0:
        _mie._raise(rc, model._h)
    return res


def radiometer_multi(model, tables, st, dz=None, k_gas=None, t_sfc=None, rcfgs=None, want=("tb_toa",), out=None, stream=None):
    """The radiometer of a device-resident state at len(tables) channels (kidmp[32]_radiometer_multi_device): one launch.

    tables  a list of 1 to MAX_CHANNELS RadiometerTable of this model, all on the same grids
    st, dz, t_sfc, want, stream   as radiometer takes them; they are shared by the channels
    k_gas   None (zero) or the gas absorption in 1/m: [nz] or [ncol, nz] for all channels, [nch, nz] or [nch, ncol, nz]
            per channel (a two-dimensional array whose first extent is ncol is read as [ncol, nz])
    rcfgs   None (the defaults), one RadiometerCfg for all channels, or a sequence of one per channel
    out     None, or a dict name -> tensor of the result's shape and dtype to write into instead of a fresh one
    Returns a dict name -> tensor [nch, ncol, nz], or [nch, ncol] for tb_toa, tb_ground and tau_abs; slab c holds the bits
    of radiometer(model, tables[c], ..., rcfg=rcfgs[c])."""
    return _radiometer(_Device("radiometer_multi", model, st, _rad.RADIOMETER_INPUTS), model, tables, st, dz, k_gas, t_sfc, rcfgs, want, out, stream)


def radiometer_multi_host(model, tables, st, dz=None, k_gas=None, t_sfc=None, rcfgs=None, want=("tb_toa",), out=None):
    """radiometer_multi on numpy arrays (kidmp[32]_radiometer_multi_host): chunks of columns through the context's staging
    memory; returns numpy arrays, bit for bit what radiometer_multi gives."""
    return _radiometer(_Host("radiometer_multi_host", model, st, _rad.RADIOMETER_INPUTS), model, tables, st, dz, k_gas, t_sfc, rcfgs, want, out, None)


def mie_radar_multi(model, tables, st, dz=None, w=None, k_gas=None, want=("dbz",), out=None, stream=None):
    """The cloud radar of a device-resident state at len(tables) channels (kidmp[32]_mie_radar_multi_device): one launch.

    tables  a list of 1 to MAX_CHANNELS MieTable of this model, all on the same grids
    st, dz, w, want, stream   as mie_radar takes them; they are shared by the channels
    k_gas   None (zero) or the one-way gas extinction in 1/m, shaped as radiometer_multi's
    out     None, or a dict name -> tensor of the result's shape and dtype to write into instead of a fresh one
    Returns a dict name -> tensor [nch, ncol, nz], or [nch, ncol] for pia_total; slab c holds the bits of
    mie_radar(model, tables[c], ...).  A dual-wavelength ratio is dbz[i] - dbz[j] on the result."""
    return _mie_radar(_Device("mie_radar_multi", model, st, _mie.MIE_INPUTS), model, tables, st, dz, w, k_gas, want, out, stream)


def mie_radar_multi_host(model, tables, st, dz=None, w=None, k_gas=None, want=("dbz",), out=None):
    """mie_radar_multi on numpy arrays (kidmp[32]_mie_radar_multi_host): chunks of columns through the context's staging
    memory; returns numpy arrays, bit for bit what mie_radar_multi gives."""
    return _mie_radar(_Host("mie_radar_multi_host", model, st, _mie.MIE_INPUTS), model, tables, st, dz, w, k_gas, want, out, None)
