"""A lidar / ceilometer forward operator on the device (include/kidmp_lidar.h): the geometric-optics extinction of the five
species from the scheme's own size distributions, backscatter, the optical depth seen from the ground and from space, the
layer-mean attenuated backscatter, the scattering ratio and eight numbers per column -- one launch per call.

The four entries of kidmp_lidar.h are declared here, on the object load_library() returned, the first time one of them is
needed: include/kidmp.h and its mirror in thompson.py stay what they are.  There is no fallback: without the library or
the device a call raises KidmpError.
"""
import ctypes as C
import math

import numpy as np

from . import thompson as _th
from .thompson import KidmpError

LIDAR_NAMES = ("ext_c", "ext_i", "ext_r", "ext_s", "ext_g", "ext", "bsc", "bsc_mol", "tau_up", "tau_dn", "att_up", "att_dn",
               "sr_up", "sr_dn")                               # kidmp_lidar_out
LIDAR_SUMMARY_N = 8                                            # KIDMP_LIDAR_SUMMARY_N
LIDAR_SUMMARY_NAMES = ("tau_part", "tau_mol", "z_base_up", "z_lost_up", "z_top_dn", "z_lost_dn", "n_up", "n_dn")   # slot s is KIDMP_LIDAR_<NAME>
LIDAR_INPUTS = ("t", "p", "qv", "qc", "nc", "qi", "ni", "qr", "nr", "qs", "qg")
LIDAR_SPECIES = ("c", "i", "r", "s", "g")                      # the order of s_ratio
_OPTIONAL = ("nc", "qi", "ni", "qs", "qg")                     # whether one may be left out is the library's to say
_LOCAL = LIDAR_NAMES[:8]                                       # need no neighbouring level: no scan, dz is not read
_CFG_KEYS = ("s_ratio", "eta", "c_mol", "beta_detect", "trans_lost")


class _LidarOut(C.Structure):
    """kidmp_lidar_out / kidmp32_lidar_out: fourteen pointers."""
    _fields_ = [(n, C.c_void_p) for n in LIDAR_NAMES]


class _LidarCfg(C.Structure):
    """kidmp_lidar_cfg."""
    _fields_ = [("s_ratio", C.c_double * 5), ("eta", C.c_double), ("c_mol", C.c_double), ("beta_detect", C.c_double),
                ("trans_lost", C.c_double)]


class LidarCfg:
    """The configuration of the operator; what is not given keeps the value of a NULL cfg (conventions of this library)."""

    def __init__(self, s_ratio=(18.8, 25.0, 18.8, 25.0, 25.0), eta=0.7, c_mol=6.2446e-32, beta_detect=2.0e-5, trans_lost=2.5e-3):
        self.s_ratio, self.eta, self.c_mol, self.beta_detect, self.trans_lost = s_ratio, eta, c_mol, beta_detect, trans_lost

    def as_dict(self):
        return {k: getattr(self, k) for k in _CFG_KEYS}


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_lidar.h."""
    i32, i64, vp, rc = C.c_int32, C.c_int64, C.c_void_p, C.c_int
    host = [vp, i64, i32] + [vp] * 12 + [i64, C.POINTER(_LidarCfg), C.POINTER(_LidarOut), vp]
    return {
        "kidmp_lidar_profiles_device": (rc, host + [vp]),
        "kidmp32_lidar_profiles_device": (rc, host + [vp]),
        "kidmp_lidar_profiles_host": (rc, host),
        "kidmp32_lidar_profiles_host": (rc, host),
    }


def declare(L):
    """Declare the entries of kidmp_lidar.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the lidar entries declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _refuse(who, msg):
    raise KidmpError("%s: %s" % (who, msg))


def _wanted(who, want, summary):
    if isinstance(want, str):
        want = (want,)
    try:
        want = tuple(want)
    except TypeError:
        _refuse(who, "want must be a name or a sequence of names out of %s" % (LIDAR_NAMES,))
    for n in want:
        if n not in LIDAR_NAMES:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, LIDAR_NAMES))
    if len(set(want)) != len(want):
        _refuse(who, "want names an output twice")
    if not isinstance(summary, bool):
        _refuse(who, "summary must be True or False")
    if not want and not summary:
        _refuse(who, "nothing requested: want is empty and summary is False")
    return want


def _cfg(who, cfg, want):
    """None, or the kidmp_lidar_cfg of a LidarCfg / a dict with keys out of s_ratio (five numbers in the order c, i, r, s, g,
    or a dict by species), eta, c_mol, beta_detect, trans_lost.  What the library would refuse is refused here."""
    if cfg is None:
        return None
    if isinstance(cfg, LidarCfg):
        cfg = cfg.as_dict()
    try:
        if not isinstance(cfg, dict) or set(cfg) - set(_CFG_KEYS):
            raise ValueError
        full = dict(LidarCfg().as_dict(), **cfg)
        s = full["s_ratio"]
        if isinstance(s, dict):
            if set(s) - set(LIDAR_SPECIES):
                raise ValueError
            s = [s.get(x, d) for x, d in zip(LIDAR_SPECIES, LidarCfg().s_ratio)]
        s = [float(x) for x in s]
        v = [float(full[k]) for k in _CFG_KEYS[1:]]
    except (TypeError, ValueError):
        _refuse(who, "cfg must be None, a LidarCfg, or a dict with keys out of %s" % (_CFG_KEYS,))
    if len(s) != 5 or not all(math.isfinite(x) for x in s + v):
        _refuse(who, "cfg must hold five lidar ratios and four numbers, all finite")
    if not all(x > 0.0 for x in s):
        _refuse(who, "cfg: a lidar ratio must be positive")
    if not 0.0 < v[0] <= 1.0:
        _refuse(who, "cfg: eta outside (0, 1]")
    if v[1] < 0.0:
        _refuse(who, "cfg: c_mol < 0")
    if v[1] == 0.0 and ("sr_up" in want or "sr_dn" in want):
        _refuse(who, "cfg: a scattering ratio needs c_mol > 0")
    return _LidarCfg((C.c_double * 5)(*s), *v)


def _dz_stride(who, dz, shape, ncol, nz, need):
    if dz is None:
        if need:
            _refuse(who, "dz is needed for the optical depths, the attenuated profiles, the ratios and the summary")
        return 0
    if tuple(shape) == (nz,):
        return 0
    if tuple(shape) == (ncol, nz):
        return nz
    _refuse(who, "dz must be [nz] = [%d] or [ncol, nz] = [%d, %d], got %s" % (nz, ncol, nz, list(shape)))


def _call(fn, model, ncol, nz, ptrs, dz, stride, c, out, summary, *stream):
    o = _LidarOut(**out)
    rc = fn(model._h, ncol, nz, *ptrs, dz, stride, C.byref(c) if c is not None else None, C.byref(o), summary, *stream)
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, library().kidmp_last_error(model._h).decode()))


def lidar_profiles(model, st, dz=None, cfg=None, want=LIDAR_NAMES, summary=False, stream=None):
    """The lidar profiles of a device-resident state (kidmp[32]_lidar_profiles_device): one launch.

    st        dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load), keys LIDAR_INPUTS; nc may
              be missing (or None) unless the context is aerosol-aware, qi, ni, qs and qg in an iiwarm context
    dz        layer depths in m (positive), [nz] for all columns or [ncol, nz], of the state's dtype; None is allowed when
              only names out of ext_*, ext, bsc, bsc_mol are wanted
    cfg       None = the library's conventions, a LidarCfg, or a dict with keys out of s_ratio, eta, c_mol, beta_detect,
              trans_lost
    want      the profiles to form, names out of LIDAR_NAMES; one that is not named costs no store
    summary   True: the result also holds "summary", [ncol, 8] float64, column LIDAR_SUMMARY_NAMES.index(name); NaN where
              the level a slot asks for does not exist
    Returns a dict name -> [ncol, nz] tensor of the state's dtype.  Asynchronous on `stream` (default: torch's current)."""
    import torch
    who = "lidar_profiles"
    if not isinstance(st, dict) or not isinstance(st.get("t"), torch.Tensor):
        _refuse(who, "the state must be a dict of torch tensors with the keys %s" % (LIDAR_INPUTS,))
    q = st["t"]
    if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 tensors [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = int(q.shape[0]), int(q.shape[1])
    want = _wanted(who, want, summary)
    c = _cfg(who, cfg, want)

    def check(a, k):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        model._want(a, q.dtype, (ncol, nz), who + ": ", k)

    ptrs = _th._pointers(st, LIDAR_INPUTS, _OPTIONAL, check, torch.Tensor.data_ptr)
    if dz is not None and not isinstance(dz, torch.Tensor):
        _refuse(who, "dz must be a torch tensor, got %s" % type(dz).__name__)
    stride = _dz_stride(who, dz, () if dz is None else dz.shape, ncol, nz, summary or any(n not in _LOCAL for n in want))
    if dz is not None:
        model._want(dz, q.dtype, tuple(dz.shape), who + ": ", "dz")
    res = {n: torch.empty((ncol, nz), dtype=q.dtype, device=q.device) for n in want}
    summ = torch.empty((ncol, LIDAR_SUMMARY_N), dtype=torch.float64, device=q.device) if summary else None
    L = library()
    fn = L.kidmp_lidar_profiles_device if q.dtype == torch.float64 else L.kidmp32_lidar_profiles_device
    _call(fn, model, ncol, nz, ptrs, dz.data_ptr() if dz is not None else None, stride, c, {n: res[n].data_ptr() for n in want},
          summ.data_ptr() if summary else None, _th._stream(stream, q))
    if summary:
        res["summary"] = summ
    return res


def lidar_profiles_host(model, st, dz=None, cfg=None, want=LIDAR_NAMES, summary=False):
    """lidar_profiles on numpy arrays [ncol, nz] (float64 or float32; dz [nz] or [ncol, nz] of the same dtype): chunks of
    columns through the context's staging memory (kidmp[32]_lidar_profiles_host); only the profiles in `want` come back
    over PCIe.  Returns numpy arrays, bit for bit what lidar_profiles gives."""
    who = "lidar_profiles_host"
    if not isinstance(st, dict) or not isinstance(st.get("t"), np.ndarray):
        _refuse(who, "the state must be a dict of numpy arrays with the keys %s" % (LIDAR_INPUTS,))
    q = st["t"]
    if q.dtype not in (np.float64, np.float32) or q.ndim != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the state must be float64 or float32 arrays [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = q.shape
    want = _wanted(who, want, summary)
    c = _cfg(who, cfg, want)

    def check(a, k, shape=(ncol, nz)):
        if not (isinstance(a, np.ndarray) and a.dtype == q.dtype and a.flags.c_contiguous and a.shape == shape):
            _refuse(who, "%s must be a contiguous %s array %s" % (k, q.dtype.name, list(shape)))

    ptrs = _th._pointers(st, LIDAR_INPUTS, _OPTIONAL, check, lambda a: a.ctypes.data)
    if dz is not None and not isinstance(dz, np.ndarray):
        _refuse(who, "dz must be a numpy array, got %s" % type(dz).__name__)
    stride = _dz_stride(who, dz, () if dz is None else dz.shape, ncol, nz, summary or any(n not in _LOCAL for n in want))
    if dz is not None:
        check(dz, "dz", dz.shape)
    res = {n: np.empty((ncol, nz), dtype=q.dtype) for n in want}
    summ = np.empty((ncol, LIDAR_SUMMARY_N), dtype=np.float64) if summary else None
    L = library()
    fn = L.kidmp_lidar_profiles_host if q.dtype == np.float64 else L.kidmp32_lidar_profiles_host
    _call(fn, model, ncol, nz, ptrs, dz.ctypes.data if dz is not None else None, stride, c, {n: res[n].ctypes.data for n in want},
          summ.ctypes.data if summary else None)
    if summary:
        res["summary"] = summ
    return res
