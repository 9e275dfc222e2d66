"""Range-height (RHI) radar scans of an x-z slab on the device (include/kidmp_scan.h): slant beams that cross columns,
range gates that are not model levels, attenuation along the beam, beam broadening in elevation and the radial velocity,
in one launch per call (scan).  A geometric operator over [ncol, nz] fields that any radar operator of the library made;
it returns the sampled cell indices, so that `torch.take(field, cell.long())` pulls any other field onto the same gates.

The definitions are the project's own and parity with a radar simulator is unpinned; rhi_rays, which builds the ray table
with numpy, is an illustrative convention as well: the beam is broadened in elevation only, because a slab has no y.

The entries of kidmp_scan.h are declared here, on the object load_library() returned, the first time one of them is
needed.  There is no fallback: without the library or the device a call raises KidmpError.
"""
import ctypes as C
import math

import numpy as np

from . import thompson as _th
from .thompson import KidmpError

SCAN_NAMES = ("dbz", "dbz_att", "pia", "vr", "height", "cell")  # kidmp_scan_out
SCAN_FIELDS = ("dbz", "ext", "vd", "u")                         # the fields a scan reads; only dbz is required
SCAN_MAX_GATES = 1024                                           # KIDMP_SCAN_MAX_GATES
SCAN_MAX_SUB = 9                                                # KIDMP_SCAN_MAX_SUB
RAY_WORDS = ("slab", "x0", "z0", "ce", "se", "wgt")             # a row of the ray table


class _ScanCfg(C.Structure):
    """kidmp_scan_cfg."""
    _fields_ = [("r0", C.c_double), ("dr", C.c_double), ("ngate", C.c_int32), ("nsub", C.c_int32), ("half_inv_ae", C.c_double),
                ("periodic", C.c_int32), ("missing", C.c_double)]


class _ScanOut(C.Structure):
    """kidmp_scan_out / kidmp32_scan_out: five value pointers and cell."""
    _fields_ = [(n, C.c_void_p) for n in SCAN_NAMES]


class ScanCfg:
    """The configuration of a scan: gate g is centred at r0 + (g + 0.5)*dr metres along the beam, g = 0 .. ngate-1; nsub
    rows of the ray table make one output ray; half_inv_ae = 1/(2 a_e) with a_e the effective earth radius in m (0: a flat
    earth; ScanCfg.earth(a_e) forms it); periodic wraps x into the slab, otherwise a beam leaves through its sides;
    missing is stored where a gate has no sample inside the slab."""

    def __init__(self, r0=0.0, dr=100.0, ngate=256, nsub=1, half_inv_ae=0.0, periodic=False, missing=float("nan")):
        self.r0, self.dr, self.ngate, self.nsub = r0, dr, ngate, nsub
        self.half_inv_ae, self.periodic, self.missing = half_inv_ae, periodic, missing

    @staticmethod
    def earth(a_e=8.5e6):
        """1/(2 a_e): the curvature term of a beam over an earth of effective radius a_e (4/3 of the earth's: 8.5e6 m)."""
        return 1.0 / (2.0 * float(a_e))


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_scan.h."""
    i32, i64, vp, rc, d = C.c_int32, C.c_int64, C.c_void_p, C.c_int, C.c_double
    entry = [vp, i64, i32, i32, d, vp, vp, vp, vp, i32, vp, vp, i64, C.POINTER(_ScanCfg), C.POINTER(_ScanOut), vp]
    return {"kidmp_scan_device": (rc, entry), "kidmp32_scan_device": (rc, entry)}


def declare(L):
    """Declare the entries of kidmp_scan.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the entries of kidmp_scan.h declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _refuse(who, msg):
    raise KidmpError("%s: %s" % (who, msg))


def _config(who, cfg):
    """The kidmp_scan_cfg of a ScanCfg, refused here where the library would refuse it."""
    if not isinstance(cfg, ScanCfg):
        _refuse(who, "cfg must be a ScanCfg")
    try:
        r0, dr, hae, missing = float(cfg.r0), float(cfg.dr), float(cfg.half_inv_ae), float(cfg.missing)
        ngate, nsub = int(cfg.ngate), int(cfg.nsub)
    except (TypeError, ValueError):
        _refuse(who, "the members of cfg must be numbers")
    if ngate != cfg.ngate or nsub != cfg.nsub or not 1 <= ngate <= SCAN_MAX_GATES or not 1 <= nsub <= SCAN_MAX_SUB:
        _refuse(who, "cfg: ngate must be a whole number in [1, %d] and nsub one in [1, %d]" % (SCAN_MAX_GATES, SCAN_MAX_SUB))
    if not (dr > 0.0 and math.isfinite(dr)) or not (r0 >= 0.0 and math.isfinite(r0)) or not math.isfinite(hae):
        _refuse(who, "cfg: dr must be finite and above 0, r0 finite and not below 0, half_inv_ae finite")
    return _ScanCfg(r0, dr, ngate, nsub, hae, 1 if cfg.periodic else 0, missing)


def _wanted(who, want):
    if isinstance(want, str):
        want = (want,)
    try:
        want = tuple(want)
    except TypeError:
        _refuse(who, "want must be a name or a sequence of names out of %s" % (SCAN_NAMES,))
    for n in want:
        if n not in SCAN_NAMES:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, SCAN_NAMES))
    if len(set(want)) != len(want):
        _refuse(who, "want names an output twice")
    if not want:
        _refuse(who, "nothing requested: want is empty")
    return want


def rhi_rays(slab, x0, z0, elevations_deg, beamwidth_deg=0.0, nsub=1):
    """The ray table [nray*nsub, 6] (float64, rows slab, x0, z0, ce, se, wgt) of a range-height sweep: one radar at
    (x0, z0) metres in slab `slab`, one output ray per elevation in degrees from the +x axis (above 90: looking back).

    nsub == 1 (or beamwidth_deg == 0 with nsub == 1): one row per ray with wgt = 1.  nsub > 1: the sub-rays are evenly
    spaced over +/- one beamwidth in elevation, delta_j = beamwidth*(2 j/(nsub-1) - 1), with the two-way Gaussian
    weights exp(-8 ln2 (delta_j/beamwidth)**2) normalised to a sum of 1 (beamwidth_deg: the one-way half-power width).
    Cosine and sine are numpy's of the angle in radians, except that a multiple of 90 degrees gives 0 and +/-1 exactly."""
    who = "rhi_rays"
    el = np.atleast_1d(np.asarray(elevations_deg, dtype=np.float64))
    if el.ndim != 1 or not np.isfinite(el).all():
        _refuse(who, "elevations_deg must be finite numbers, a scalar or a sequence")
    if isinstance(nsub, bool) or int(nsub) != nsub or not 1 <= nsub <= SCAN_MAX_SUB:
        _refuse(who, "nsub must be a whole number in [1, %d]" % SCAN_MAX_SUB)
    nsub = int(nsub)
    bw = float(beamwidth_deg)
    if not (bw >= 0.0 and math.isfinite(bw)) or (nsub > 1 and not bw > 0.0):
        _refuse(who, "beamwidth_deg must be finite and not below 0, and above 0 with nsub > 1")
    if int(slab) != slab or slab < 0:
        _refuse(who, "slab must be a whole number >= 0")
    if nsub == 1:
        delta, wgt = np.zeros(1), np.ones(1)
    else:
        delta = bw * (2.0 * np.arange(nsub) / (nsub - 1) - 1.0)
        wgt = np.exp(-8.0 * math.log(2.0) * (delta / bw) ** 2)
        wgt = wgt / wgt.sum()
    ang = el[:, None] + delta[None, :]
    ce, se = np.cos(np.deg2rad(ang)), np.sin(np.deg2rad(ang))
    quarter = np.mod(ang, 360.0) / 90.0                               # 0, 1, 2, 3 exactly at the axes
    for q, c, s in ((0.0, 1.0, 0.0), (1.0, 0.0, 1.0), (2.0, -1.0, 0.0), (3.0, 0.0, -1.0)):
        ce = np.where(quarter == q, c, ce)
        se = np.where(quarter == q, s, se)
    rays = np.empty((el.size, nsub, len(RAY_WORDS)))
    rays[..., 0], rays[..., 1], rays[..., 2] = float(slab), float(x0), float(z0)
    rays[..., 3], rays[..., 4], rays[..., 5] = ce, se, wgt[None, :]
    return np.ascontiguousarray(rays.reshape(el.size * nsub, len(RAY_WORDS)))


def scan(model, fields, zf, rays, dx, nx, cfg, want=("dbz_att",), out=None, stream=None):
    """A scan of device-resident fields (kidmp[32]_scan_device): one launch, no allocation beyond the results, no
    synchronisation.

    fields  dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load): "dbz" (required, dBZ of any
            radar operator), "ext" (one-way extinction in 1/m; missing or None: no attenuation), "vd" (mean Doppler
            velocity of a vertical beam, positive downward, w applied; missing: 0), "u" (x velocity at the left face of
            each cell as advect_slab takes it, [ncol, nz] or [nx, nz] for every slab; missing: 0).  ncol = nslab*nx and
            column s*nx + i is cell i of slab s.
    zf      float64 CUDA tensor [nz+1]: the level faces in m, ascending
    rays    float64 CUDA tensor [nray*nsub, 6] (rhi_rays): rows slab, x0, z0, ce, se, wgt
    dx      cell width in m; nx cells per slab
    cfg     a ScanCfg
    want    names out of SCAN_NAMES: dbz the unattenuated and dbz_att the attenuated reflectivity in dBZ, pia the two-way
            path attenuation in dB, vr the radial velocity (positive away from the radar; needs vd or u), height the
            gate centres' height in m, cell (int32) the flat index col*nz + k of the sampled cell or -1; all [nray, ngate]
    out     None, or the dict an earlier call returned (or name -> tensor of the result's shape and dtype): rewritten in
            place, nothing is allocated
    Returns a dict name -> tensor.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    who = "scan"
    if not isinstance(fields, dict) or not isinstance(fields.get("dbz"), torch.Tensor):
        _refuse(who, "fields must be a dict of torch tensors with the key 'dbz' and any of %s" % (SCAN_FIELDS[1:],))
    bad = [k for k in fields if k not in SCAN_FIELDS]
    if bad:
        _refuse(who, "unknown fields %s: the keys are %s" % (bad, SCAN_FIELDS))
    q = fields["dbz"]
    if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "the fields must be float64 or float32 tensors [ncol, nz] with nz in [2, %d]" % _th.MAX_NZ)
    ncol, nz = int(q.shape[0]), int(q.shape[1])
    if isinstance(nx, bool) or not isinstance(nx, int) or nx < 1 or ncol % nx != 0:
        _refuse(who, "nx must be a whole number >= 1 that divides ncol = %d, got %r" % (ncol, nx))
    nslab = ncol // nx
    try:
        dx = float(dx)
    except (TypeError, ValueError):
        _refuse(who, "dx must be a number")
    if not (dx > 0.0 and math.isfinite(dx)):
        _refuse(who, "dx must be finite and above 0")
    c_cfg = _config(who, cfg)
    want = _wanted(who, want)

    def check(a, k, shape, dtype=q.dtype):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (k, type(a).__name__))
        model._want(a, dtype, shape, who + ": ", k)

    ptr = {}
    for k in SCAN_FIELDS:
        a = fields.get(k)
        if a is not None:
            shared = k == "u" and isinstance(a, torch.Tensor) and tuple(a.shape) == (nx, nz)
            check(a, k, (nx, nz) if shared else (ncol, nz))
        ptr[k] = None if a is None else a.data_ptr()
    u = fields.get("u")
    shared_flow = 1 if u is not None and tuple(u.shape) == (nx, nz) else 0
    if "vr" in want and ptr["vd"] is None and ptr["u"] is None:
        _refuse(who, "vr needs 'vd' or 'u' among the fields")
    check(zf, "zf", (nz + 1,), torch.float64)
    if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != len(RAY_WORDS) or rays.shape[0] % c_cfg.nsub != 0:
        _refuse(who, "rays must be a float64 CUDA tensor [nray*nsub, 6] with nsub = %d" % c_cfg.nsub)
    check(rays, "rays", tuple(rays.shape), torch.float64)
    nray = int(rays.shape[0]) // c_cfg.nsub
    if "cell" in want and ncol * nz > 0x7fffffff:
        _refuse(who, "cell is 32 bits wide: ncol*nz = %d is above 0x7fffffff" % (ncol * nz))
    if out is not None and not isinstance(out, dict):
        _refuse(who, "out must be a dict name -> tensor")
    res = {}
    for n in want:
        dtype = torch.int32 if n == "cell" else q.dtype
        if out is not None and out.get(n) is not None:
            check(out[n], "out[%r]" % n, (nray, c_cfg.ngate), dtype)
            res[n] = out[n]
        else:
            res[n] = torch.empty((nray, c_cfg.ngate), dtype=dtype, device=q.device)
    o = _ScanOut(**{n: a.data_ptr() for n, a in res.items()})
    L = library()
    fn = L.kidmp_scan_device if q.dtype == torch.float64 else L.kidmp32_scan_device
    rc = fn(model._h, nslab, nx, nz, dx, ptr["dbz"], ptr["ext"], ptr["vd"], ptr["u"], shared_flow, zf.data_ptr(), rays.data_ptr(), nray,
            C.byref(c_cfg), C.byref(o), _th._stream(stream, q))
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, L.kidmp_last_error(model._h).decode()))
    return res
