"""Host side of the MI355X Thompson-09n column solver.

Mirrors the reference's operator interface for the hot path
(/root/reference/module_mp_thompson09n.f90, "M:"):

    thompson_init()                 M:374      -> thompson_init(...) / ThompsonMP(...)
    mp_thompson(qv1d, ..., dt)      M:1156     -> mp_thompson(...) / ThompsonMP.mp_thompson
    do i=1,nx ... (KiD adapter)     W:54-246   -> ThompsonMP.batch_step (one launch)

Everything numerical happens in kid_amd/libkidmp.so (HIP kernels, C ABI of
include/kidmp.h).  There is deliberately NO CPU fallback: if the library or a
gfx950 device is missing, calls raise KidmpError.  torch is used only as the
owner of device memory and streams.
"""
import ctypes as C
import os

import numpy as np

STATE_NAMES = ("qv", "qc", "qi", "qr", "qs", "qg", "ni", "nr", "nc", "nwfa", "nifa", "t")   # INOUT, M:1168-1170
FORCING_NAMES = ("p", "w", "dz")                                                               # IN, M:1171
RATE_NAMES = (
    "pri_inu pri_ide prs_ide prs_sde prg_gde pri_wfz prs_scw prg_scw prg_gcw "
    "pri_ihm pri_rfz prs_iau prs_sci pri_rci pni_inu pni_ihm pni_wfz pni_rfz "
    "pni_ide pni_iau pni_sci pni_rci prr_sml prr_gml pnr_rcs pnr_rcg pnr_rci "
    "pnr_sml pnr_gml pnr_rfz prr_wau prr_rcw prv_rev pnr_wau pnr_rev pnr_rcr"
).split()                                                                                      # M:2967-3119
NRATES = 36
MAX_NZ = 256
PPT_LIMBS = 24            # KIDMP_PPT_LIMBS: exact precipitation accumulators (include/kidmp.h)

_HERE = os.path.dirname(os.path.abspath(__file__))


class KidmpError(RuntimeError):
    pass


class _Cfg(C.Structure):
    _fields_ = [("iiwarm", C.c_int32), ("l_sediment", C.c_int32), ("set_Nc", C.c_double),
                ("device", C.c_int32), ("is_aerosol_aware", C.c_int32)]


class _Outputs(C.Structure):
    """kidmp_outputs / kidmp32_outputs (include/kidmp.h): four pointers, null = not wanted."""
    _fields_ = [("dbz", C.c_void_p), ("re_qc", C.c_void_p), ("re_qi", C.c_void_p), ("re_qs", C.c_void_p)]


KID_FIELDS = ("theta", "qv", "qc", "qr", "nr", "qi", "ni", "qs", "qg")     # members of kidmp_kid_fields; the last four frozen
KID_WORK_NAMES = STATE_NAMES + FORCING_NAMES                                  # the 15 profiles of the adapter's workspace
_STEP_REQUIRED = STATE_NAMES + ("p", "dz")                                    # what a device step cannot do without (w: optional)


class _KidFields(C.Structure):
    """kidmp_kid_fields / kidmp32_kid_fields (include/kidmp.h): nine pointers, null = absent."""
    _fields_ = [(k, C.c_void_p) for k in KID_FIELDS]


def lib_path():
    """The in-tree build.  No environment override: a profiling or A/B build is selected explicitly with
    load_library(path) (bench.py --lib) before the first context is made."""
    return os.path.join(_HERE, "libkidmp.so")


_lib = None
_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_vp = C.c_void_p


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp.h.  An entry that exists as kidmp_* (binary64 arrays)
    and kidmp32_* (binary32 arrays, plus the `arith` selector where the entry steps) is written once."""
    i32, i64, size, text, rc = C.c_int32, C.c_int64, C.c_size_t, C.c_char_p, C.c_int
    cfg, outs, fields = C.POINTER(_Cfg), C.POINTER(_Outputs), C.POINTER(_KidFields)
    step64 = [_vp, i64, i32, C.c_double] + [_dp] * 16 + [_dp, _ip]       # the host step of either prefix, see below
    d = {
        "kidmp_init": (rc, [cfg, C.POINTER(_vp)]),
        "kidmp_finalize": (None, [_vp]),
        "kidmp_last_error": (text, [_vp]),
        "kidmp_init_seconds": (C.c_double, [_vp]),
        "kidmp_kernel_name": (text, []),
        "kidmp_reserve": (rc, [_vp, i64, i32]),
        "kidmp_host_alloc": (_vp, [size]),
        "kidmp_host_free": (None, [_vp]),
        "kidmp_set_host_chunk": (rc, [_vp, i64]),
        "kidmp_set_column_nc": (rc, [_vp, i64, _vp]),
        "kidmp_column_nc_count": (i64, [_vp]),
        "kidmp_batch_step_host_diag": (rc, step64),
        "kidmp_default_aerosols_device": (rc, [_vp, i64] + [_vp] * 6 + [_vp]),
        "kidmp_reduce_ppt_device": (rc, [_vp, i64, _vp, _vp, _vp]),
        "kidmp_reduce_ppt_exact_device": (rc, [_vp, i64, _vp, _vp, _vp]),
        "kidmp_ppt_limbs_to_sums": (rc, [C.POINTER(i64), _dp]),
        "kidmp_reduce_rates_device": (rc, [_vp, i64, i32, _vp, _vp, _vp]),
        "kidmp_sanity_device": (rc, [_vp, i64] + [_vp] * 9 + [_vp]),
        "kidmp_shard_bounds": (rc, [i64, i32, i32, C.POINTER(i64), C.POINTER(i64)]),
        "kidmp_init_multi": (rc, [cfg, i32, _ip, C.POINTER(_vp)]),
        "kidmp_finalize_multi": (None, [_vp]),
        "kidmp_multi_last_error": (text, [_vp]),
        "kidmp_multi_size": (i32, [_vp]),
        "kidmp_multi_context": (_vp, [_vp, i32]),
        "kidmp_batch_step_host_multi": (rc, step64 + [_dp]),
        "kidmp_batch_step_host_multi_diag": (rc, step64 + [_dp, _dp]),
        "kidmp_math_probe": (rc, [_vp, i32, i64, _dp, _dp, _dp]),
        "kidmp_math_probe_ex": (rc, [_vp, i32, i32, i64, _dp, _dp, _dp, _dp]),
        "kidmp_get_table": (i64, [_vp, text, _dp, i64]),
        "kidmp_get_const": (i64, [_vp, text, _dp, i64]),
        "kidmp_save_table_cache": (rc, [_vp, text]),
        "kidmp_load_table_cache": (rc, [_vp, text]),
        "kidmp_table_cache_reuse": (rc, [_vp, text, i32, i32, _ip]),
        "kidmp_cache_write_file": (rc, [text, i32, C.POINTER(_dp), i64]),
        "kidmp_cache_read_file": (rc, [text, i32, C.POINTER(_dp), i64]),
    }
    for pre, real, rp in (("kidmp", C.c_double, _dp), ("kidmp32", C.c_float, _fp)):
        arith = [i32] if pre == "kidmp32" else []
        head = [_vp, i64, i32, real]                         # ctx, ncol, nz, dt
        host = head + [rp] * 16 + [_dp, _ip]                 # 12 state + 3 forcing profiles, ppt; rates, nstep
        kid = [_vp, i64, i32, real, real, real] + [fields] * 3 + [_vp, _vp, fields, _vp, _vp, _vp, outs]
        d.update({
            pre + "_column_step": (rc, [_vp, i32, real] + [rp] * 16 + arith),
            # (kidmp_batch_step_host alone is older than nstep: kidmp_batch_step_host_diag is its full form)
            pre + "_batch_step_host": (rc, host + arith if arith else host[:-1]),
            pre + "_batch_step_host_refl": (rc, host + arith + [rp]),
            pre + "_batch_step_host_out": (rc, host + arith + [outs]),
            pre + "_batch_step_device": (rc, head + [_vp] * 18 + arith + [_vp]),
            pre + "_effective_radii_device": (rc, [_vp, i64] + [_vp] * 11 + [_vp]),
            pre + "_effective_radii_host": (rc, [_vp, i64] + [rp] * 11),
            pre + "_reflectivity_device": (rc, [_vp, i64, i32] + [_vp] * 8 + [_vp]),
            pre + "_reflectivity_host": (rc, [_vp, i64, i32] + [rp] * 8),
            pre + "_column_outputs_device": (rc, [_vp, i64, i32] + [_vp] * 11 + [outs, _vp]),
            pre + "_kernel_fingerprint": (text, [_vp] + arith),
            pre + "_kid_workspace_bytes": (size, [i64, i32]),
            pre + "_kid_workspace_offset": (size, [i64, i32, i32]),
            pre + "_kid_interface_device": (rc, kid + arith + [_vp, size, _vp]),
            pre + "_kid_interface_host": (rc, kid + arith),
            pre + "_kid_gather_device": (rc, kid[:11] + [_vp, _vp, size, _vp]),
        })
    return d


def load_library(path=None):
    """dlopen kid_amd/libkidmp.so (or an explicitly named build of it) and declare the C ABI (include/kidmp.h)."""
    global _lib
    if _lib is not None:
        if path is not None and os.path.abspath(path) != _lib._name:
            raise KidmpError("load_library: %s is already loaded" % _lib._name)
        return _lib
    path = os.path.abspath(path) if path else lib_path()
    # torch ships its own HIP runtime: when this process is going to use torch (the device entries of this mirror
    # take torch tensors) it must be loaded FIRST, so that libkidmp.so binds to the same libamdhip64 -- two HIP
    # runtimes in one process leave the second one without a device ("No HIP GPUs are available").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise KidmpError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
    L = C.CDLL(path)
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    _lib = L
    return L


def _np_dtype(dtype):
    """numpy's name for a numpy or torch floating dtype."""
    return str(dtype).replace("torch.", "") if type(dtype).__module__.split(".")[0] == "torch" else dtype


def _np_ptr(a, pt=_dp):
    return a.ctypes.data_as(pt)


def _stream(stream, like):
    """The stream an asynchronous entry runs on: the caller's, else torch's current stream on the device of `like`."""
    if stream is not None:
        return stream
    import torch
    return torch.cuda.current_stream(like.device).cuda_stream


def _pointers(st, names, optional, check, addr):
    """The arrays of the dict `st` under `names` as the addresses an entry takes, each judged by check(a, name).  A name
    in `optional` that is missing (or None) gives a null pointer: whether it may be left out is the library's to say."""
    out = []
    for k in names:
        a = st.get(k)
        if a is None and k in optional:
            out.append(None)
        else:
            check(a, k)
            out.append(addr(a))
    return out


def _host_check(who, dtype, shape):
    def check(a, k):
        if not (a.dtype == dtype and a.flags.c_contiguous and a.shape == shape):
            raise KidmpError("%s: %s must be contiguous %s [ncol, nz]" % (who, k, np.dtype(dtype).name))
    return check


def _outputs(dbz, radii, addr):
    """The kidmp_outputs that names `dbz` and the three `radii`; None = not wanted."""
    return _Outputs(addr(dbz) if dbz is not None else None, *([addr(a) for a in radii] if radii is not None else [None] * 3))


def _host_step(who, st, dtype, dt, ppt, want_rates, want_nstep):
    """What the host-array step entries share.  Checks the [ncol, nz] arrays of `st` (any of them may be missing: what
    KiD itself never fills, include/kidmp.h) and makes ppt, rates and nstep.  Returns (ppt, rates, nstep) and the
    arguments from ncol to nstep."""
    ncol, nz = st["qv"].shape
    pt = _dp if dtype == np.float64 else _fp
    ptrs = _pointers(st, KID_WORK_NAMES, KID_WORK_NAMES, _host_check(who, dtype, (ncol, nz)), lambda a: _np_ptr(a, pt))
    if ppt is None:
        ppt = np.zeros((ncol, 4), dtype=dtype)
    rates = np.zeros((ncol, NRATES, nz)) if want_rates else None
    nstep = np.zeros((ncol, 4), dtype=np.int32) if want_nstep else None
    return (ppt, rates, nstep), [ncol, nz, float(dt)] + ptrs + [_np_ptr(ppt, pt), _np_ptr(rates) if want_rates else None,
                                                                _np_ptr(nstep, _ip) if want_nstep else None]


class _PinnedBlock:
    """Owner of one kidmp_host_alloc block.  numpy arrays made from it (and their views) hold it as their base,
    so the block is freed when the last of them goes away."""

    def __init__(self, nbytes):
        self.nbytes = max(int(nbytes), 1)
        self.ptr = load_library().kidmp_host_alloc(self.nbytes)
        if not self.ptr:
            raise KidmpError("kidmp_host_alloc(%d) failed: %s" % (nbytes, load_library().kidmp_last_error(None).decode()))
        self.__array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 3}

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.kidmp_host_free(self.ptr)
            self.ptr = None


def host_empty(shape, dtype=np.float64):
    """numpy array in page-locked host memory (kidmp_host_alloc): what the host-array entries can move by DMA."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape))
    raw = np.asarray(_PinnedBlock(n * dtype.itemsize))       # base = the block
    return raw[: n * dtype.itemsize].view(dtype).reshape(shape)


def host_pinned_copy(a):
    """A page-locked copy of a numpy array."""
    b = host_empty(a.shape, a.dtype)
    b[...] = a
    return b


def column_nc_pointer(values, device=None):
    """What kidmp_set_column_nc takes, from a numpy array or a torch tensor (host or CUDA): (address, count) of a
    contiguous one-dimensional float64 array with at least one element.  Anything else raises KidmpError here, before
    the library is called; the values themselves (finite, > 0) are the library's to judge."""
    if isinstance(values, np.ndarray):
        if values.dtype != np.float64 or values.ndim != 1 or values.size == 0 or not values.flags.c_contiguous:
            raise KidmpError("set_column_nc: a numpy array must be contiguous float64 [ncol], ncol >= 1 (got %s %s)"
                             % (values.dtype, list(values.shape)))
        return values.ctypes.data, int(values.size)
    if type(values).__module__.split(".")[0] == "torch" and hasattr(values, "data_ptr"):
        import torch
        if values.dtype != torch.float64 or values.dim() != 1 or values.numel() == 0 or not values.is_contiguous():
            raise KidmpError("set_column_nc: a tensor must be contiguous float64 [ncol], ncol >= 1 (got %s %s)"
                             % (str(values.dtype).replace("torch.", ""), list(values.shape)))
        if values.is_cuda and device is not None and values.device.index != device:
            raise KidmpError("set_column_nc: the tensor lives on cuda:%d but this context is bound to cuda:%d"
                             % (values.device.index, device))
        return values.data_ptr(), int(values.numel())
    raise KidmpError("set_column_nc: expected a numpy array, a torch tensor or None, got %s" % type(values).__name__)


class ThompsonMP:
    """One context = the module state of module_mp_thompson09n after thompson_init:
    constants on the host, lookup tables resident in HBM."""

    def __init__(self, iiwarm=False, set_Nc=100.0, l_sediment=True, device=0, aerosol_aware=False):
        self._h = None
        L = load_library()
        cfg = _Cfg(int(bool(iiwarm)), int(bool(l_sediment)), float(set_Nc), int(device), int(bool(aerosol_aware)))
        self.aerosol_aware = bool(aerosol_aware)
        h = _vp()
        rc = L.kidmp_init(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise KidmpError("kidmp_init failed (%d): %s" % (rc, L.kidmp_last_error(None).decode()))
        self._h = h
        self.iiwarm = bool(iiwarm)
        self.device = int(device)
        self.init_seconds = L.kidmp_init_seconds(h)

    def close(self):
        if getattr(self, "_h", None):
            load_library().kidmp_finalize(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise KidmpError("kidmp error %d: %s" % (rc, load_library().kidmp_last_error(self._h).decode()))
        return rc

    # ---- mp_thompson(qv1d, ..., dt): host arrays, one column (M:1156-1177) ----
    def mp_thompson(self, qv1d, qc1d, qi1d, qr1d, qs1d, qg1d, ni1d, nr1d, nc1d, nwfa1d, nifa1d, t1d,
                    p1d, w1d, dzq, pptrain=0.0, pptsnow=0.0, pptgraul=0.0, pptice=0.0, dt=10.0):
        """Arrays (float64, length nz) are updated in place like the Fortran INOUT dummies.
        Returns the accumulated (pptrain, pptsnow, pptgraul, pptice)."""
        arrs = [qv1d, qc1d, qi1d, qr1d, qs1d, qg1d, ni1d, nr1d, nc1d, nwfa1d, nifa1d, t1d, p1d, w1d, dzq]
        nz = len(qv1d)
        for a in arrs:
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.shape == (nz,)):
                raise KidmpError("mp_thompson: arrays must be contiguous float64 of one length")
        ppt = np.array([pptrain, pptsnow, pptgraul, pptice], dtype=np.float64)
        self._check(load_library().kidmp_column_step(self._h, nz, float(dt), *[_np_ptr(a) for a in arrs], _np_ptr(ppt)))
        return tuple(ppt)

    # ---- batched host entry: numpy [ncol, nz] ----
    def _host_outputs(self, ncol, nz, dtype, want_dbz, want_radii):
        """The output arrays of a host step and the kidmp_outputs that names them."""
        dbz = np.empty((ncol, nz), dtype=dtype) if want_dbz else None
        radii = tuple(np.empty((ncol, nz), dtype=dtype) for _ in range(3)) if want_radii else None
        return dbz, radii, _outputs(dbz, radii, lambda a: a.ctypes.data)

    def batch_step_host(self, st, dt, ppt=None, want_rates=False, want_dbz=False, want_radii=False):
        """numpy float64 [ncol, nz] arrays, in place.  Keys KiD itself never fills may be missing (or None): nc, nwfa,
        nifa and w for a context without aerosol_aware, qi, qs, qg, ni for an iiwarm context (include/kidmp.h).
        Returns (ppt, rates); with want_dbz (ppt, rates, dbz): the reflectivity of the post-step state, formed on the
        device in the same call (kidmp_batch_step_host_refl).  want_radii appends (re_qc, re_qi, re_qs) of the
        post-step state in the form of the scheme's driver, presets where the species is absent
        (kidmp_batch_step_host_out: one launch per chunk for everything wanted)."""
        (ppt, rates, _), args = _host_step("batch_step_host", st, np.float64, dt, ppt, want_rates, False)
        ncol, nz = args[:2]
        L = load_library()
        if want_radii:
            dbz, radii, o = self._host_outputs(ncol, nz, np.float64, want_dbz, True)
            self._check(L.kidmp_batch_step_host_out(self._h, *args, C.byref(o)))
            return (ppt, rates, dbz, radii) if want_dbz else (ppt, rates, radii)
        if want_dbz:
            dbz = np.empty((ncol, nz))
            self._check(L.kidmp_batch_step_host_refl(self._h, *args, _np_ptr(dbz)))
            return ppt, rates, dbz
        self._check(L.kidmp_batch_step_host(self._h, *args[:-1]))            # the one entry without nstep
        return ppt, rates

    def _device_check(self, who, dtype, shape):
        return lambda a, k: self._want(a, dtype, shape, who + ": " + k)

    def _want(self, a, dtype, shape, what, key=""):
        """A device-entry argument: contiguous CUDA tensor of the given dtype/shape on THIS context's GPU.  A message
        names it `what` + `key` (two parts, so that a loop over keys does not join strings for tensors that are right)."""
        if not (a.is_cuda and a.dtype == dtype and a.is_contiguous() and tuple(a.shape) == tuple(shape)):
            raise KidmpError("%s must be a contiguous %s CUDA tensor %s" % (what + key, str(dtype).replace("torch.", ""), list(shape)))
        if a.device.index != self.device:
            raise KidmpError("%s lives on cuda:%d but this context is bound to cuda:%d" % (what + key, a.device.index, self.device))

    # ---- batched device entry: torch CUDA tensors [ncol, nz], in place ----
    def _step_device(self, who, st, dt, ppt, rates, nstep, stream, arith=None):
        """batch_step (arith None: float64 tensors, kidmp_batch_step_device) and batch_step32 (float32 tensors,
        kidmp32_batch_step_device).  On the clock of bench.py: nothing here that a call does not need."""
        import torch
        dtype = torch.float64 if arith is None else torch.float32
        q = st["qv"]
        ncol, nz = q.shape
        w = st.get("w")
        for k in _STEP_REQUIRED:
            self._want(st[k], dtype, (ncol, nz), who, k)
        if w is not None:
            self._want(w, dtype, (ncol, nz), who, "w")
        self._want(ppt, dtype, (ncol, 4), who, "ppt")
        if rates is not None:
            self._want(rates, torch.float64, (ncol, NRATES, nz), who, "rates")
        if nstep is not None:
            self._want(nstep, torch.int32, (ncol, 4), who, "nstep")
        s = _stream(stream, q)
        args = [st[k].data_ptr() for k in STATE_NAMES] + [st["p"].data_ptr(), w.data_ptr() if w is not None else None,
                                                          st["dz"].data_ptr(), ppt.data_ptr(),
                                                          rates.data_ptr() if rates is not None else None,
                                                          nstep.data_ptr() if nstep is not None else None]
        if arith is None:
            self._check(load_library().kidmp_batch_step_device(self._h, ncol, nz, float(dt), *args, s))
        else:
            self._check(load_library().kidmp32_batch_step_device(self._h, ncol, nz, float(dt), *args, self.ARITH[arith], s))

    def batch_step(self, st, dt, ppt, rates=None, nstep=None, stream=None):
        """st: dict of float64 CUDA tensors [ncol, nz] (STATE_NAMES + p, dz; w optional).
        ppt: float64 [ncol, 4], accumulated in place.  Asynchronous on `stream`
        (default: torch's current stream)."""
        self._step_device("batch_step: ", st, dt, ppt, rates, nstep, stream)

    # ---- binary32 state: the reference's native arithmetic ("p32n": REAL = binary32, DOUBLE PRECISION = binary64)
    #      and the all-binary32 build ("f32") -- include/kidmp.h, kidmp32_* ----
    ARITH = {"p32n": 0, "f32": 1}

    def batch_step32_host(self, st, dt, arith="p32n", ppt=None, want_rates=False, want_nstep=False, want_dbz=False,
                          want_radii=False):
        """numpy float32 [ncol, nz] arrays, in place.  Returns (ppt float32 [ncol, 4], rates float64 or None, nstep or None),
        with want_dbz a fourth element: the float32 reflectivity of the post-step state (kidmp32_batch_step_host_refl);
        want_radii appends the float32 (re_qc, re_qi, re_qs) of that state (kidmp32_batch_step_host_out)."""
        (ppt, rates, nstep), args = _host_step("batch_step32_host", st, np.float32, dt, ppt, want_rates, want_nstep)
        ncol, nz = args[:2]
        args.append(self.ARITH[arith])
        L = load_library()
        if want_radii:
            dbz, radii, o = self._host_outputs(ncol, nz, np.float32, want_dbz, True)
            self._check(L.kidmp32_batch_step_host_out(self._h, *args, C.byref(o)))
            return (ppt, rates, nstep, dbz, radii) if want_dbz else (ppt, rates, nstep, radii)
        if want_dbz:
            dbz = np.empty((ncol, nz), dtype=np.float32)
            self._check(L.kidmp32_batch_step_host_refl(self._h, *args, _np_ptr(dbz, _fp)))
            return ppt, rates, nstep, dbz
        self._check(L.kidmp32_batch_step_host(self._h, *args))
        return ppt, rates, nstep

    def batch_step32(self, st, dt, ppt, arith="p32n", rates=None, nstep=None, stream=None):
        """torch float32 CUDA tensors [ncol, nz], in place, asynchronous (the device entry of the binary32 builds)."""
        self._step_device("batch_step32: ", st, dt, ppt, rates, nstep, stream, arith)

    def default_aerosols(self, qv, t, p, stream=None):
        """nc, nwfa, nifa for the inputs the KiD wrapper leaves unset (W:36; formulas M:958-964)."""
        import torch
        for name, a in (("qv", qv), ("t", t), ("p", p)):
            self._want(a, torch.float64, tuple(qv.shape), "default_aerosols: " + name)
        nc, nwfa, nifa = torch.empty_like(qv), torch.empty_like(qv), torch.empty_like(qv)
        s = _stream(stream, qv)
        self._check(load_library().kidmp_default_aerosols_device(
            self._h, qv.numel(), qv.data_ptr(), t.data_ptr(), p.data_ptr(), nc.data_ptr(), nwfa.data_ptr(),
            nifa.data_ptr(), s))
        return nc, nwfa, nifa

    def set_column_nc(self, values):
        """Bind a droplet number per column (kidmp_set_column_nc): `values` is set_Nc in cm**-3, float64 [ncol], a
        numpy array or a torch tensor on the host or on this context's GPU; None unbinds.  While bound, column c of
        every batch steps with Nt_c = values[c]*1e6 (an Nd ensemble in one launch), batches must have exactly ncol
        columns, and the radii and default aerosols follow.  The values are copied: the array may go away."""
        if values is None:
            self._check(load_library().kidmp_set_column_nc(self._h, 0, None))
            return
        ptr, n = column_nc_pointer(values, self.device)
        self._check(load_library().kidmp_set_column_nc(self._h, n, ptr))

    @property
    def column_nc_count(self):
        """How many columns set_column_nc has bound; 0 when nothing is bound."""
        return int(load_library().kidmp_column_nc_count(self._h))

    def set_host_chunk(self, ncol_per_chunk):
        """Columns per pipeline chunk of the host-array entries (0 = default)."""
        self._check(load_library().kidmp_set_host_chunk(self._h, int(ncol_per_chunk)))

    def reduce_ppt(self, ppt, stream=None):
        """Domain sums of the surface precipitation on the device (W:248-275 analogue)."""
        import torch
        self._want(ppt, torch.float64, (ppt.shape[0], 4), "reduce_ppt: ppt")
        out = torch.empty(4, dtype=torch.float64, device=ppt.device)
        s = _stream(stream, ppt)
        self._check(load_library().kidmp_reduce_ppt_device(self._h, ppt.shape[0], ppt.data_ptr(), out.data_ptr(), s))
        return out

    def reduce_ppt_exact(self, ppt, stream=None):
        """The same four sums as exact fixed-point accumulators: int64 [PPT_LIMBS] on the device.  Integer sums are
        associative: multi-GPU callers all-reduce(SUM) the limbs and get identical bits for every partition of the
        columns; limbs_to_sums() converts."""
        import torch
        self._want(ppt, torch.float64, (ppt.shape[0], 4), "reduce_ppt_exact: ppt")
        out = torch.empty(PPT_LIMBS, dtype=torch.int64, device=ppt.device)
        s = _stream(stream, ppt)
        self._check(load_library().kidmp_reduce_ppt_exact_device(self._h, ppt.shape[0], ppt.data_ptr(), out.data_ptr(), s))
        return out

    def reduce_rates(self, rates, stream=None):
        """Sum over columns of the rate diagnostics: [ncol, 36, nz] -> [36, nz] (the nx-mean profiles KiD plots are
        this / ncol).  Fixed summation order."""
        import torch
        ncol, nr, nz = rates.shape
        self._want(rates, torch.float64, (ncol, NRATES, nz), "reduce_rates: rates")
        out = torch.empty(NRATES, nz, dtype=torch.float64, device=rates.device)
        s = _stream(stream, rates)
        self._check(load_library().kidmp_reduce_rates_device(self._h, ncol, nz, rates.data_ptr(), out.data_ptr(), s))
        return out

    def reserve(self, ncol, nz=120):
        """Deprecated no-op (kidmp_reserve): the step owns no per-batch device memory.  Kept so that hosts written
        against rounds 1-2 keep working; validates its arguments like every entry."""
        self._check(load_library().kidmp_reserve(self._h, int(ncol), int(nz)))

    SANITY_MAX = ("qc", "qr", "nr", "qs", "qi", "qg", "ni")
    SANITY_NEG = ("qc", "qr", "nr", "qs", "qi", "qg", "ni", "qv")

    def sanity(self, st, stream=None):
        """The post-step scan of the scheme's 3-D driver (M:1025-1094): [15] float64 on the device =
        maxima of SANITY_MAX, then counts of negative entries of SANITY_NEG."""
        import torch
        q = st["qv"]
        for k in self.SANITY_NEG:
            self._want(st[k], torch.float64, tuple(q.shape), "sanity: " + k)
        out = torch.empty(15, dtype=torch.float64, device=q.device)
        s = _stream(stream, q)
        self._check(load_library().kidmp_sanity_device(self._h, q.numel(), *[st[k].data_ptr() for k in self.SANITY_NEG],
                                                       out.data_ptr(), s))
        return out

    def effective_radii(self, st, preset=(2.49e-6, 4.99e-6, 9.99e-6), stream=None):
        """calc_effectRad (M:4834-4935): (re_qc, re_qi, re_qs) [ncol, nz] on the device, started from the presets of the
        scheme's driver (M:1111-1113).  A caller that wants the radii every step wants column_outputs: it does not fill
        three preset tensors first, and returns the reflectivity from the same read of the state."""
        import torch
        q = st["qv"]
        ptrs = _pointers(st, self.RADII_NAMES, (), self._device_check("effective_radii", torch.float64, tuple(q.shape)),
                         torch.Tensor.data_ptr)
        out = [torch.full_like(q, v) for v in preset]
        s = _stream(stream, q)
        self._check(load_library().kidmp_effective_radii_device(self._h, q.numel(), *ptrs, *[o.data_ptr() for o in out], s))
        return tuple(out)

    RADII_NAMES = ("t", "p", "qv", "qc", "nc", "qi", "ni", "qs")                    # calc_effectRad's IN dummies, M:4842
    OUTPUT_NAMES = ("t", "p", "qv", "qc", "nc", "qi", "ni", "qr", "nr", "qs", "qg")   # kidmp_column_outputs_device

    def effective_radii_host(self, st, preset=(2.49e-6, 4.99e-6, 9.99e-6)):
        """calc_effectRad on numpy arrays [ncol, nz] (float64 or float32, keys RADII_NAMES): (re_qc, re_qi, re_qs) of
        the same dtype (kidmp_effective_radii_host / kidmp32_effective_radii_host), INOUT like the subroutine.
        `preset`: three scalars to start from, or three arrays that are updated in place and returned.  nc may be
        missing (or None) unless the context is aerosol-aware; qi + ni and qs in an iiwarm context, where re_qi and
        re_qs are then returned as they were preset."""
        q = st["t"]
        if q.dtype not in (np.float64, np.float32) or q.ndim != 2:
            raise KidmpError("effective_radii_host: state must be float64 or float32 numpy arrays [ncol, nz]")
        pt = _dp if q.dtype == np.float64 else _fp
        ptrs = _pointers(st, self.RADII_NAMES, ("nc", "qi", "ni", "qs"), _host_check("effective_radii_host", q.dtype, q.shape),
                         lambda a: _np_ptr(a, pt))
        out = []
        for v in preset:
            if isinstance(v, np.ndarray):
                if not (v.dtype == q.dtype and v.flags.c_contiguous and v.shape == q.shape):
                    raise KidmpError("effective_radii_host: preset arrays must match the state")
                out.append(v)
            else:
                out.append(np.full(q.shape, v, dtype=q.dtype))
        fn = load_library().kidmp_effective_radii_host if q.dtype == np.float64 else load_library().kidmp32_effective_radii_host
        self._check(fn(self._h, q.size, *ptrs, *[_np_ptr(o, pt) for o in out]))
        return tuple(out)

    def column_outputs(self, st, dbz=True, radii=True, stream=None):
        """What a host model takes from the state beside the step (kidmp_column_outputs_device): the reflectivity of
        calc_refl10cm and the effective radii of calc_effectRad in the driver's form (preset where the species is
        absent, M:1111-1116), of float64 or float32 CUDA tensors [ncol, nz] with the keys OUTPUT_NAMES.  nc may be
        missing unless the context is aerosol-aware, qi + ni and qs + qg in an iiwarm context.  With both wanted, one
        kernel reads the column once.  Returns (dbz, (re_qc, re_qi, re_qs)), None for what was not asked for.
        Asynchronous on `stream`."""
        import torch
        q = st["t"]
        if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2:
            raise KidmpError("column_outputs: state must be float64 or float32 CUDA tensors [ncol, nz]")
        ncol, nz = q.shape
        ptrs = _pointers(st, self.OUTPUT_NAMES, self.OUTPUT_NAMES, self._device_check("column_outputs", q.dtype, (ncol, nz)),
                         torch.Tensor.data_ptr)
        o_dbz = torch.empty_like(q) if dbz else None
        o_rad = tuple(torch.empty_like(q) for _ in range(3)) if radii else None
        o = _outputs(o_dbz, o_rad, torch.Tensor.data_ptr)
        s = _stream(stream, q)
        fn = load_library().kidmp_column_outputs_device if q.dtype == torch.float64 else load_library().kidmp32_column_outputs_device
        self._check(fn(self._h, ncol, nz, *ptrs, C.byref(o), s))
        return o_dbz, o_rad

    def level_stats(self, fields, group=None, ngroup=1, edges=None, floor=None, work=None, stream=None):
        """Moments and histograms of [ncol, nz] CUDA tensors over the columns, per level and per ensemble group
        (include/kidmp_stats.h): kid_amd.stats.level_stats on this context."""
        from .stats import level_stats
        return level_stats(self, fields, group, ngroup, edges, floor, work, stream)

    def column_summary(self, st, dz, cfg=None, out=None, stream=None):
        """Water paths, cloud optical depth, echo and cloud heights: [ncol, 16] float64 on the device, one number per
        column and slot (include/kidmp_summary.h): kid_amd.summary.column_summary on this context."""
        from .summary import column_summary
        return column_summary(self, st, dz, cfg, out, stream)

    def column_summary_host(self, st, dz, cfg=None):
        """column_summary on numpy arrays: kid_amd.summary.column_summary_host on this context."""
        from .summary import column_summary_host
        return column_summary_host(self, st, dz, cfg)

    def fall_speeds(self, st, boost=None, dz=None, dt=None, want=None, stream=None):
        """Block-O fall speeds and sedimentation fluxes of every level, and the substep counts when dz and dt are given
        (include/kidmp_fall.h): kid_amd.fall.fall_speeds on this context."""
        from .fall import FALL_NAMES, fall_speeds
        return fall_speeds(self, st, boost, dz, dt, FALL_NAMES if want is None else want, stream)

    def fall_speeds_host(self, st, boost=None, dz=None, dt=None, want=None):
        """fall_speeds on numpy arrays: kid_amd.fall.fall_speeds_host on this context."""
        from .fall import FALL_NAMES, fall_speeds_host
        return fall_speeds_host(self, st, boost, dz, dt, FALL_NAMES if want is None else want)

    def size_spectra(self, st, want=None, grids=None, out=None, stream=None):
        """The size distributions of every level on diameter bins, and their parameters (include/kidmp_spectra.h):
        kid_amd.spectra.size_spectra on this context."""
        from .spectra import SPECTRA_SPECIES, size_spectra
        return size_spectra(self, st, SPECTRA_SPECIES if want is None else want, grids, out, stream)

    def size_spectra_host(self, st, want=None, grids=None, out=None):
        """size_spectra on numpy arrays: kid_amd.spectra.size_spectra_host on this context."""
        from .spectra import SPECTRA_SPECIES, size_spectra_host
        return size_spectra_host(self, st, SPECTRA_SPECIES if want is None else want, grids, out)

    def doppler_moments(self, st, w=None, want=None, stream=None):
        """Reflectivity, mean Doppler velocity and spectrum width of every level, with the per-species parts they are
        formed from (include/kidmp_doppler.h): kid_amd.doppler.doppler_moments on this context."""
        from .doppler import DOPPLER_NAMES, doppler_moments
        return doppler_moments(self, st, w, DOPPLER_NAMES if want is None else want, stream)

    def doppler_moments_host(self, st, w=None, want=None):
        """doppler_moments on numpy arrays: kid_amd.doppler.doppler_moments_host on this context."""
        from .doppler import DOPPLER_NAMES, doppler_moments_host
        return doppler_moments_host(self, st, w, DOPPLER_NAMES if want is None else want)

    def lidar_profiles(self, st, dz=None, cfg=None, want=None, summary=False, stream=None):
        """Extinction, backscatter, optical depth and attenuated backscatter of every level as a lidar on the ground and
        one in space see them (include/kidmp_lidar.h): kid_amd.lidar.lidar_profiles on this context."""
        from .lidar import LIDAR_NAMES, lidar_profiles
        return lidar_profiles(self, st, dz, cfg, LIDAR_NAMES if want is None else want, summary, stream)

    def lidar_profiles_host(self, st, dz=None, cfg=None, want=None, summary=False):
        """lidar_profiles on numpy arrays: kid_amd.lidar.lidar_profiles_host on this context."""
        from .lidar import LIDAR_NAMES, lidar_profiles_host
        return lidar_profiles_host(self, st, dz, cfg, LIDAR_NAMES if want is None else want, summary)

    def doppler_spectrum(self, st, v0, dv, nv, w=None, grids=None, want=("total",), out=None, stream=None):
        """The Doppler spectrum of every level on a uniform velocity grid (include/kidmp_dspectrum.h):
        kid_amd.dspectrum.doppler_spectrum on this context."""
        from .dspectrum import doppler_spectrum
        return doppler_spectrum(self, st, v0, dv, nv, w, grids, want, out, stream)

    def spectrum_process(self, spec, v0, dv, sigma=None, noise=None, cfg=None,
                         want=("dbz", "vm", "sw", "skew", "kurt", "v_lo", "v_hi", "nbins"), out=None, stream=None):
        """Broadening, noise floor, detection and moments of spectra [ncol, nv, nz] (include/kidmp_specproc.h):
        kid_amd.specproc.spectrum_process on this context."""
        from .specproc import spectrum_process
        return spectrum_process(self, spec, v0, dv, sigma, noise, cfg, want, out, stream)

    def doppler_spectrum_host(self, st, v0, dv, nv, w=None, grids=None, want=("total",), out=None):
        """doppler_spectrum on numpy arrays: kid_amd.dspectrum.doppler_spectrum_host on this context."""
        from .dspectrum import doppler_spectrum_host
        return doppler_spectrum_host(self, st, v0, dv, nv, w, grids, want, out)

    def bright_band(self, st, cfg=None, grids=None, want=("dbz",), out=None, stream=None):
        """calc_refl10cm with melting snow and graupel below the melting level (include/kidmp_brightband.h):
        kid_amd.brightband.bright_band on this context."""
        from .brightband import bright_band
        return bright_band(self, st, cfg, grids, want, out, stream)

    def bright_band_host(self, st, cfg=None, grids=None, want=("dbz",), out=None):
        """bright_band on numpy arrays: kid_amd.brightband.bright_band_host on this context."""
        from .brightband import bright_band_host
        return bright_band_host(self, st, cfg, grids, want, out)

    def mie_table(self, cfg=None, grids=None):
        """The Mie rows of rain, snow and graupel for one wavelength on this context's device (include/kidmp_mie.h):
        a kid_amd.mie.MieTable."""
        from .mie import MieTable
        return MieTable(self, cfg, grids)

    def mie_radar(self, table, st, dz=None, w=None, k_gas=None, want=("dbz",), out=None, stream=None):
        """Mie reflectivity, extinction, path-integrated attenuation and mean Doppler velocity at the table's wavelength:
        kid_amd.mie.mie_radar on this context."""
        from .mie import mie_radar
        return mie_radar(self, table, st, dz, w, k_gas, want, out, stream)

    def mie_radar_host(self, table, st, dz=None, w=None, k_gas=None, want=("dbz",), out=None):
        """mie_radar on numpy arrays: kid_amd.mie.mie_radar_host on this context."""
        from .mie import mie_radar_host
        return mie_radar_host(self, table, st, dz, w, k_gas, want, out)

    def scan(self, fields, zf, rays, dx, nx, cfg, want=("dbz_att",), out=None, stream=None):
        """A range-height radar scan of an x-z slab (slant beams, path attenuation, beam broadening, radial velocity):
        kid_amd.scan.scan on this context."""
        from .scan import scan
        return scan(self, fields, zf, rays, dx, nx, cfg, want, out, stream)

    def pol_table(self, mie_cfg=None, pol_cfg=None, grids=None):
        """The spheroid rows of rain, snow and graupel on this context's device (include/kidmp_polarimetric.h): a
        kid_amd.polarimetric.PolTable."""
        from .polarimetric import PolTable
        return PolTable(self, mie_cfg, pol_cfg, grids)

    def polarimetric(self, table, st, want=("dbz_h", "zdr", "kdp", "rhohv"), out=None, stream=None):
        """Z_DR, K_DP, rho_hv and the reflectivity at horizontal polarisation of oblate spheroids:
        kid_amd.polarimetric.polarimetric on this context."""
        from .polarimetric import polarimetric
        return polarimetric(self, table, st, want, out, stream)

    def polarimetric_host(self, table, st, want=("dbz_h", "zdr", "kdp", "rhohv"), out=None):
        """polarimetric on numpy arrays: kid_amd.polarimetric.polarimetric_host on this context."""
        from .polarimetric import polarimetric_host
        return polarimetric_host(self, table, st, want, out)

    def radiometer_table(self, cfg=None, grids=None):
        """The radiometer's rows of rain, snow and graupel for one wavelength on this context's device
        (include/kidmp_radiometer.h): a kid_amd.radiometer.RadiometerTable."""
        from .radiometer import RadiometerTable
        return RadiometerTable(self, cfg, grids)

    def radiometer(self, table, st, dz=None, k_gas=None, t_sfc=None, rcfg=None, want=("tb_toa",), out=None, stream=None):
        """Two-stream brightness temperatures at the table's wavelength, seen from the ground and from orbit:
        kid_amd.radiometer.radiometer on this context."""
        from .radiometer import radiometer
        return radiometer(self, table, st, dz, k_gas, t_sfc, rcfg, want, out, stream)

    def radiometer_host(self, table, st, dz=None, k_gas=None, t_sfc=None, rcfg=None, want=("tb_toa",), out=None):
        """radiometer on numpy arrays: kid_amd.radiometer.radiometer_host on this context."""
        from .radiometer import radiometer_host
        return radiometer_host(self, table, st, dz, k_gas, t_sfc, rcfg, want, out)

    def radiometer_multi(self, tables, st, dz=None, k_gas=None, t_sfc=None, rcfgs=None, want=("tb_toa",), out=None, stream=None):
        """The radiometer at len(tables) channels in one launch (include/kidmp_multichannel.h):
        kid_amd.multichannel.radiometer_multi on this context."""
        from .multichannel import radiometer_multi
        return radiometer_multi(self, tables, st, dz, k_gas, t_sfc, rcfgs, want, out, stream)

    def radiometer_multi_host(self, tables, st, dz=None, k_gas=None, t_sfc=None, rcfgs=None, want=("tb_toa",), out=None):
        """radiometer_multi on numpy arrays: kid_amd.multichannel.radiometer_multi_host on this context."""
        from .multichannel import radiometer_multi_host
        return radiometer_multi_host(self, tables, st, dz, k_gas, t_sfc, rcfgs, want, out)

    def mie_radar_multi(self, tables, st, dz=None, w=None, k_gas=None, want=("dbz",), out=None, stream=None):
        """The cloud radar at len(tables) channels in one launch (include/kidmp_multichannel.h):
        kid_amd.multichannel.mie_radar_multi on this context."""
        from .multichannel import mie_radar_multi
        return mie_radar_multi(self, tables, st, dz, w, k_gas, want, out, stream)

    def mie_radar_multi_host(self, tables, st, dz=None, w=None, k_gas=None, want=("dbz",), out=None):
        """mie_radar_multi on numpy arrays: kid_amd.multichannel.mie_radar_multi_host on this context."""
        from .multichannel import mie_radar_multi_host
        return mie_radar_multi_host(self, tables, st, dz, w, k_gas, want, out)

    REFL_NAMES = ("t", "p", "qv", "qr", "nr", "qs", "qg")      # the inputs of calc_refl10cm that are read (qc1d is not)

    def reflectivity(self, st, out=None, stream=None):
        """calc_refl10cm (M:4946-5244): 10-cm radar reflectivity in dBZ, [ncol, nz] on the device, of the state in `st`
        (float64 or float32 CUDA tensors [ncol, nz] with the keys REFL_NAMES; qs and qg may be missing or None in an
        iiwarm context).  float32 state is widened, computed in binary64 and rounded once.  Asynchronous on `stream`."""
        import torch
        q = st["t"]
        if q.dtype not in (torch.float64, torch.float32) or q.dim() != 2:
            raise KidmpError("reflectivity: state must be float64 or float32 CUDA tensors [ncol, nz]")
        ncol, nz = q.shape
        ptrs = _pointers(st, self.REFL_NAMES, ("qs", "qg"), self._device_check("reflectivity", q.dtype, (ncol, nz)),
                         torch.Tensor.data_ptr)
        if out is None:
            out = torch.empty((ncol, nz), dtype=q.dtype, device=q.device)
        self._want(out, q.dtype, (ncol, nz), "reflectivity: out")
        s = _stream(stream, q)
        fn = load_library().kidmp_reflectivity_device if q.dtype == torch.float64 else load_library().kidmp32_reflectivity_device
        self._check(fn(self._h, ncol, nz, *ptrs, out.data_ptr(), s))
        return out

    def reflectivity_host(self, st):
        """calc_refl10cm on numpy arrays [ncol, nz] (float64 or float32, keys REFL_NAMES; qs/qg optional in an iiwarm
        context): returns dbz of the same dtype (kidmp_reflectivity_host / kidmp32_reflectivity_host)."""
        q = st["t"]
        if q.dtype not in (np.float64, np.float32) or q.ndim != 2:
            raise KidmpError("reflectivity_host: state must be float64 or float32 numpy arrays [ncol, nz]")
        ncol, nz = q.shape
        pt = _dp if q.dtype == np.float64 else _fp
        ptrs = _pointers(st, self.REFL_NAMES, ("qs", "qg"), _host_check("reflectivity_host", q.dtype, (ncol, nz)),
                         lambda a: _np_ptr(a, pt))
        out = np.empty((ncol, nz), dtype=q.dtype)
        fn = load_library().kidmp_reflectivity_host if q.dtype == np.float64 else load_library().kidmp32_reflectivity_host
        self._check(fn(self._h, ncol, nz, *ptrs, _np_ptr(out, pt)))
        return out

    # ---- mphys_thompson09_interfacen (W:28-310): KiD's theta-form fields in, tendencies out ----
    @staticmethod
    def kid_workspace_bytes(ncol, nz, dtype):
        """kidmp[32]_kid_workspace_bytes: 15 profiles of ncol*nz values, each stride rounded up to 256 bytes."""
        L = load_library()
        fn = L.kidmp_kid_workspace_bytes if np.dtype(_np_dtype(dtype)) == np.float64 else L.kidmp32_kid_workspace_bytes
        return int(fn(int(ncol), int(nz)))

    def kid_workspace(self, ncol, nz, dtype):
        """The workspace of kid_interface for [ncol, nz] fields of `dtype` (torch or numpy float64 / float32): a uint8
        tensor on this context's GPU.  After a call it holds the post-step state: see kid_workspace_views."""
        import torch
        n = self.kid_workspace_bytes(ncol, nz, dtype)
        if n == 0 and ncol > 0:
            raise KidmpError("kid_workspace: bad ncol / nz (%d, %d)" % (ncol, nz))
        return torch.empty(max(n, 1), dtype=torch.uint8, device="cuda:%d" % self.device)

    @staticmethod
    def kid_workspace_views(work, ncol, nz, dtype):
        """dict name -> [ncol, nz] view of the workspace, names KID_WORK_NAMES (the state in the order of mp_thompson's
        dummies, then p, w, dz), placed by kidmp[32]_kid_workspace_offset."""
        import torch
        L = load_library()
        is64 = np.dtype(_np_dtype(dtype)) == np.float64
        off = L.kidmp_kid_workspace_offset if is64 else L.kidmp32_kid_workspace_offset
        tdt, size = (torch.float64, 8) if is64 else (torch.float32, 4)
        return {k: work[off(ncol, nz, v): off(ncol, nz, v) + ncol * nz * size].view(tdt).view(ncol, nz)
                for v, k in enumerate(KID_WORK_NAMES)}

    def _kid_members(self, who, d, name, required, check):
        """The members of one kidmp_kid_fields argument: `d` is a dict (or None = all absent) with keys KID_FIELDS.
        In an iiwarm context the frozen members are not looked at.  Returns the list of present (key, array)."""
        if d is None:
            if required:
                raise KidmpError("%s: %s is required" % (who, name))
            return []
        if not isinstance(d, dict):
            raise KidmpError("%s: %s must be a dict with keys from %s" % (who, name, ", ".join(KID_FIELDS)))
        bad = [k for k in d if k not in KID_FIELDS]
        if bad:
            raise KidmpError("%s: %s has unknown members %s" % (who, name, bad))
        keys = KID_FIELDS[:5] if self.iiwarm else KID_FIELDS
        got = []
        for k in keys:
            a = d.get(k)
            if a is None:
                if required:
                    raise KidmpError("%s: %s[%r] is required%s" % (who, name, k, "" if k in KID_FIELDS[:5] else " in a mixed-phase context"))
                continue
            check(a, "%s: %s[%r]" % (who, name, k))
            got.append((k, a))
        return got

    def _kid_interface(self, who, q, is64, check, addr, outputs, state, dt, p0, r_on_cp, exner, dz, adv, div, dbz, radii, arith):
        """What kid_interface and kid_interface_host share.  They differ in how an array is judged (check(a, what[, shape])),
        in how its address is taken (addr) and in outputs(keys), which checks or makes what the call writes: the
        dict that is returned -- a tendency for each of `keys`, ppt, dbz / radii when wanted -- and rates, nstep or None.
        Returns that dict, the 16 arguments every entry begins with and, for the kidmp32_* entries, [arith]."""
        ncol, nz = q.shape
        if is64 and arith is not None:
            raise KidmpError("%s: arith applies to float32 fields only" % who)
        if not is64 and (arith or "p32n") not in self.ARITH:
            raise KidmpError("%s: arith must be 'p32n' or 'f32'" % who)
        f_state = self._kid_members(who, state, "state", True, check)
        f_adv = self._kid_members(who, adv, "adv", False, check)
        f_div = self._kid_members(who, div, "div", False, check)
        check(exner, who + ": exner")
        check(dz, who + ": dz", (nz,))
        keys = [k for k, _ in f_state]
        res, rates, nstep = outputs(keys)

        def fields(members):
            d = dict(members)
            return _KidFields(*[addr(d[k]) if k in d else None for k in KID_FIELDS])
        c_state, c_adv, c_div = fields(f_state), fields(f_adv), fields(f_div)
        c_out = fields([(k, res[k]) for k in keys if k in res])
        o = _outputs(res["dbz"] if dbz else None, res["radii"] if radii else None, addr)
        args = [self._h, ncol, nz, float(dt), float(p0), float(r_on_cp), C.byref(c_state), C.byref(c_adv) if adv is not None else None,
                C.byref(c_div) if div is not None else None, addr(exner), addr(dz), C.byref(c_out), addr(res["ppt"]),
                addr(rates) if rates is not None else None, addr(nstep) if nstep is not None else None,
                C.byref(o) if (dbz or radii) else None]
        return res, args, [] if is64 else [self.ARITH[arith or "p32n"]]

    def kid_interface(self, state, dt, p0, r_on_cp, exner, dz, adv=None, div=None, work=None, rates=None, nstep=None,
                      dbz=False, radii=False, arith=None, stream=None, out=None, gather_only=False):
        """The KiD adapter on the device (kidmp[32]_kid_interface_device).  state / adv / div: dicts of float64 or float32
        CUDA tensors [ncol, nz] with keys from KID_FIELDS (adv, div and any of their members may be missing: zero;
        the frozen members only matter in a mixed-phase context); exner [ncol, nz]; dz [nz].  Returns a dict: the
        tendencies under the keys of KID_FIELDS, "ppt" [ncol, 4] (rain, snow, graupel, ice), with dbz / radii also "dbz" /
        "radii" of the post-step state, and "work", the workspace (kid_workspace_views).  `out`: a dict returned by
        an earlier call, whose tensors are then written again (nothing is allocated: what a captured graph needs).
        float32 fields step in `arith` "p32n" (default) or "f32"; `rates` stays float64.  Asynchronous on `stream`.
        gather_only (kidmp[32]_kid_gather_device): only the workspace is filled with the step's inputs and ppt zeroed;
        returns {"ppt", "work"}."""
        import torch
        q = state.get("theta") if isinstance(state, dict) else None
        if q is None or not hasattr(q, "is_cuda") or q.dtype not in (torch.float64, torch.float32) or q.dim() != 2:
            raise KidmpError("kid_interface: state['theta'] must be a float64 or float32 CUDA tensor [ncol, nz]")
        ncol, nz = q.shape
        is64 = q.dtype == torch.float64

        def check(a, what, shape=(ncol, nz)):
            if not hasattr(a, "is_cuda"):
                raise KidmpError("%s must be a torch tensor" % what)
            self._want(a, q.dtype, shape, what)

        def outputs(keys):
            if rates is not None:
                self._want(rates, torch.float64, (ncol, NRATES, nz), "kid_interface: rates")
            if nstep is not None:
                self._want(nstep, torch.int32, (ncol, 4), "kid_interface: nstep")
            need = 15 * ((ncol * nz * q.element_size() + 255) // 256 * 256)
            if work is not None:
                if not (hasattr(work, "is_cuda") and work.is_cuda and work.dtype == torch.uint8 and work.dim() == 1 and work.is_contiguous()
                        and work.device.index == self.device and work.numel() >= need and work.data_ptr() % 16 == 0):
                    raise KidmpError("kid_interface: work must be a contiguous uint8 CUDA tensor of at least %d bytes on cuda:%d "
                                     "(kid_workspace)" % (need, self.device))
            if out is not None:
                if not isinstance(out, dict) or out.get("ppt") is None or (dbz and out.get("dbz") is None) or (radii and out.get("radii") is None):
                    raise KidmpError("kid_interface: out must be a dict holding ppt (and dbz / radii when they are wanted)")
                self._kid_members("kid_interface", {k: out.get(k) for k in KID_FIELDS}, "out", True, check)
                self._want(out["ppt"], q.dtype, (ncol, 4), "kid_interface: out['ppt']")
                res = out
            else:
                res = {k: torch.empty_like(q) for k in ([] if gather_only else keys)}
                res["ppt"] = torch.empty((ncol, 4), dtype=q.dtype, device=q.device)
                if dbz:
                    res["dbz"] = torch.empty_like(q)
                if radii:
                    res["radii"] = tuple(torch.empty_like(q) for _ in range(3))
            if dbz:
                check(res["dbz"], "kid_interface: out['dbz']")
            if radii:
                for a in res["radii"]:
                    check(a, "kid_interface: out['radii']")
            res["work"] = work if work is not None else self.kid_workspace(ncol, nz, q.dtype)
            return res, rates, nstep
        res, args, code = self._kid_interface("kid_interface", q, is64, check, torch.Tensor.data_ptr, outputs, state, dt, p0,
                                              r_on_cp, exner, dz, adv, div, dbz, radii, arith)
        work = res["work"]
        s = _stream(stream, q)
        L = load_library()
        if gather_only:
            fn = L.kidmp_kid_gather_device if is64 else L.kidmp32_kid_gather_device
            self._check(fn(*args[:11], res["ppt"].data_ptr(), work.data_ptr(), work.numel(), s))
            return {"ppt": res["ppt"], "work": work}
        fn = L.kidmp_kid_interface_device if is64 else L.kidmp32_kid_interface_device
        self._check(fn(*args, *code, work.data_ptr(), work.numel(), s))
        return res

    def kid_interface_host(self, state, dt, p0, r_on_cp, exner, dz, adv=None, div=None, want_rates=False, want_nstep=False,
                           dbz=False, radii=False, arith=None):
        """The KiD adapter on numpy arrays (kidmp[32]_kid_interface_host): arguments as kid_interface, float64 or float32
        arrays [ncol, nz] (page-locked ones, host_empty, move by DMA).  Returns the dict of tendencies and "ppt", with
        "rates" / "nstep" / "dbz" / "radii" when asked for.  Bit for bit the device entry, for any chunking."""
        q = state.get("theta") if isinstance(state, dict) else None
        if not isinstance(q, np.ndarray) or q.dtype not in (np.float64, np.float32) or q.ndim != 2:
            raise KidmpError("kid_interface_host: state['theta'] must be a float64 or float32 numpy array [ncol, nz]")
        ncol, nz = q.shape
        is64 = q.dtype == np.float64

        def check(a, what, shape=(ncol, nz)):
            if not (isinstance(a, np.ndarray) and a.dtype == q.dtype and a.flags.c_contiguous and a.shape == shape):
                raise KidmpError("%s must be a contiguous %s numpy array %s" % (what, q.dtype, list(shape)))

        def outputs(keys):
            res = {k: np.empty_like(q) for k in keys}
            res["ppt"] = np.empty((ncol, 4), dtype=q.dtype)
            if want_rates:
                res["rates"] = np.zeros((ncol, NRATES, nz))
            if want_nstep:
                res["nstep"] = np.zeros((ncol, 4), dtype=np.int32)
            if dbz:
                res["dbz"] = np.empty_like(q)
            if radii:
                res["radii"] = tuple(np.empty_like(q) for _ in range(3))
            return res, res.get("rates"), res.get("nstep")
        res, args, code = self._kid_interface("kid_interface_host", q, is64, check, lambda a: a.ctypes.data, outputs, state, dt, p0,
                                              r_on_cp, exner, dz, adv, div, dbz, radii, arith)
        L = load_library()
        fn = L.kidmp_kid_interface_host if is64 else L.kidmp32_kid_interface_host
        self._check(fn(*args, *code))
        return res

    def kid_advect(self, state, w, rho, dz, dt, want=("sum",), courant=False, out=None, stream=None):
        """Prescribed-w vertical advection of KiD's fields in the adapter's adv / div form (include/kidmp_kinematic.h):
        kid_amd.kinematic.advect on this context."""
        from .kinematic import advect
        return advect(self, state, w, rho, dz, dt, want, courant, out, stream)

    def kid_update(self, state, dt, *tendencies, clip=True, stream=None):
        """state <- state + (t1 + t2 + t3)*dt in place, with the clip at zero: kid_amd.kinematic.update on this context."""
        from .kinematic import update
        return update(self, state, dt, *tendencies, clip=clip, stream=stream)

    def kid_run(self, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, w, fix_theta=False, on_step=None, stream=None, **kid_interface_options):
        """A device-resident 1-D KiD case, advect -> kid_interface -> update per step: kid_amd.kinematic.run on this context."""
        from .kinematic import run
        return run(self, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, w, fix_theta, on_step, stream, **kid_interface_options)

    def kid_advect_slab(self, state, u, w, rho, dz, dx, dt, nx, want=("sum",), courant=False, out=None, stream=None):
        """Prescribed-(u, w) advection on periodic x-z slabs in the adapter's adv / div form (include/kidmp_slab.h):
        kid_amd.slab.advect_slab on this context."""
        from .slab import advect_slab
        return advect_slab(self, state, u, w, rho, dz, dx, dt, nx, want, courant, out, stream)

    def kid_run_slab(self, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, dx, nx, u, w, fix_theta=False, on_step=None, stream=None,
                     **kid_interface_options):
        """A device-resident x-z KiD case, advect_slab -> kid_interface -> update per step: kid_amd.slab.run_slab on this context."""
        from .slab import run_slab
        return run_slab(self, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, dx, nx, u, w, fix_theta, on_step, stream, **kid_interface_options)

    # ---- prognostic aerosols in the KiD path (include/kidmp_aerosol.h): kid_amd.aerosol on this context ----
    def kid_interface_aero(self, state, dt, p0, r_on_cp, exner, dz, **options):
        """The KiD adapter with nc, nwfa and nifa as state and the updraft w: kid_amd.aerosol.kid_interface_aero."""
        from .aerosol import kid_interface_aero
        return kid_interface_aero(self, state, dt, p0, r_on_cp, exner, dz, **options)

    def kid_advect_aero(self, state, w, rho, dz, dt, want=("sum",), out=None, stream=None):
        """Vertical advection of the aerosols: kid_amd.aerosol.advect_aero."""
        from .aerosol import advect_aero
        return advect_aero(self, state, w, rho, dz, dt, want, out, stream)

    def kid_advect_slab_aero(self, state, u, w, rho, dz, dx, dt, nx, want=("sum",), out=None, stream=None):
        """x-z advection of the aerosols on periodic slabs: kid_amd.aerosol.advect_slab_aero."""
        from .aerosol import advect_slab_aero
        return advect_slab_aero(self, state, u, w, rho, dz, dx, dt, nx, want, out, stream)

    def kid_update_aero(self, state, dt, *tendencies, clip=True, stream=None):
        """nc, nwfa, nifa <- A + (t1 + t2 + t3)*dt in place, with the clip at zero: kid_amd.aerosol.update_aero."""
        from .aerosol import update_aero
        return update_aero(self, state, dt, *tendencies, clip=clip, stream=stream)

    def kid_run_aero(self, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, w, nwfa_source=None, fix_theta=False, on_step=None, stream=None,
                     **kid_interface_options):
        """A device-resident 1-D KiD case with prognostic aerosols: kid_amd.aerosol.run_aero."""
        from .aerosol import run_aero
        return run_aero(self, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, w, nwfa_source, fix_theta, on_step, stream,
                        **kid_interface_options)

    def kid_run_slab_aero(self, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, dx, nx, u, w, nwfa_source=None, fix_theta=False,
                          on_step=None, stream=None, **kid_interface_options):
        """A device-resident x-z KiD case with prognostic aerosols: kid_amd.aerosol.run_slab_aero."""
        from .aerosol import run_slab_aero
        return run_slab_aero(self, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, dx, nx, u, w, nwfa_source, fix_theta, on_step, stream,
                             **kid_interface_options)

    # ---- the advection scheme of the KiD path (include/kidmp_advection.h): kid_amd.advection on this context ----
    def set_advection(self, name):
        """Select the scheme of every later kid_advect*, kid_run* call: "vanleer" (a new context's) or "ultimate"."""
        from .advection import set_scheme
        return set_scheme(self, name)

    @property
    def advection(self):
        """The name of the scheme this context advects with."""
        from .advection import scheme
        return scheme(self)

    def kernel_fingerprint(self, arith="p64"):
        """'src:<hash>;vgpr:<n>;lds:<bytes>;scratch:<bytes>' of this context's nz <= 120 column-step kernel, in the
        parity arithmetic (p64) or one of the binary32 ones (p32n, f32)."""
        if arith == "p64":
            return load_library().kidmp_kernel_fingerprint(self._h).decode()
        return load_library().kidmp32_kernel_fingerprint(self._h, {"p32n": 0, "f32": 1}[arith]).decode()

    # ---- introspection for parity tests ----
    MATH_FUNCS = ("log", "log10", "exp", "exp10", "sqrt", "cbrt", "pow", "rcp_seed", "div", "ieee_div", "rcp")

    def math_probe(self, fn, x, y=None):
        """Evaluate one of the column kernel's fp64 math helpers (csrc/fastmath.h) on the device, elementwise."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(x if y is None else y, dtype=np.float64)
        out = np.empty_like(x)
        self._check(load_library().kidmp_math_probe(self._h, self.MATH_FUNCS.index(fn), x.size, _np_ptr(x), _np_ptr(y),
                                                    _np_ptr(out)))
        return out

    MATH_FUNCS_EX = MATH_FUNCS + ("pow10_times_pow", "plain_div", "plain_rcp", "pow_df", "pow_fd")
    MATH_DECISIONS = {"limit_bracket": 32}       # KIDMP_MATH_LIMIT_BRACKET: not a function of fastmath.h, a code range of its own

    def math_probe_ex(self, fn, x, y=None, z=None, binary32=False):
        """math_probe on up to three operands, in binary64 or (binary32=True) through the float overloads, from a unit
        built with the column kernel's flags: "plain_div" / "plain_rcp" are the kernel's binary32 x / y and 1 / y.
        "pow10_times_pow": 10**x * y**z.  "pow_df" / "pow_fd": pow(double x, float y) / pow(float x, double y).
        "limit_bracket": a size-limit test decided by csrc/limit_bracket.h (b) and by the kernel's original expression (o)
        for x = num, y = den, z = site (0 ice, 1 rain, 2 .. 15 cloud droplets with nu = z), returned as b + 4 o + 16 i
        (i: lb::certainly_inside, what the kernel votes on).
        Operands that the device narrows to float must be binary32-representable."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(x if y is None else y, dtype=np.float64)
        z = np.ascontiguousarray(x if z is None else z, dtype=np.float64)
        if not (x.shape == y.shape == z.shape):
            raise ValueError("math_probe_ex: x, y and z must have one shape")
        narrowed = (x, y, z) if binary32 else {"pow_df": (y,), "pow_fd": (x,)}.get(fn, ())
        for a in narrowed:
            with np.errstate(over="ignore"):
                if not np.array_equal(a.astype(np.float32).astype(np.float64), a):
                    raise ValueError("math_probe_ex: an operand the device narrows to binary32 is not binary32-representable")
        out = np.empty_like(x)
        code = self.MATH_DECISIONS[fn] if fn in self.MATH_DECISIONS else self.MATH_FUNCS_EX.index(fn)
        self._check(load_library().kidmp_math_probe_ex(self._h, code, int(bool(binary32)), x.size,
                                                       _np_ptr(x), _np_ptr(y), _np_ptr(z), _np_ptr(out)))
        return out

    def table(self, name, shape=None):
        L = load_library()
        n = self._check(L.kidmp_get_table(self._h, name.encode(), None, 0))
        out = np.empty(n)
        self._check(L.kidmp_get_table(self._h, name.encode(), _np_ptr(out), n))
        return out.reshape(shape, order="F") if shape else out

    def const(self, name):
        L = load_library()
        n = self._check(L.kidmp_get_const(self._h, name.encode(), None, 0))
        out = np.empty(n)
        self._check(L.kidmp_get_const(self._h, name.encode(), _np_ptr(out), n))
        return out

    # ---- the reference's run_data/*.data table caches (M:3717-3829, M:3864-4078) ----
    def save_table_cache(self, directory):
        self._check(load_library().kidmp_save_table_cache(self._h, os.fsencode(directory)))

    def load_table_cache(self, directory):
        self._check(load_library().kidmp_load_table_cache(self._h, os.fsencode(directory)))

    def table_cache_reuse(self, directory, l_reuse, write_if_built=True):
        """thompson_init's use of run_data/*.data (M:3717-3729, M:3864-3895): read a file that exists when l_reuse,
        else write the GPU-built tables.  Returns the status bits (1, 2: racg, racs read; 4, 8: written)."""
        st = C.c_int32(0)
        self._check(load_library().kidmp_table_cache_reuse(self._h, os.fsencode(directory), int(bool(l_reuse)),
                                                           int(bool(write_if_built)), C.byref(st)))
        return st.value

    @staticmethod
    def kernel_name():
        return load_library().kidmp_kernel_name().decode()


def limbs_to_sums(limbs):
    """int64 [PPT_LIMBS] (host: numpy array or CPU tensor) -> the four precipitation domain sums (float64 numpy)."""
    a = np.ascontiguousarray(np.asarray(limbs, dtype=np.int64))
    if a.shape != (PPT_LIMBS,):
        raise KidmpError("limbs_to_sums: expected %d int64 limbs" % PPT_LIMBS)
    out = np.empty(4)
    load_library().kidmp_ppt_limbs_to_sums(a.ctypes.data_as(C.POINTER(C.c_int64)), _np_ptr(out))
    return out


def shard_bounds(ncol, nshard, shard):
    """The library's contiguous column ranges (kidmp_shard_bounds; no GPU needed)."""
    lo, hi = C.c_int64(), C.c_int64()
    rc = load_library().kidmp_shard_bounds(int(ncol), int(nshard), int(shard), C.byref(lo), C.byref(hi))
    if rc != 0:
        raise KidmpError("kidmp_shard_bounds failed (%d): %s" % (rc, load_library().kidmp_last_error(None).decode()))
    return lo.value, hi.value


class ThompsonMulti:
    """Several GPUs behind one host-array call (kidmp_init_multi / kidmp_batch_step_host_multi): contiguous column
    ranges over the device list, one pipeline per device on its own host thread, the precipitation domain sums
    all-reduced with RCCL inside the library.  This is what the Fortran drop-in uses when more than one device is
    configured; the Python mirror exists for the tests."""

    def __init__(self, devices, iiwarm=False, set_Nc=100.0, l_sediment=True, aerosol_aware=False):
        self._h = None
        L = load_library()
        cfg = _Cfg(int(bool(iiwarm)), int(bool(l_sediment)), float(set_Nc), 0, int(bool(aerosol_aware)))
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        h = _vp()
        rc = L.kidmp_init_multi(C.byref(cfg), len(devices), devs, C.byref(h))
        if rc != 0:
            raise KidmpError("kidmp_init_multi failed (%d): %s" % (rc, L.kidmp_last_error(None).decode()))
        self._h = h
        self.devices = [int(d) for d in devices]
        self.iiwarm = bool(iiwarm)

    def close(self):
        if getattr(self, "_h", None):
            load_library().kidmp_finalize_multi(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def batch_step_host(self, st, dt, ppt=None, want_rates=False, want_nstep=False, want_sanity=False):
        """numpy float64 [ncol, nz] arrays, in place (optional keys as ThompsonMP.batch_step_host).
        Returns (ppt, rates or None, nstep or None, precip_sums[4]) -- with want_sanity a fifth element, the 15-number
        sanity scan of the end state (kidmp_batch_step_host_multi_diag), reduced over the devices like the sums."""
        (ppt, rates, nstep), args = _host_step("batch_step_host", st, np.float64, dt, ppt, want_rates, want_nstep)
        sums = np.zeros(4)
        L = load_library()
        if want_sanity:
            sanity = np.zeros(15)
            rc = L.kidmp_batch_step_host_multi_diag(self._h, *args, _np_ptr(sums), _np_ptr(sanity))
        else:
            rc = L.kidmp_batch_step_host_multi(self._h, *args, _np_ptr(sums))
        if rc != 0:
            raise KidmpError("kidmp_batch_step_host_multi failed (%d): %s" % (rc, L.kidmp_multi_last_error(self._h).decode()))
        return (ppt, rates, nstep, sums, sanity) if want_sanity else (ppt, rates, nstep, sums)


# ---- module-level mirror of the Fortran module procedures ----
_module_ctx = None


def thompson_init(iiwarm=False, set_Nc=100.0, l_sediment=True, device=0):
    """thompson_init (M:374): builds the module-level context once, like the
    `micro_unset` guard of the KiD adapter (W:100-103)."""
    global _module_ctx
    if _module_ctx is None:
        _module_ctx = ThompsonMP(iiwarm=iiwarm, set_Nc=set_Nc, l_sediment=l_sediment, device=device)
    return _module_ctx


def mp_thompson(*args, **kw):
    """mp_thompson (M:1156) on the module-level context."""
    if _module_ctx is None:
        raise KidmpError("mp_thompson called before thompson_init")
    return _module_ctx.mp_thompson(*args, **kw)


def cache_write_file(path, tables):
    """Write `tables` (list of equally sized float64 arrays, Fortran element order) in the list-directed
    text format of the reference's `write(12,*) table` statements (M:3823-3828)."""
    arrs = [np.ascontiguousarray(np.asarray(t, dtype=np.float64).ravel(order="F")) for t in tables]
    n = arrs[0].size
    if any(a.size != n for a in arrs):
        raise KidmpError("cache_write_file: tables must have equal sizes")
    ptrs = (_dp * len(arrs))(*[_np_ptr(a) for a in arrs])
    rc = load_library().kidmp_cache_write_file(os.fsencode(path), len(arrs), ptrs, n)
    if rc != 0:
        raise KidmpError("cache_write_file failed (%d): %s" % (rc, load_library().kidmp_last_error(None).decode()))


def cache_read_file(path, ntab, n_each):
    """Read ntab tables of n_each values written by a Fortran `write(u,*)` (or by cache_write_file)."""
    arrs = [np.empty(n_each) for _ in range(ntab)]
    ptrs = (_dp * ntab)(*[_np_ptr(a) for a in arrs])
    rc = load_library().kidmp_cache_read_file(os.fsencode(path), ntab, ptrs, n_each)
    if rc != 0:
        raise KidmpError("cache_read_file failed (%d): %s" % (rc, load_library().kidmp_last_error(None).decode()))
    return arrs
