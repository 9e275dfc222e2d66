"""Prognostic aerosols in the KiD path (include/kidmp_aerosol.h): the droplet number nc and the aerosol numbers nwfa and
nifa carried through the adapter, both advection entries and the update on the device, for a context made with
aerosol_aware=True, and `run_aero` / `run_slab_aero`, the device-resident loops over them.

State, forcing and result dicts carry twelve members, KID_FIELDS + AEROSOL_FIELDS; the wrappers split them into the
nine-member calls of kid_amd.kinematic / kid_amd.slab and the three-member entries declared here.  The cell-centre updraft
the step wants (w1d, M:2797) is formed from the face velocities as 0.5*(w[k] + w[k+1]): the project's convention, KiD's own
is not part of the reference.

Only the ten entries of kidmp_aerosol.h are declared here, on the object load_library() returned, the first time one of
them is needed.  There is no fallback: without the library or the device a call raises KidmpError.
"""
import ctypes as C

from . import kinematic as _kk
from . import slab as _ks
from . import thompson as _th
from .thompson import KID_FIELDS, NRATES, KidmpError, _KidFields, _Outputs  # noqa: F401

AEROSOL_FIELDS = ("nc", "nwfa", "nifa")                    # members of kidmp_kid_aerosols: workspace profiles 8, 9, 10
ALL_FIELDS = KID_FIELDS + AEROSOL_FIELDS
ADVECT_OUTPUTS = _kk.ADVECT_OUTPUTS


class _KidAerosols(C.Structure):
    """kidmp_kid_aerosols / kidmp32_kid_aerosols (include/kidmp_aerosol.h): three pointers, null = absent."""
    _fields_ = [(k, C.c_void_p) for k in AEROSOL_FIELDS]


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_aerosol.h."""
    i32, i64, vp, rc, size, d = C.c_int32, C.c_int64, C.c_void_p, C.c_int, C.c_size_t, C.c_double
    f, a, o = C.POINTER(_KidFields), C.POINTER(_KidAerosols), C.POINTER(_Outputs)
    out = {}
    for pre, real, arith in (("kidmp", d, []), ("kidmp32", C.c_float, [i32])):
        head = [vp, i64, i32, real, real, real, f, f, f, vp, vp]
        out.update({
            pre + "_kid_interface_aero_device": (rc, head + [f, vp, vp, vp, o] + arith + [a, a, a, a, vp, i64, vp, vp, size, vp]),
            pre + "_kid_gather_aero_device": (rc, head + [vp, a, a, a, vp, i64, vp, size, vp]),
            pre + "_kid_advect_aero_device": (rc, [vp, i64, i32, d, a, vp, i64, vp, vp, a, a, a, vp]),
            pre + "_kid_advect_slab_aero_device": (rc, [vp, i64, i32, i32, d, d, a, vp, vp, i32, vp, vp, a, a, a, vp]),
            pre + "_kid_update_aero_device": (rc, [vp, i64, i32, real, a, a, a, a, i32, vp]),
        })
    return out


def declare(L):
    """Declare the entries of kidmp_aerosol.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the aerosol entries declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


# ---- what the wrappers share ----
def _split(who, d, name):
    """(the KiD members, the aerosol members) of a twelve-member dict; None gives (None, {})."""
    if d is None:
        return None, {}
    if not isinstance(d, dict):
        _kk._refuse(who, "%s must be a dict with keys from %s" % (name, ", ".join(ALL_FIELDS)))
    bad = [k for k in d if k not in ALL_FIELDS]
    if bad:
        _kk._refuse(who, "%s has unknown members %s" % (name, bad))
    return {k: d[k] for k in KID_FIELDS if k in d}, {k: d[k] for k in AEROSOL_FIELDS if d.get(k) is not None}


def _aer_state(who, model, state):
    """(a tensor, ncol, nz, check, the present aerosol members) of a dict that holds aerosol members (the KiD members of a
    twelve-member dict are passed over)."""
    import torch
    _, aer = _split(who, state, "state")
    q = next((a for a in aer.values() if isinstance(a, torch.Tensor)), None)
    if q is None:
        _kk._refuse(who, "state must be a dict of float64 or float32 CUDA tensors [ncol, nz] with members out of %s"
                    % ", ".join(AEROSOL_FIELDS))
    q, ncol, nz, check = _kk._state(who, model, {"theta": q})
    return q, ncol, nz, check, aer


def _check_members(aer, check, name="state"):
    for k, a in aer.items():
        check(a, "%s[%r]" % (name, k))


def _aerosols(members):
    return _KidAerosols(*[members[k].data_ptr() if k in members else None for k in AEROSOL_FIELDS])


def _aer_outputs(who, q, keys, want, out, check):
    """The output dicts of an advection call: made, or those of `out` (which may hold other members too)."""
    import torch
    if out is None:
        return {n: {k: torch.empty_like(q) for k in keys} for n in want}
    if not isinstance(out, dict) or any(not isinstance(out.get(n), dict) for n in want):
        _kk._refuse(who, "out must be a dict returned by an earlier call with the same want")
    for n in want:
        for k in keys:
            if out[n].get(k) is None:
                _kk._refuse(who, "out[%r] must hold the members %s" % (n, list(keys)))
            check(out[n][k], "out[%r][%r]" % (n, k))
    return out


def _byref(c_out, n):
    return C.byref(c_out[n]) if n in c_out else None


def _face_w(who, w, ncol, nz):
    """The column stride of the face velocities w, [nz+1] or [ncol, nz+1], from its shape."""
    import torch
    if not isinstance(w, torch.Tensor):
        _kk._refuse(who, "w must be a torch tensor, got %s" % type(w).__name__)
    if tuple(w.shape) == (nz + 1,):
        stride = 0
    elif tuple(w.shape) == (ncol, nz + 1):
        stride = nz + 1
    else:
        _kk._refuse(who, "w must hold the face velocities, [nz+1] = [%d] or [ncol, nz+1] = [%d, %d], got %s"
                    % (nz + 1, ncol, nz + 1, list(w.shape)))
    return stride


def _source(who, nwfa_source, ncol):
    import torch
    if nwfa_source is not None and (not isinstance(nwfa_source, torch.Tensor) or tuple(nwfa_source.shape) != (ncol,)):
        _kk._refuse(who, "nwfa_source must be a tensor [ncol] = [%d]" % ncol)


def _require_aerosols(who, aer):
    for k in AEROSOL_FIELDS:
        if k not in aer:
            _kk._refuse(who, "state[%r] is required" % k)


# ---- the five entries ----
def advect_aero(model, state, w, rho, dz, dt, want=("sum",), out=None, stream=None):
    """Vertical advection tendencies of the aerosols (kidmp[32]_kid_advect_aero_device): one launch, the operations of
    kinematic.advect member for member.

    state   dict with members out of AEROSOL_FIELDS (CUDA tensors [ncol, nz], float64 or float32); a missing member is not
            advected; the KiD members of a twelve-member dict are passed over
    w       FACE velocities, [nz+1] or [ncol, nz+1], as for kinematic.advect; rho, dz [nz]; dt in s
    want, out, stream   as for kinematic.advect; there is no courant: the nine-field call reports it
    Returns {"sum": {member: tensor}, ...} for the names in `want`."""
    import torch
    who = "kid_advect_aero"
    q, ncol, nz, check, aer = _aer_state(who, model, state)
    want = _kk._wanted(who, want)
    if not want:
        _kk._refuse(who, "nothing requested: want is empty")
    dt = _kk._number(who, "dt", dt)
    stride = _face_w(who, w, ncol, nz)
    _check_members(aer, check)
    check(w, "w", tuple(w.shape))
    check(rho, "rho", (nz,))
    check(dz, "dz", (nz,))
    res = _aer_outputs(who, q, list(aer), want, out, check)
    c_out = {n: _aerosols({k: res[n][k] for k in aer}) for n in want}
    L = library()
    fn = L.kidmp_kid_advect_aero_device if q.dtype == torch.float64 else L.kidmp32_kid_advect_aero_device
    _kk._check(model, fn(model._h, ncol, nz, dt, C.byref(_aerosols(aer)), w.data_ptr(), stride, rho.data_ptr(), dz.data_ptr(),
                         *[_byref(c_out, n) for n in ADVECT_OUTPUTS], _th._stream(stream, q)))
    return res


def advect_slab_aero(model, state, u, w, rho, dz, dx, dt, nx, want=("sum",), out=None, stream=None):
    """x-z advection tendencies of the aerosols on periodic slabs (kidmp[32]_kid_advect_slab_aero_device): one launch, the
    operations of slab.advect_slab member for member.  state, want, out as for advect_aero; u, w, rho, dz, dx, dt, nx as
    for slab.advect_slab."""
    import torch
    who = "kid_advect_slab_aero"
    q, ncol, nz, check, aer = _aer_state(who, model, state)
    nslab = _ks._slab_shape(who, ncol, nx)
    want = _kk._wanted(who, want)
    if not want:
        _kk._refuse(who, "nothing requested: want is empty")
    dt = _kk._number(who, "dt", dt)
    dx = _kk._number(who, "dx", dx)
    shared = _ks._flow(who, u, w, ncol, nx, nz)
    _check_members(aer, check)
    check(u, "u", tuple(u.shape))
    check(w, "w", tuple(w.shape))
    check(rho, "rho", (nz,))
    check(dz, "dz", (nz,))
    res = _aer_outputs(who, q, list(aer), want, out, check)
    c_out = {n: _aerosols({k: res[n][k] for k in aer}) for n in want}
    L = library()
    fn = L.kidmp_kid_advect_slab_aero_device if q.dtype == torch.float64 else L.kidmp32_kid_advect_slab_aero_device
    _kk._check(model, fn(model._h, nslab, nx, nz, dt, dx, C.byref(_aerosols(aer)), u.data_ptr(), w.data_ptr(), shared, rho.data_ptr(),
                         dz.data_ptr(), *[_byref(c_out, n) for n in ADVECT_OUTPUTS], _th._stream(stream, q)))
    return res


def update_aero(model, state, dt, *tendencies, clip=True, stream=None):
    """nc, nwfa, nifa <- A + ((t1 + t2) + t3)*dt in place (kidmp[32]_kid_update_aero_device): one launch.  state and up to
    three tendencies as for kinematic.update, with members out of AEROSOL_FIELDS (other keys are passed over); clip: every
    member then becomes max(A, +0.0).  Returns `state`."""
    import torch
    who = "kid_update_aero"
    q, ncol, nz, check, aer = _aer_state(who, model, state)
    dt = _kk._number(who, "dt", dt)
    if len(tendencies) > 3:
        _kk._refuse(who, "at most three tendencies, got %d" % len(tendencies))
    for i, t in enumerate(tendencies):
        if t is not None and not isinstance(t, dict):
            _kk._refuse(who, "tendency %d must be a dict with keys from %s" % (i + 1, ", ".join(AEROSOL_FIELDS)))
    _check_members(aer, check)
    c_t = []
    for i, t in enumerate(tendencies):
        got = {} if t is None else {k: t[k] for k in aer if t.get(k) is not None}
        for k, a in got.items():
            check(a, "tendency %d[%r]" % (i + 1, k))
        c_t.append(_aerosols(got) if t is not None else None)
    c_t += [None] * (3 - len(c_t))
    L = library()
    fn = L.kidmp_kid_update_aero_device if q.dtype == torch.float64 else L.kidmp32_kid_update_aero_device
    _kk._check(model, fn(model._h, ncol, nz, dt, C.byref(_aerosols(aer)), *[C.byref(t) if t is not None else None for t in c_t],
                         1 if clip else 0, _th._stream(stream, q)))
    return state


def kid_interface_aero(model, state, dt, p0, r_on_cp, exner, dz, adv=None, div=None, w=None, nwfa_source=None, work=None,
                       rates=None, nstep=None, dbz=False, radii=False, arith=None, stream=None, out=None, gather_only=False):
    """The KiD adapter with prognostic aerosols (kidmp[32]_kid_interface_aero_device), for an aerosol-aware context.

    state       dict of the twelve members KID_FIELDS + AEROSOL_FIELDS (the frozen ones only in a mixed-phase context),
                float64 or float32 CUDA tensors [ncol, nz]; nc, nwfa and nifa are required
    adv, div    dicts of the same kind; a missing dict or member is a zero operand
    w           the CELL-CENTRE updraft in m/s, [nz] for all columns or [ncol, nz]; None: zeros
    nwfa_source [ncol], per kg per second: added to the lowest level's nwfa after the step (M:1001)
    the rest    as for ThompsonMP.kid_interface, except that float32 fields step in arith "p32n" only ("f32" is refused)
    Returns a dict: the twelve tendencies, "ppt", "dbz" / "radii" when wanted, and "work".  gather_only
    (kidmp[32]_kid_gather_aero_device): returns {"ppt", "work"}."""
    import torch
    who = "kid_interface_aero"
    if not getattr(model, "aerosol_aware", False):
        _kk._refuse(who, "the context is not aerosol-aware (ThompsonMP(aerosol_aware=True)); kid_interface serves it")
    nine, aer = _split(who, state, "state")
    q, ncol, nz, check = _kk._state(who, model, nine)
    is64 = q.dtype == torch.float64
    if is64 and arith is not None:
        _kk._refuse(who, "arith applies to float32 fields only")
    if not is64 and (arith or "p32n") != "p32n":
        _kk._refuse(who, "float32 fields step in arith 'p32n' only with prognostic aerosols, got %r" % (arith,))
    dt = _kk._number(who, "dt", dt)
    keys = KID_FIELDS[:5] if model.iiwarm else KID_FIELDS
    _require_aerosols(who, aer)
    split = [(name,) + _split(who, d, name) for name, d in (("adv", adv), ("div", div))]
    stride = 0
    if w is not None:
        if not isinstance(w, torch.Tensor):
            _kk._refuse(who, "w must be a torch tensor, got %s" % type(w).__name__)
        if tuple(w.shape) == (ncol, nz):
            stride = nz
        elif tuple(w.shape) != (nz,):
            _kk._refuse(who, "w must hold the cell-centre updraft, [nz] = [%d] or [ncol, nz] = [%d, %d], got %s (the nz+1 face "
                             "velocities belong to advect_aero)" % (nz, ncol, nz, list(w.shape)))
    _source(who, nwfa_source, ncol)
    f_state = _kk._members(who, model, nine, "state", check, required=keys)
    _check_members(aer, check)
    forcing = []
    for name, f9, f3 in split:
        _check_members(f3, check, name)
        forcing.append((None if f9 is None else _kk._fields(_kk._members(who, model, f9, name, check)), None if f9 is None else _aerosols(f3)))
    check(exner, "exner")
    check(dz, "dz", (nz,))
    if w is not None:
        check(w, "w", tuple(w.shape))
    if nwfa_source is not None:
        check(nwfa_source, "nwfa_source", (ncol,))
    if rates is not None:
        model._want(rates, torch.float64, (ncol, NRATES, nz), who + ": rates")
    if nstep is not None:
        model._want(nstep, torch.int32, (ncol, 4), who + ": nstep")
    need = 15 * ((ncol * nz * q.element_size() + 255) // 256 * 256)
    if work is not None and not (isinstance(work, torch.Tensor) and work.is_cuda and work.dtype == torch.uint8 and work.dim() == 1
                                 and work.is_contiguous() and work.device.index == model.device and work.numel() >= need
                                 and work.data_ptr() % 16 == 0):
        _kk._refuse(who, "work must be a contiguous uint8 CUDA tensor of at least %d bytes on cuda:%d (kid_workspace)" % (need, model.device))
    members = list(keys) + list(AEROSOL_FIELDS)
    if out is not None:
        if not isinstance(out, dict) or out.get("ppt") is None or (dbz and out.get("dbz") is None) or (radii and out.get("radii") is None):
            _kk._refuse(who, "out must be a dict holding ppt (and dbz / radii when they are wanted)")
        for k in ([] if gather_only else members):
            if out.get(k) is None:
                _kk._refuse(who, "out[%r] is required" % k)
            check(out[k], "out[%r]" % k)
        res = out
    else:
        res = {k: torch.empty_like(q) for k in ([] if gather_only else members)}
        res["ppt"] = torch.empty((ncol, 4), dtype=q.dtype, device=q.device)
        if dbz:
            res["dbz"] = torch.empty_like(q)
        if radii:
            res["radii"] = tuple(torch.empty_like(q) for _ in range(3))
    check(res["ppt"], "out['ppt']", (ncol, 4))
    if dbz:
        check(res["dbz"], "out['dbz']")
    if radii:
        for a in res["radii"]:
            check(a, "out['radii']")
    res["work"] = work if work is not None else model.kid_workspace(ncol, nz, q.dtype)
    work = res["work"]
    ref = lambda x: None if x is None else C.byref(x)   # noqa: E731
    ptr = lambda x: None if x is None else x.data_ptr()   # noqa: E731
    head = [model._h, ncol, nz, dt, float(p0), float(r_on_cp), C.byref(_kk._fields(f_state)), ref(forcing[0][0]), ref(forcing[1][0]),
            exner.data_ptr(), dz.data_ptr()]
    tail = [ptr(w), stride]
    s = _th._stream(stream, q)
    L = library()
    if gather_only:
        fn = L.kidmp_kid_gather_aero_device if is64 else L.kidmp32_kid_gather_aero_device
        _kk._check(model, fn(*head, res["ppt"].data_ptr(), C.byref(_aerosols(aer)), ref(forcing[0][1]), ref(forcing[1][1]), *tail,
                             work.data_ptr(), work.numel(), s))
        return {"ppt": res["ppt"], "work": work}
    o = _th._outputs(res["dbz"] if dbz else None, res["radii"] if radii else None, torch.Tensor.data_ptr)
    fn = L.kidmp_kid_interface_aero_device if is64 else L.kidmp32_kid_interface_aero_device
    _kk._check(model, fn(*head, C.byref(_kk._fields([(k, res[k]) for k in keys])), res["ppt"].data_ptr(), ptr(rates), ptr(nstep),
                         C.byref(o) if (dbz or radii) else None, *([] if is64 else [model.ARITH[arith or "p32n"]]),
                         C.byref(_aerosols(aer)), ref(forcing[0][1]), ref(forcing[1][1]), C.byref(_aerosols({k: res[k] for k in AEROSOL_FIELDS})),
                         *tail, ptr(nwfa_source), work.data_ptr(), work.numel(), s))
    return res


# ---- the device-resident runs ----
def _run(who, model, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, w, nwfa_source, fix_theta, on_step, stream, options, slab=None):
    """What run_aero and run_slab_aero share; slab = (dx, nx, u) or None."""
    import torch
    if not getattr(model, "aerosol_aware", False):
        _kk._refuse(who, "the context is not aerosol-aware (ThompsonMP(aerosol_aware=True)); kid_run serves it")
    nine, aer = _split(who, state, "state")
    q, ncol, nz, check = _kk._state(who, model, nine)
    _kk._number(who, "dt", dt)
    if slab is not None:
        dx, nx, u = slab
        nslab = _ks._slab_shape(who, ncol, nx)
        _kk._number(who, "dx", dx)
        if not callable(u) and not callable(w):
            _ks._flow(who, u, w, ncol, nx, nz)
    elif not callable(w):
        _face_w(who, w, ncol, nz)
    keys = KID_FIELDS[:5] if model.iiwarm else KID_FIELDS
    _require_aerosols(who, aer)
    _source(who, nwfa_source, ncol)
    _kk._members(who, model, nine, "state", check, required=KID_FIELDS[:5])
    _check_members(aer, check)
    for name, a, shape in (("exner", exner, (ncol, nz)), ("dz", dz, (nz,)), ("rho", rho, (nz,))):
        check(a, name, shape)
    if nwfa_source is not None:
        check(nwfa_source, "nwfa_source", (ncol,))
    bad = [k for k in options if k not in _kk._RUN_OPTIONS]
    if bad:
        _kk._refuse(who, "unknown options %s: kid_interface_aero's %s may be passed on" % (bad, ", ".join(_kk._RUN_OPTIONS)))
    if int(nsteps) != nsteps or nsteps < 0:
        _kk._refuse(who, "nsteps must be a whole number >= 0")
    mphys = {k: torch.empty_like(q) for k in keys + AEROSOL_FIELDS}
    mphys["ppt"] = torch.empty((ncol, 4), dtype=q.dtype, device=q.device)
    if options.get("dbz"):
        mphys["dbz"] = torch.empty_like(q)
    if options.get("radii"):
        mphys["radii"] = tuple(torch.empty_like(q) for _ in range(3))
    work = model.kid_workspace(ncol, nz, q.dtype)
    nine = {k: v for k, v in nine.items() if k in keys and v is not None}
    adv9 = {"sum": {k: torch.empty_like(q) for k in nine}, "courant": torch.zeros(ncol, dtype=q.dtype, device=q.device)}
    adv3 = {"sum": {k: torch.empty_like(q) for k in aer}}
    both = dict(adv9["sum"], **adv3["sum"])
    wc = torch.empty_like(q)                                   # the cell-centre updraft, [ncol, nz]
    ppt = torch.zeros((ncol, 4), dtype=q.dtype, device=q.device)
    moved = {k: v for k, v in nine.items() if not (fix_theta and k == "theta")}
    ctx = torch.cuda.stream(torch.cuda.ExternalStream(stream, device=q.device)) if stream is not None else None
    if ctx is not None:
        ctx.__enter__()
    try:
        for step in range(int(nsteps)):
            wf = w(step) if callable(w) else w
            if slab is None:
                adv9 = _kk.advect(model, nine, wf, rho, dz, dt, "sum", True, adv9, stream)
                adv3 = advect_aero(model, aer, wf, rho, dz, dt, "sum", adv3, stream)
            else:
                uf = u(step) if callable(u) else u
                adv9 = _ks.advect_slab(model, nine, uf, wf, rho, dz, dx, dt, nx, "sum", True, adv9, stream)
                adv3 = advect_slab_aero(model, aer, uf, wf, rho, dz, dx, dt, nx, "sum", adv3, stream)
            centre_updraft(wf, out=wc if slab is None else wc.view(nslab, nx, nz))
            mphys = kid_interface_aero(model, state, dt, p0, r_on_cp, exner, dz, adv=both, w=wc, nwfa_source=nwfa_source, work=work,
                                       out=mphys, stream=stream, **options)
            _kk.update(model, moved, dt, adv9["sum"], mphys, stream=stream)
            update_aero(model, aer, dt, adv3["sum"], mphys, stream=stream)
            ppt += mphys["ppt"]
            if on_step is not None:
                on_step(step, state, mphys)
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return state, ppt, adv9["courant"]


def centre_updraft(w, out=None):
    """The cell-centre updraft 0.5*(w[..., :-1] + w[..., 1:]) of face velocities, in the tensor's dtype (the project's
    convention); `out` may be a broadcast of the result (one profile for every column, one flow for every slab)."""
    c = 0.5 * (w[..., :-1] + w[..., 1:])
    if out is None:
        return c
    out.copy_(c.reshape(out.shape) if c.numel() == out.numel() else c.expand_as(out))
    return out


def run_aero(model, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, w, nwfa_source=None, fix_theta=False, on_step=None, stream=None,
             **kid_interface_options):
    """A 1-D KiD case with prognostic aerosols on the device: `nsteps` times advect and advect_aero (want="sum"), the
    cell-centre updraft 0.5*(w[k] + w[k+1]), kid_interface_aero(adv=sum, w=centre, nwfa_source), update and update_aero, with
    no host round trip and no synchronisation.  state holds the twelve members and is updated in place; everything else as
    for kinematic.run.  Returns (state, ppt, courant)."""
    return _run("kid_run_aero", model, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, w, nwfa_source, fix_theta, on_step, stream,
                kid_interface_options)


def run_slab_aero(model, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, dx, nx, u, w, nwfa_source=None, fix_theta=False, on_step=None,
                  stream=None, **kid_interface_options):
    """An x-z KiD case with prognostic aerosols on the device: run_aero with advect_slab and advect_slab_aero in the place
    of advect and advect_aero; dx, nx, u, w as for slab.run_slab.  Returns (state, ppt, courant)."""
    return _run("kid_run_slab_aero", model, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, w, nwfa_source, fix_theta, on_step, stream,
                kid_interface_options, slab=(dx, nx, u))
