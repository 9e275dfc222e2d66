"""The kinematic half of a 1-D KiD case on the device (include/kidmp_kinematic.h): prescribed-w vertical advection of
KiD's nine fields in the adv / div form the adapter consumes, the state update that closes the time loop, and `run`, the
device-resident loop over both and kid_interface.  The advection scheme is the context's (kid_amd.advection): the project's
own van Leer scheme unless ULTIMATE QUICKEST (section 4.6g) was selected; neither is KiD's code.

The four entries of kidmp_kinematic.h are declared here, on the object load_library() returned, the first time one of them
is needed: include/kidmp.h and its mirror in thompson.py stay what they are.  There is no fallback: without the library or
the device a call raises KidmpError.
"""
import ctypes as C

from . import thompson as _th
from .thompson import KID_FIELDS, KidmpError, _KidFields

ADVECT_OUTPUTS = ("adv", "div", "sum")                     # the three optional kidmp_kid_fields outputs of kid_advect
_RUN_OPTIONS = ("rates", "nstep", "dbz", "radii", "arith")  # what run() passes on to kid_interface


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_kinematic.h."""
    i32, i64, vp, rc, f = C.c_int32, C.c_int64, C.c_void_p, C.c_int, C.POINTER(_KidFields)
    advect = [vp, i64, i32, C.c_double, f, vp, i64, vp, vp, f, f, f, vp, vp]
    return {
        "kidmp_kid_advect_device": (rc, advect),
        "kidmp32_kid_advect_device": (rc, advect),
        "kidmp_kid_update_device": (rc, [vp, i64, i32, C.c_double, f, f, f, f, i32, vp]),
        "kidmp32_kid_update_device": (rc, [vp, i64, i32, C.c_float, f, f, f, f, i32, vp]),
    }


def declare(L):
    """Declare the entries of kidmp_kinematic.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the kinematic entries declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _refuse(who, msg):
    raise KidmpError("%s: %s" % (who, msg))


def _number(who, name, x):
    try:
        x = float(x)
    except (TypeError, ValueError):
        _refuse(who, "%s must be a number" % name)
    if not x > 0.0:
        _refuse(who, "%s must be > 0" % name)
    return x


def _state(who, model, state):
    """(theta, ncol, nz, check) of a dict of KiD fields on the device; check(a, what[, shape]) judges one more tensor."""
    import torch
    q = state.get("theta") if isinstance(state, dict) else None
    if not isinstance(q, torch.Tensor):
        for k in KID_FIELDS if isinstance(state, dict) else ():      # update() may leave theta out
            if isinstance(state.get(k), torch.Tensor):
                q = state[k]
                break
    if not isinstance(q, torch.Tensor) or q.dtype not in (torch.float64, torch.float32) or q.dim() != 2 or not 2 <= q.shape[1] <= _th.MAX_NZ:
        _refuse(who, "state must be a dict of float64 or float32 CUDA tensors [ncol, nz] with keys from %s and nz in [2, %d]"
                % (", ".join(KID_FIELDS), _th.MAX_NZ))
    ncol, nz = int(q.shape[0]), int(q.shape[1])

    def check(a, what, shape=(ncol, nz)):
        if not isinstance(a, torch.Tensor):
            _refuse(who, "%s must be a torch tensor, got %s" % (what, type(a).__name__))
        model._want(a, q.dtype, shape, who + ": ", what)
    return q, ncol, nz, check


def _members(who, model, d, name, check, required=(), strict=True):
    """The present (key, tensor) of one dict of KiD fields; in an iiwarm context the frozen members are not looked at.
    strict: a key that is no KiD field is refused (else passed over: the result of kid_interface holds ppt, work ...)."""
    if not isinstance(d, dict):
        _refuse(who, "%s must be a dict with keys from %s" % (name, ", ".join(KID_FIELDS)))
    bad = [k for k in d if k not in KID_FIELDS]
    if bad and strict:
        _refuse(who, "%s has unknown members %s" % (name, bad))
    got = []
    for k in KID_FIELDS[:5] if model.iiwarm else KID_FIELDS:
        a = d.get(k)
        if a is None:
            if k in required:
                _refuse(who, "%s[%r] is required" % (name, k))
            continue
        check(a, "%s[%r]" % (name, k))
        got.append((k, a))
    return got


def _fields(members):
    d = dict(members)
    return _KidFields(*[d[k].data_ptr() if k in d else None for k in KID_FIELDS])


def _check(model, rc):
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, library().kidmp_last_error(model._h).decode()))


def _wanted(who, want):
    if isinstance(want, str):
        want = (want,)
    try:
        want = tuple(want)
    except TypeError:
        _refuse(who, "want must be a name or a sequence of names out of %s" % (ADVECT_OUTPUTS,))
    for n in want:
        if n not in ADVECT_OUTPUTS:
            _refuse(who, "unknown output %r: want must be out of %s" % (n, ADVECT_OUTPUTS))
    if len(set(want)) != len(want):
        _refuse(who, "want names an output twice")
    return want


def advect(model, state, w, rho, dz, dt, want=("sum",), courant=False, out=None, stream=None):
    """Vertical advection tendencies of a device-resident KiD state (kidmp[32]_kid_advect_device): one launch.

    state   dict name -> CUDA tensor [ncol, nz], all float64 or all float32 (widened on load), keys out of KID_FIELDS;
            theta, qv, qc, qr and nr are required, a missing (or None) member is not advected; never written
    w       face velocities in m/s, [nz+1] for all columns or [ncol, nz+1]: face f is the lower face of cell f
    rho, dz [nz] each, of the state's dtype; dt in s
    want    which of "adv" (flux form), "div" and "sum" (= adv + div, the advective form) to form; one that is not named
            costs no store
    courant True: the result also holds "courant" [ncol], the largest Courant number of each column's faces
    out     a dict returned by an earlier call with the same arguments, whose tensors are then written again (nothing is
            allocated: what a captured graph needs)
    Returns {"adv": {member: tensor}, ...} for the names in `want`.  Asynchronous on `stream` (default: torch's current
    stream)."""
    import torch
    who = "kid_advect"
    q, ncol, nz, check = _state(who, model, state)
    want = _wanted(who, want)
    if not want and not courant:
        _refuse(who, "nothing requested: want is empty and courant is False")
    dt = _number(who, "dt", dt)
    f_state = _members(who, model, state, "state", check, required=KID_FIELDS[:5])
    if not isinstance(w, torch.Tensor):
        _refuse(who, "w must be a torch tensor, got %s" % type(w).__name__)
    if tuple(w.shape) == (nz + 1,):
        stride = 0
    elif tuple(w.shape) == (ncol, nz + 1):
        stride = nz + 1
    else:
        _refuse(who, "w must be [nz+1] = [%d] or [ncol, nz+1] = [%d, %d], got %s" % (nz + 1, ncol, nz + 1, list(w.shape)))
    check(w, "w", tuple(w.shape))
    check(rho, "rho", (nz,))
    check(dz, "dz", (nz,))
    keys = [k for k, _ in f_state]
    if out is None:
        res = {n: {k: torch.empty_like(q) for k in keys} for n in want}
        if courant:
            res["courant"] = torch.empty(ncol, dtype=q.dtype, device=q.device)
    else:
        res = out
        if not isinstance(out, dict) or any(not isinstance(out.get(n), dict) for n in want) or (courant and out.get("courant") is None):
            _refuse(who, "out must be a dict returned by an earlier call with the same want and courant")
        for n in want:
            if sorted(out[n]) != sorted(keys):
                _refuse(who, "out[%r] must hold exactly the members %s" % (n, keys))
            for k in keys:
                check(out[n][k], "out[%r][%r]" % (n, k))
        if courant:
            check(out["courant"], "out['courant']", (ncol,))
    c_state = _fields(f_state)
    c_out = {n: _fields(res[n].items()) for n in want}
    L = library()
    fn = L.kidmp_kid_advect_device if q.dtype == torch.float64 else L.kidmp32_kid_advect_device
    _check(model, fn(model._h, ncol, nz, dt, C.byref(c_state), w.data_ptr(), stride, rho.data_ptr(), dz.data_ptr(),
                     *[C.byref(c_out[n]) if n in c_out else None for n in ADVECT_OUTPUTS],
                     res["courant"].data_ptr() if courant else None, _th._stream(stream, q)))
    return res


def update(model, state, dt, *tendencies, clip=True, stream=None):
    """state <- state + ((t1 + t2) + t3)*dt in place, in the tensors' own format (kidmp[32]_kid_update_device): one launch.

    state        dict name -> CUDA tensor [ncol, nz], keys out of KID_FIELDS; a missing (or None) member is left alone
    tendencies   up to three dicts of the same kind (the "sum" of advect, the result of kid_interface ...); a missing dict
                 or member is a zero operand; keys that are no KiD field (ppt, work ...) are not looked at
    clip         every member except theta then becomes max(X, +0.0)
    Returns `state`.  Asynchronous on `stream` (default: torch's current stream)."""
    import torch
    who = "kid_update"
    q, ncol, nz, check = _state(who, model, state)
    dt = _number(who, "dt", dt)
    if len(tendencies) > 3:
        _refuse(who, "at most three tendencies, got %d" % len(tendencies))
    f_state = _members(who, model, state, "state", check)
    if not f_state:
        _refuse(who, "nothing requested: state has no member")
    present = [k for k, _ in f_state]
    c_t = []
    for i, t in enumerate(tendencies):
        if t is not None and not isinstance(t, dict):
            _refuse(who, "tendency %d must be a dict with keys from %s" % (i + 1, ", ".join(KID_FIELDS)))
        c_t.append(None if t is None else _fields([m for m in _members(who, model, t, "tendency %d" % (i + 1), check, strict=False)
                                                   if m[0] in present]))
    c_t += [None] * (3 - len(c_t))
    c_state = _fields(f_state)
    L = library()
    fn = L.kidmp_kid_update_device if q.dtype == torch.float64 else L.kidmp32_kid_update_device
    _check(model, fn(model._h, ncol, nz, dt, C.byref(c_state), *[C.byref(t) if t is not None else None for t in c_t],
                     1 if clip else 0, _th._stream(stream, q)))
    return state


def run(model, state, nsteps, dt, p0, r_on_cp, exner, dz, rho, w, fix_theta=False, on_step=None, stream=None, **kid_interface_options):
    """A 1-D KiD case on the device: `nsteps` times advect(want="sum"), kid_interface(adv=sum), update(state, dt, sum,
    mphys), with no host round trip and no synchronisation.

    state       dict of KiD fields as for kid_interface, updated in place
    exner, dz   as for kid_interface ([ncol, nz], [nz]); rho [nz]
    w           [nz+1] or [ncol, nz+1] face velocities, or a callable step -> such a tensor (no history is kept)
    fix_theta   theta is left out of the update, as in KiD's 1-D cases
    on_step     called as on_step(step, state, result) after each update with the live state and kid_interface's result
                (whose tensors are written again by the next step)
    kid_interface_options   rates, nstep, dbz, radii, arith
    The adapter's workspace and every output tensor are allocated once, before the first step.  Returns (state, ppt,
    courant): ppt [ncol, 4] the sum over the steps of kid_interface's ppt, courant [ncol] of the last step."""
    import torch
    who = "kid_run"
    q, ncol, nz, _ = _state(who, model, state)
    bad = [k for k in kid_interface_options if k not in _RUN_OPTIONS]
    if bad:
        _refuse(who, "unknown options %s: kid_interface's %s may be passed on" % (bad, ", ".join(_RUN_OPTIONS)))
    if int(nsteps) != nsteps or nsteps < 0:
        _refuse(who, "nsteps must be a whole number >= 0")
    keys = KID_FIELDS[:5] if model.iiwarm else KID_FIELDS
    mphys = {k: torch.empty_like(q) for k in keys}
    mphys["ppt"] = torch.empty((ncol, 4), dtype=q.dtype, device=q.device)
    if kid_interface_options.get("dbz"):
        mphys["dbz"] = torch.empty_like(q)
    if kid_interface_options.get("radii"):
        mphys["radii"] = tuple(torch.empty_like(q) for _ in range(3))
    work = model.kid_workspace(ncol, nz, q.dtype)
    adv = {"sum": {k: torch.empty_like(q) for k in keys if state.get(k) is not None},
           "courant": torch.zeros(ncol, dtype=q.dtype, device=q.device)}
    ppt = torch.zeros((ncol, 4), dtype=q.dtype, device=q.device)
    moved = {k: v for k, v in state.items() if not (fix_theta and k == "theta")}
    ctx = torch.cuda.stream(torch.cuda.ExternalStream(stream, device=q.device)) if stream is not None else None
    if ctx is not None:
        ctx.__enter__()
    try:
        for step in range(int(nsteps)):
            adv = advect(model, state, w(step) if callable(w) else w, rho, dz, dt, "sum", True, adv, stream)
            mphys = model.kid_interface(state, dt, p0, r_on_cp, exner, dz, adv=adv["sum"], work=work, out=mphys, stream=stream,
                                        **kid_interface_options)
            update(model, moved, dt, adv["sum"], mphys, stream=stream)
            ppt += mphys["ppt"]
            if on_step is not None:
                on_step(step, state, mphys)
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    return state, ppt, adv["courant"]
