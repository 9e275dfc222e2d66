"""The advection scheme of the KiD path (include/kidmp_advection.h): a setting of the context that the eight advection
entries -- kinematic.advect, slab.advect_slab, aerosol.advect_aero, aerosol.advect_slab_aero in both precisions, and with
them run, run_slab, run_aero and run_slab_aero -- read when they are called.  "vanleer" is the scheme of a new context
(DESIGN.md section 4.6c); "ultimate" is Leonard's ULTIMATE QUICKEST (section 4.6g): the published algorithm, not KiD's code.

The two entries of kidmp_advection.h are declared here, on the object load_library() returned, the first time one of them
is needed: include/kidmp.h and its mirror in thompson.py stay what they are.  An unknown name is refused before the library
is reached.
"""
import ctypes as C

from . import thompson as _th
from .thompson import KidmpError

SCHEMES = ("vanleer", "ultimate")                          # KIDMP_ADVECT_VANLEER = 0, KIDMP_ADVECT_ULTIMATE = 1


def _declarations():
    """name -> (restype, argtypes) of every entry of include/kidmp_advection.h."""
    return {"kidmp_set_advection": (C.c_int, [C.c_void_p, C.c_int32]), "kidmp_advection": (C.c_int, [C.c_void_p])}


def declare(L):
    """Declare the entries of kidmp_advection.h on the loaded library `L`."""
    for name, (restype, argtypes) in _declarations().items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, argtypes
    return L


_declared = None


def library():
    """The library of load_library() with the entries of kidmp_advection.h declared."""
    global _declared
    L = _th.load_library()
    if _declared is not L:
        declare(L)
        _declared = L
    return L


def _check(model, L, rc):
    if rc < 0:
        raise KidmpError("kidmp error %d: %s" % (rc, L.kidmp_last_error(model._h).decode()))
    return rc


def set_scheme(model, name):
    """Select the scheme of every later advection call on `model`: a name out of SCHEMES.  Returns the name."""
    if not isinstance(name, str) or name not in SCHEMES:
        raise KidmpError("set_advection: unknown scheme %r: it must be one of %s" % (name, ", ".join(SCHEMES)))
    L = library()
    _check(model, L, L.kidmp_set_advection(model._h, SCHEMES.index(name)))
    return name


def scheme(model):
    """The name of the scheme `model` advects with."""
    L = library()
    return SCHEMES[_check(model, L, L.kidmp_advection(model._h))]
