"""The aerosol half of the KiD adapter (include/kidmp_aerosol.h) restated in numpy: the gather of nc, nwfa, nifa and the
updraft, the surface source and the back-out, every operation rounded once in the arrays' own format (binary64 or
binary32).  No GPU code and no test."""
import numpy as np

AEROSOLS = ("nc", "nwfa", "nifa")


def _operand(d, k, like):
    return np.zeros_like(like) if d is None or d.get(k) is None else d[k]


def gather(aer, adv, div, w, dt):
    """Workspace profiles 8, 9, 10 and 13: A1 = A + (dA_adv + dA_div)*dt (the expression of W:60-93) and the updraft, a
    [nz] profile broadcast over the columns, a [ncol, nz] array copied, None zeros.  A missing forcing is a zero operand."""
    T = aer["nc"].dtype.type
    out = {}
    for k in AEROSOLS:
        out[k] = aer[k] + (_operand(adv, k, aer[k]) + _operand(div, k, aer[k])) * T(dt)
        assert out[k].dtype == aer[k].dtype
    out["w"] = np.zeros_like(aer["nc"]) if w is None else np.ascontiguousarray(np.broadcast_to(w, aer["nc"].shape))
    return out


def source(nwfa1, src, dt):
    """M:1001 on the post-step nwfa: level 0 of every column gains src*dt."""
    T = nwfa1.dtype.type
    out = nwfa1.copy()
    if src is not None:
        out[:, 0] = nwfa1[:, 0] + src * T(dt)
    assert out.dtype == nwfa1.dtype
    return out


def backout(aer, adv, div, post, dt):
    """dA_mphys = (A1 - A)/dt - (dA_adv + dA_div) from the post-step profiles `post` (nwfa after the source)."""
    T = aer["nc"].dtype.type
    return {k: (post[k] - aer[k]) / T(dt) - (_operand(adv, k, aer[k]) + _operand(div, k, aer[k])) for k in AEROSOLS}
