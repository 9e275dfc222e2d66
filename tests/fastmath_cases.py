"""Deterministic edge cases for kid_amd/csrc/fastmath.h, shared by test_fastmath_edges.py (host build) and
test_gpu_fastmath_edges.py (device).  Nothing here is random except a seeded filler over the ranges of
tests/native/fastmath_check.cpp.  Every construction aims at a place where a table-driven reduction can go wrong:

  ln table     the 65 bin edges of the 64-entry table (high dword LOG_OFFHI + (i << LOG_SHIFT), low dword 0; the constants
               are parsed out of fastmath_tables.h) and their +-1, 2, 3 ulp neighbours, scaled by 2**k, k = -148 .. 84
  near 1       1 +- d ulps, d = 0 .. 2000 (the relative error of ln is asked there)
  powers of 2  pow(2**k, y), integral y: exact
  exp, exp10   (n + h/2) ln2/64 resp. log10(2)/64, h in {0, 1}, and +-1, 2 ulps: where the table index and the binary
               exponent change (h = 0 sits on an index, h = 1 on the rint tie between two)
  pow          the ln-table points (every fourth k, the ends and -1, 0, 1, 5) crossed with the exponents POW_Y
  pow10_times_pow  a grid over the ranges of fastmath_check.cpp, and rows where la*log2(10) and y*log2(x) cancel to
               within 1 and to within 2**-20 of a whole or half number of 64ths
  roots        mantissas 1, 1+ulp, 2-ulp at every exponent of the domain, perfect squares and cubes, the ends of the domain
  division     denominators of mantissa 1, 1+ulp, 2-ulp, neighbours of reciprocals, powers of two, a == b, quotients one
               ulp either side of 1 and 2

cases64() / cases32() return {name: (x, y, z)} of binary64 arrays (for cases32 every value is binary32-representable);
the part of a name before "@" is the function (fn_of; codes in FN).  An operand a function does not read is 1.0.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
f32 = np.float32

# the codes of include/kidmp.h in the order of ThompsonMP.MATH_FUNCS_EX
FN = ("log", "log10", "exp", "exp10", "sqrt", "cbrt", "pow", "rcp_seed", "div", "ieee_div", "rcp", "pow10_times_pow", "plain_div",
      "plain_rcp", "pow_df", "pow_fd")
POW_Y = (-4.2, -3.0, -1.0, -1.0 / 3.0, 0.0, 1e-3, 0.5, 1.0, 2.0, 2.5, 3.5, 4.2)
FLT_MIN, FLT_MAX = float(np.finfo(f32).tiny), float(np.finfo(f32).max)
LOG2_10, LOG2_E = np.log2(LD(10)), LD(1) / np.log(LD(2))


def table_constants():
    """LOG_OFFHI, LOG_N, LOG_SHIFT as fastmath_tables.h states them."""
    text = open(os.path.join(ROOT, "kid_amd", "csrc", "fastmath_tables.h")).read()
    off = int(re.search(r"LOG_OFFHI\s*=\s*(0x[0-9A-Fa-f]+)u", text).group(1), 16)
    n = int(re.search(r"\bLOG_N\s*=\s*(\d+)", text).group(1))
    shift = int(re.search(r"\bLOG_SHIFT\s*=\s*(\d+)", text).group(1))
    return off, n, shift


def _step64(x, d):
    """x moved by d ulps (positive normal binary64, integer arithmetic on the bits)."""
    x, d = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(d, dtype=np.int64))
    return (np.ascontiguousarray(x).view(np.int64) + d).view(np.float64)


def _step32(x, d):
    x, d = np.broadcast_arrays(np.asarray(x, dtype=f32), np.asarray(d, dtype=np.int32))
    return (np.ascontiguousarray(x).view(np.int32) + d).view(f32)


def _cross(a, b):
    """every element of a with every element of b, flattened"""
    A, B = np.meshgrid(np.asarray(a), np.asarray(b), indexing="ij")
    return A.ravel(), B.ravel()


def _ones(x):
    return np.ones_like(x)


def _filler(lo, hi, n, seed):
    """the seeded filler: 10**U(lo, hi) * (1 + U(0, 1)), as fastmath_check.cpp draws its arguments"""
    rng = np.random.default_rng(seed)
    return 10.0 ** rng.uniform(lo, hi, n) * (1.0 + rng.uniform(0, 1, n))


# ---------------------------------------------------------------- binary64
def ln_table_points(ks=range(-148, 85)):
    off, n, shift = table_constants()
    hi = (off + (np.arange(n + 1, dtype=np.int64) << shift)) << 32          # low dword 0
    edges = hi.view(np.float64)
    pts = _step64(edges[:, None], np.arange(-3, 4)[None, :]).ravel()
    return (pts[:, None] * 2.0 ** np.asarray(list(ks), dtype=np.float64)[None, :]).ravel()      # exact scaling


def near_one64():
    return np.concatenate([_step64(1.0, np.arange(0, 2001)), _step64(1.0, -np.arange(1, 2001))])


def _ties64(step_ld, lo, hi):
    """fl((n + h/2) * step), h in {0, 1}, for every integer n that keeps the argument in [lo, hi], and +-1, 2 ulps"""
    n = np.arange(int(np.ceil(LD(lo) / step_ld)), int(np.floor(LD(hi) / step_ld)) + 1).astype(LD)
    base = np.concatenate([(n * step_ld), ((n + LD(0.5)) * step_ld)]).astype(np.float64)
    base = base[(base >= lo) & (base <= hi) & (base != 0.0)]
    return _step64(base[:, None], np.arange(-2, 3)[None, :]).ravel()


def _pow_ks():
    return sorted(set(range(-148, 85, 4)) | {-148, 84, -1, 0, 1, 5})


def _p10_rows64(narrow=None):
    """(la, x, y): a grid over la in [-12, 12], x in [1e-12, 1], y in [0, 3], then cancelling rows.  narrow: a function
    that rounds an array to the arithmetic under test (binary32), applied to x and y BEFORE la is solved for."""
    nar = narrow or (lambda a: a)
    la_g = np.linspace(-12, 12, 25)
    x_g = nar(np.concatenate([10.0 ** np.arange(-12, 1), 10.0 ** np.linspace(-12, 0, 23) * 1.37, [1.0]]))
    x_g = x_g[(x_g >= 1e-12) & (x_g <= 1.0)]
    y_g = nar(np.array([0.0, 0.25, 0.5, 1.0, 4.0 / 3.0, 2.0, 2.5, 3.0]))
    la, xy = _cross(la_g, np.arange(x_g.size * y_g.size))
    x, y = x_g[xy // y_g.size], y_g[xy % y_g.size]
    # cancellation: la = (t - y log2 x) / log2 10 with the total t = (m/2 + delta) / 64, |t| <= 1
    xs, ys = _cross(nar(np.array([1e-3, 3.7e-3, 0.02, 0.11, 0.5, 0.93])), nar(np.array([0.5, 1.0, 4.0 / 3.0, 2.0, 3.0])))
    m = np.arange(-128, 129)
    delta = np.array([0.0, 2.0 ** -21, -2.0 ** -21, 2.0 ** -30, -2.0 ** -30])
    mm, dd = _cross(m, delta)
    t = ((mm.astype(LD) / 2 + dd.astype(LD)) / 64)
    yl = ys.astype(LD) * np.log2(xs.astype(LD))
    la_c = ((t[None, :] - yl[:, None]) / LOG2_10).astype(np.float64)
    xc, yc = np.repeat(xs, t.size), np.repeat(ys, t.size)
    la_c = nar(la_c.ravel())
    keep = np.abs(la_c) <= 12
    return np.concatenate([la, la_c[keep]]), np.concatenate([x, xc[keep]]), np.concatenate([y, yc[keep]])


def _root_points64():
    e = np.arange(-123, 123)
    base = 2.0 ** e.astype(np.float64)
    pts = np.concatenate([base, _step64(base, 1), _step64(2.0 * base, -1)])
    n = np.arange(1, 2001, dtype=np.float64)
    sq = np.concatenate([n * n, (n * n)[:, None].repeat(4, 1).ravel() * np.tile(2.0 ** np.array([-120, -62, 60, 118.0]), n.size)])
    cu = np.concatenate([n ** 3, (n ** 3)[:, None].repeat(4, 1).ravel() * np.tile(2.0 ** np.array([-120, -63, 60, 87.0]), n.size)])
    ends = np.concatenate([_step64(1e-37, np.arange(0, 4)), _step64(1e37, -np.arange(0, 4))])
    allp = np.concatenate([pts, sq, cu, ends, _filler(-36, 36, 20000, 11)])
    return allp[(allp >= 1e-37) & (allp <= 1e37)]


def _div_rows(step, dtype, emax, seed, lo10, hi10):
    """(a, b) for a / b: denominators of exponent -emax .. emax, a seeded filler over 10**lo10 .. 10**hi10 on both sides.
    step = _step64 or _step32."""
    e = np.arange(-emax, emax + 1)
    base = (2.0 ** e.astype(np.float64)).astype(dtype)
    b = np.concatenate([base, step(base, 1), step((2 * base).astype(dtype), -1)]).astype(dtype)
    one, two = dtype(1), dtype(2)
    rows = [(b, b), (_ones(b), b)]                                                     # a == b; 1 / b
    for q in (step(one, -1), step(one, 1), step(two, -1), step(two, 1)):              # quotients one ulp either side of 1, 2
        rows.append(((b * q).astype(dtype), b))
    fill = _filler(lo10, hi10, 4000, seed).astype(dtype)
    rc = (one / fill).astype(dtype)                                                    # neighbours of reciprocals: b * fl(1/b) ~ 1
    for d in (-2, -1, 0, 1, 2):
        rows.append((_ones(fill), step(rc, d)))
        rows.append((fill, step(rc, d)))
    rows.append((_filler(lo10, hi10, 20000, seed + 1).astype(dtype), _filler(lo10, hi10, 20000, seed + 2).astype(dtype)))
    a = np.concatenate([r[0] for r in rows]).astype(np.float64)
    bb = np.concatenate([r[1] for r in rows]).astype(np.float64)
    return a, bb


_cache = {}


def cases64():
    if "64" in _cache:
        return _cache["64"]
    c = {}
    lt = ln_table_points()
    n1 = near_one64()
    for f in ("log", "log10"):
        c[f + "@table"] = (lt, _ones(lt), _ones(lt))
        c[f + "@near1"] = (n1, _ones(n1), _ones(n1))
    k, y = _cross(np.arange(-100, 81), np.arange(-4, 5))
    c["pow@pow2"] = (2.0 ** k.astype(np.float64), y.astype(np.float64), _ones(y.astype(np.float64)))
    ln2_64, l10_64 = np.log(LD(2)) / 64, np.log10(LD(2)) / 64
    xe = np.concatenate([_ties64(ln2_64, -100, 50), [0.0, -0.0, 1e-300, -1e-300]])
    c["exp@ties"] = (xe, _ones(xe), _ones(xe))
    xt = np.concatenate([_ties64(l10_64, -40, 20), [0.0, -0.0, 1e-300, -1e-300]])
    c["exp10@ties"] = (xt, _ones(xt), _ones(xt))
    px, py = _cross(ln_table_points(_pow_ks()), np.array(POW_Y))
    keep = np.abs(py * np.log2(px)) <= 1000
    px, py = px[keep], py[keep]
    c["pow@table"] = (px, py, _ones(px))
    la, x, y = _p10_rows64()
    c["pow10_times_pow@grid"] = (la, x, y)
    r = _root_points64()
    c["sqrt@edges"] = (r, _ones(r), _ones(r))
    c["cbrt@edges"] = (r, _ones(r), _ones(r))
    a, b = _div_rows(_step64, np.float64, 100, 21, -30, 30)
    for f in ("div", "rcp", "ieee_div", "plain_div", "plain_rcp"):
        c[f + "@edges"] = (a, b, _ones(a))
    _cache["64"] = c
    return c


# ---------------------------------------------------------------- binary32
def _binades32():
    """2**k -3 .. +3 ulps for every binade 2**-126 .. 2**127, sixteen mantissas inside each, never below FLT_MIN or non-finite"""
    base = (2.0 ** np.arange(-126, 128).astype(np.float64)).astype(f32)
    pts = _step32(base[:, None], np.arange(-3, 4)[None, :]).ravel()
    inner = (base[:, None].astype(np.float64) * (1.0 + np.arange(1, 17) / 17.0)[None, :]).astype(f32).ravel()
    top = _step32(f32(FLT_MAX), -np.arange(0, 4))
    allp = np.concatenate([pts, inner, top])
    return allp[np.isfinite(allp) & (allp >= f32(FLT_MIN))]


def near_one32():
    return np.concatenate([_step32(f32(1), np.arange(0, 2001)), _step32(f32(1), -np.arange(1, 2001))])


def _ties32(scale_ld, lo, hi):
    """binary32 x with hi = x * scale next to an integer or a half-integer (the rint ties), +-1, 2 ulps, x in [lo, hi]"""
    n = np.arange(int(np.ceil(LD(lo) * scale_ld)) - 1, int(np.floor(LD(hi) * scale_ld)) + 2).astype(LD)
    base = np.concatenate([n / scale_ld, (n + LD(0.5)) / scale_ld]).astype(f32)
    base = base[base != 0]
    pts = _step32(base[:, None], np.arange(-2, 3)[None, :]).ravel()
    return pts[(pts >= f32(lo)) & (pts <= f32(hi))]


def _w(a):
    return np.ascontiguousarray(a, dtype=f32).astype(np.float64)


def cases32():
    if "32" in _cache:
        return _cache["32"]
    c = {}
    bn = _binades32()
    n1 = near_one32()
    fill = _filler(-45, 25, 20000, 31)
    fill = fill[(fill >= 1.2e-38)]
    lx = _w(np.concatenate([bn, n1, fill.astype(f32)]))
    for f in ("log", "log10"):
        c[f + "@all"] = (lx, _ones(lx), _ones(lx))
    rng = np.random.default_rng(32)
    xe = _w(np.concatenate([_ties32(LOG2_E, -87, 88), rng.uniform(-87, 50, 20000).astype(f32), f32([0.0, -0.0, 1e-30, -1e-30])]))
    c["exp@ties"] = (xe, _ones(xe), _ones(xe))
    xt = _w(np.concatenate([_ties32(LOG2_10, -37, 38), rng.uniform(-37, 20, 20000).astype(f32), f32([0.0, -0.0, 1e-30, -1e-30])]))
    c["exp10@ties"] = (xt, _ones(xt), _ones(xt))
    px, py = _cross(np.concatenate([bn, n1[::50], fill[::4].astype(f32)]), f32(POW_Y))
    px, py = _w(px), _w(py)
    keep = np.abs(py * np.log2(px)) <= 120
    c["pow@all"] = (px[keep], py[keep], _ones(px[keep]))
    la, x, y = _p10_rows64(narrow=lambda a: np.asarray(a).astype(f32).astype(np.float64))
    la = _w(la)
    tot = la * float(LOG2_10) + y * np.log2(x)
    keep = (np.abs(tot) <= 120) & (np.abs(la) <= 12)
    c["pow10_times_pow@grid"] = (la[keep], x[keep], y[keep])
    n = np.arange(1, 2001, dtype=np.float64)
    sq = np.concatenate([n * n, n * n * 2.0 ** -120, n * n * 2.0 ** 100])                     # n*n < 2**24: exact in binary32
    cu = n[:255] ** 3                                                                         # < 2**24
    cu = np.concatenate([cu, cu * 2.0 ** -123, cu * 2.0 ** 99])
    base = (2.0 ** np.arange(-126, 128).astype(np.float64)).astype(f32)
    r = _w(np.concatenate([base, _step32(base, 1), _step32(base[1:], -1), [f32(FLT_MAX)], sq.astype(f32), cu.astype(f32),
                           _filler(-36, 36, 20000, 33).astype(f32)]))
    c["sqrt@edges"] = (r, _ones(r), _ones(r))
    c["cbrt@edges"] = (r, _ones(r), _ones(r))
    # operands kept where neither 1/b nor a/b leaves the binary32 normal range: |log2 b| <= 60 (+1), quotients within 2**+-121
    a, b = _div_rows(_step32, f32, 60, 41, -17, 17)
    for f in ("plain_div", "plain_rcp", "rcp_seed"):
        c[f + "@edges"] = (a, b, _ones(a))
    for v in c.values():
        for arr in v:
            assert np.array_equal(arr.astype(f32).astype(np.float64), arr) and np.isfinite(arr).all()
    _cache["32"] = c
    return c


def subnormal_rows32():
    """Characterisation only: each binary32 function at FLT_MIN and at the largest denormal."""
    return _w(np.array([FLT_MIN, np.nextafter(f32(FLT_MIN), f32(0))], dtype=f32))


def mixed_pow_cases():
    """pow(double, float) and pow(float, double): binary32-representable x resp. y from the tables above, the other
    operand a genuine binary64 value."""
    px, py = _cross(ln_table_points([-60, -1, 0, 1, 5, 40]), np.array(POW_Y))
    df = (px, _w(py.astype(f32)), _ones(px))                                        # y narrowed
    bx = _w(np.concatenate([_binades32()[::3], near_one32()[::20]]))
    fx, fy = _cross(bx, np.array(POW_Y))
    keep = np.abs(fy * np.log2(fx)) <= 120
    return {"pow_df@table": df, "pow_fd@table": (fx[keep], fy[keep], _ones(fx[keep]))}


# ---------------------------------------------------------------- references and error measures
def fn_of(name):
    return name.split("@")[0]


def reference(name, x, y, z):
    """The function in numpy longdouble (64-bit mantissa on x86)."""
    f = fn_of(name)
    xl, yl, zl = x.astype(LD), y.astype(LD), z.astype(LD)
    with np.errstate(all="ignore"):
        if f == "log":
            return np.log(xl)
        if f == "log10":
            return np.log10(xl)
        if f == "exp":
            return np.exp(xl)
        if f == "exp10":
            return np.power(LD(10), xl)
        if f == "sqrt":
            return np.sqrt(xl)
        if f == "cbrt":
            return np.cbrt(xl)
        if f in ("pow", "pow_df", "pow_fd"):
            return np.power(xl, yl)
        if f in ("div", "ieee_div", "plain_div"):
            return xl / yl
        if f in ("rcp", "plain_rcp", "rcp_seed"):
            return LD(1) / yl
        if f == "pow10_times_pow":
            return np.exp2(xl * LOG2_10 + zl * np.log2(yl))
    raise KeyError(name)


def ulp_err(got, want_ld, dtype=np.float64):
    """|got - want| in ulps of the correctly rounded result (ulp of its binade), elementwise"""
    w = want_ld.astype(dtype)
    u = np.abs(np.nextafter(w, dtype(np.inf)) - w).astype(LD)
    return (np.abs(got.astype(LD) - want_ld) / u).astype(np.float64)


def exponent_bits(name, x, y, z):
    """sum of the |exponent terms in bits| of an exponential-family function: what its binary32 error bound scales with"""
    f = fn_of(name)
    if f == "exp":
        return np.abs(x * float(LOG2_E))
    if f == "exp10":
        return np.abs(x * float(LOG2_10))
    if f == "pow":
        return np.abs(y * np.log2(x))
    if f == "pow10_times_pow":
        return np.abs(x * float(LOG2_10)) + np.abs(z * np.log2(y))
    raise KeyError(name)


def exp_family_C(name, got, x, y, z):
    """max of relative error / (2**-24 (1 + sum |terms|))"""
    want = reference(name, x, y, z)
    rel = np.abs(got.astype(LD) - want) / np.abs(want)
    return (rel / (LD(2.0) ** -24 * (1 + exponent_bits(name, x, y, z)))).astype(np.float64)
