"""kid_amd/csrc/fastmath.h at the edges of its reductions, host build (no GPU): the deterministic cases of
fastmath_cases.py through tests/native/fastmath_eval.cpp against numpy longdouble (64-bit mantissa).

binary64: the bounds of test_fastmath.py (its BOUNDS, imported), and the exact equalities the reductions promise.
binary32: the header's own claims -- sqrt, cbrt <= 1 ulp; log, log10 <= 2 ulp outside |x - 1| <= 2**-4 and 1e-7 absolute
inside; exp, exp10, pow, pow10_times_pow: relative error <= C 2**-24 (1 + sum of the |exponent terms in bits|) with C <= 1
on the host, where glibc's log2f / exp2f stand in for the special-function units.  The sum runs over the TERMS
(|la log2 10| + |y log2 x| for pow10_times_pow): the binary32 roundings of the two terms do not cancel when the terms do.
"""
import os
import subprocess

import numpy as np
import pytest

import fastmath_cases as fc
from test_fastmath import BOUNDS

ROOT = fc.ROOT


@pytest.fixture(scope="module")
def host_eval(tmp_path_factory):
    d = tmp_path_factory.mktemp("fmeval")
    exe = str(d / "fastmath_eval")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "kid_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "fastmath_eval.cpp"), "-o", exe])
    return lambda name, x, y, z, binary32=False: run_host_eval(exe, str(d), name, x, y, z, binary32)


def run_host_eval(exe, workdir, name, x, y, z, binary32=False):
    """out = fn(x, y, z) on the host build of fastmath.h (shared with test_gpu_fastmath_edges.py)"""
    fin, fout = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([fc.FN.index(fc.fn_of(name)), int(binary32)], dtype=np.int32).tobytes())
        f.write(np.array([x.size], dtype=np.int64).tobytes())
        for a in (x, y, z):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    subprocess.check_call([exe, fin, fout])
    out = np.fromfile(fout, dtype=np.float64)
    assert out.size == x.size
    return out


BOUND64 = {"log": BOUNDS["log"], "log10": BOUNDS["log10"], "exp": BOUNDS["exp"], "exp10": BOUNDS["exp10"], "pow": BOUNDS["pow"],
           "pow10_times_pow": BOUNDS["pow10_times_pow"], "sqrt": BOUNDS["sqrt_pos"], "cbrt": BOUNDS["cbrt_pos"],
           "div": BOUNDS["div"], "rcp": BOUNDS["rcp"]}


def worst(err, x, y, z):
    i = int(np.argmax(err))
    return "max %.3f at x=%s y=%s z=%s" % (err[i], float(x[i]).hex(), float(y[i]).hex(), float(z[i]).hex())


@pytest.mark.parametrize("name", [n for n in fc.cases64() if fc.fn_of(n) in BOUND64])
def test_binary64_edges_within_the_bounds(name, host_eval):
    x, y, z = fc.cases64()[name]
    got = host_eval(name, x, y, z)
    err = fc.ulp_err(got, fc.reference(name, x, y, z))
    print(name, worst(err, x, y, z))
    assert err.max() <= BOUND64[fc.fn_of(name)], worst(err, x, y, z)


def check_exact64(ev):
    """The equalities the binary64 reductions promise; ev(name, x, y, z) evaluates (host or device)."""
    one = np.array([1.0])
    for f in ("log", "log10"):
        r = ev(f, one, one, one)
        assert r[0] == 0.0 and not np.signbit(r[0]), f                     # +0.0 exactly
    x, y, z = fc.cases64()["pow@pow2"]
    assert np.array_equal(ev("pow", x, y, z), np.exp2(np.log2(x) * y))      # 2**(k y), integral: exact
    e = np.array([0.0, -0.0, 1e-300, -1e-300])
    assert np.array_equal(ev("exp", e, _1(e), _1(e)), _1(e))
    assert np.array_equal(ev("exp10", e, _1(e), _1(e)), _1(e))
    x, y, z = fc.cases64()["pow@table"]
    x0 = x[y == 0.0]
    assert np.array_equal(ev("pow", x0, np.zeros_like(x0), _1(x0)), _1(x0))
    x1 = x[y == 1.0]
    assert fc.ulp_err(ev("pow", x1, _1(x1), _1(x1)), x1.astype(fc.LD)).max() <= BOUNDS["pow"]


def _1(a):
    return np.ones_like(a)


def test_binary64_exact_values(host_eval):
    check_exact64(host_eval)


def test_mixed_type_powers_are_the_binary64_power(host_eval):
    for name, (x, y, z) in fc.mixed_pow_cases().items():
        got = host_eval(name, x, y, z)
        assert np.array_equal(got, host_eval("pow", x, y, z)), name
        assert fc.ulp_err(got, fc.reference(name, x, y, z)).max() <= BOUNDS["pow"], name


# ---- binary32: the claims of the header's comment
ULP32 = {"sqrt": 1.0, "cbrt": 1.0, "log": 2.0, "log10": 2.0}
EXP_FAMILY = ("exp", "exp10", "pow", "pow10_times_pow")


def binary32_figures(name, got, x, y, z):
    """What the header bounds for this function: {"ulp": max ulps [, "abs_near_1": max absolute error]} or {"C": max C}"""
    f = fc.fn_of(name)
    if f in EXP_FAMILY:
        return {"C": float(fc.exp_family_C(name, got, x, y, z).max())}
    want = fc.reference(name, x, y, z)
    err = fc.ulp_err(got, want, np.float32)
    if f in ("log", "log10"):
        near = np.abs(x - 1.0) <= 2.0 ** -4
        return {"ulp": float(err[~near].max()), "abs_near_1": float(np.abs(got.astype(fc.LD) - want)[near].max())}
    return {"ulp": float(err.max())}


@pytest.mark.parametrize("name", [n for n in fc.cases32() if fc.fn_of(n) in ULP32 or fc.fn_of(n) in EXP_FAMILY])
def test_binary32_edges_within_the_header_claims(name, host_eval):
    x, y, z = fc.cases32()[name]
    got = host_eval(name, x, y, z, binary32=True)
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got)
    fig = binary32_figures(name, got, x, y, z)
    print(name, fig)
    if "C" in fig:
        assert fig["C"] <= 1.0, fig
    else:
        assert fig["ulp"] <= ULP32[fc.fn_of(name)], fig
        assert fig.get("abs_near_1", 0.0) <= 1e-7, fig


def test_binary32_division_on_the_host_is_ieee(host_eval):
    x, y, z = fc.cases32()["plain_div@edges"]
    q = host_eval("plain_div", x, y, z, binary32=True)
    assert np.array_equal(q, (x.astype(np.float32) / y.astype(np.float32)).astype(np.float64))
    r = host_eval("plain_rcp", x, y, z, binary32=True)
    assert np.array_equal(r, (np.float32(1) / y.astype(np.float32)).astype(np.float64))


def test_the_generator_hits_what_it_says():
    """The constructions, checked on the cases themselves: the table edges are where the bin index changes, the ties are
    within an ulp of a half-integer number of 64ths, and the cancelling rows of pow10_times_pow do cancel."""
    off, n, shift = fc.table_constants()
    x = fc.ln_table_points([0])
    hi = (x.view(np.int64) >> 32).astype(np.int64)
    idx = ((hi - off) >> shift) & (n - 1)
    edge_rows = idx.reshape(n + 1, 7)
    assert all(edge_rows[i, 2] != edge_rows[i, 3] for i in range(1, n))      # -1 ulp and the edge itself: different bins
    xe = fc.cases64()["exp@ties"][0]
    t = xe.astype(fc.LD) * 64 / np.log(fc.LD(2))
    assert np.mean(np.abs(t * 2 - np.rint(t * 2)) < 1e-10) > 0.99
    la, xx, yy = fc.cases64()["pow10_times_pow@grid"]
    tot = la.astype(fc.LD) * fc.LOG2_10 + yy.astype(fc.LD) * np.log2(xx.astype(fc.LD))
    terms = np.abs(la * float(fc.LOG2_10)) + np.abs(yy * np.log2(xx))
    cancelling = (np.abs(tot) <= 1) & (terms > 4)
    assert cancelling.sum() > 1000
    frac = tot[cancelling] * 128
    assert np.mean(np.abs(frac - np.rint(frac)) < 128 * 2.0 ** -20) > 0.9
    for c in (fc.cases64(), fc.cases32()):
        for name, arrs in c.items():
            assert 1000 < arrs[0].size <= 400_000, name
