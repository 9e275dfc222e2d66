"""fastmath.h on the device at the edges of its reductions (-m gpu): the cases of fastmath_cases.py through
kidmp_math_probe_ex, whose unit is compiled with the column kernel's own flags.

  bit identity   binary64 log, log10, exp, exp10, pow, pow10_times_pow and the mixed-type powers give the bits of the host
                 build of the header (tests/native/fastmath_eval.cpp) on every case: the header's claim, and what makes
                 the host accuracy tests count for the GPU.  sqrt, cbrt, div, rcp start from other seeds on the device and
                 are held to 1 ulp against longdouble instead (the bounds of test_gpu_fastmath.py)
  old = new      the eleven codes of kidmp_math_probe (built without the column flags) and the same codes of the new entry
                 agree bit for bit: the flags do not change the fm:: functions
  binary32       the header's bounds for sqrt, cbrt, log (1, 1, 2 ulp); for log10 the bound derived in the header from the
                 unit's 1 ulp, the product's rounding and the rounding of fl32(log10 2), 2.51 ulp (2 ulp hold on the host
                 only: 2.48 measured on the device); C <= 2 for the exponential family (the special-function
                 units are specified to 1 ulp where the host's libm is sub-ulp; the host test asserts C <= 1);
                 the plain x / y and 1 / y of the column objects (v_rcp_f32 and a product) <= 2.5 ulp: 1 ulp of the
                 reciprocal, 1/2 of the product, and the slack of judging in the quotient's binade
  refusals       write nothing
Every measured maximum is printed (pytest -s) and recorded in DESIGN.md.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import fastmath_cases as fc
from test_fastmath_edges import BOUND64, EXP_FAMILY, ULP32, binary32_figures, check_exact64, host_eval, worst  # noqa: F401

pytestmark = pytest.mark.gpu

BIT_IDENTICAL = ("log", "log10", "exp", "exp10", "pow", "pow10_times_pow")
SEEDED = ("sqrt", "cbrt", "div", "rcp")                       # other seeds on the device: 1 ulp each, as test_gpu_fastmath.py


def _log_bound32(c_exact, unit_ulp=1.0):
    """ulps of fl32(c) * log2_hw(x), as fastmath.h derives it: the unit's error scaled by the ratio of the two ulps (c
    brought into [1, 2)), the rounding of the constant times the result's mantissa (< 2), the product's half ulp"""
    k = float(c_exact / fc.LD(2) ** np.floor(np.log2(c_exact)))
    dc = float(abs(fc.LD(np.float32(c_exact)) / c_exact - 1))
    return unit_ulp * k + 2 * dc * 2.0 ** 23 + 0.5


DEVICE_ULP32 = dict(ULP32, log10=_log_bound32(np.log10(fc.LD(2))))
assert _log_bound32(np.log(fc.LD(2))) <= ULP32["log"] and 2.50 < DEVICE_ULP32["log10"] < 2.51
DIV_ULP32 = {"plain_div": 2.5, "plain_rcp": 2.5}              # x / y and 1 / y of the column objects (see above); read by parity32.probe_ulps


@functools.lru_cache(maxsize=None)
def _ref(bits, name):
    return fc.reference(name, *(fc.cases64() if bits == 64 else fc.cases32())[name])


@pytest.mark.parametrize("name", [n for n in fc.cases64() if fc.fn_of(n) in BIT_IDENTICAL])
def test_binary64_device_bits_are_the_host_bits(name, gpu_mixed, host_eval):
    x, y, z = fc.cases64()[name]
    dev = gpu_mixed.math_probe_ex(fc.fn_of(name), x, y, z)
    host = host_eval(name, x, y, z)
    differ = dev.view(np.int64) != host.view(np.int64)
    err = fc.ulp_err(dev, _ref(64, name))
    print(name, "device", worst(err, x, y, z), "| differing from the host build:", int(differ.sum()))
    assert not differ.any(), (name, int(differ.sum()), float(x[differ][0]).hex(), float(y[differ][0]).hex(), float(z[differ][0]).hex())
    assert err.max() <= BOUND64[fc.fn_of(name)]


def test_mixed_type_powers_on_the_device(gpu_mixed, host_eval):
    for name, (x, y, z) in fc.mixed_pow_cases().items():
        dev = gpu_mixed.math_probe_ex(fc.fn_of(name), x, y, z)
        assert np.array_equal(dev.view(np.int64), host_eval(name, x, y, z).view(np.int64)), name
        assert np.array_equal(dev.view(np.int64), gpu_mixed.math_probe_ex("pow", x, y, z).view(np.int64)), name


def test_binary64_exact_values_on_the_device(gpu_mixed):
    check_exact64(lambda f, x, y, z: gpu_mixed.math_probe_ex(f, x, y, z))


@pytest.mark.parametrize("name", [n for n in fc.cases64() if fc.fn_of(n) in SEEDED])
def test_binary64_seeded_functions_within_one_ulp(name, gpu_mixed):
    x, y, z = fc.cases64()[name]
    err = fc.ulp_err(gpu_mixed.math_probe_ex(fc.fn_of(name), x, y, z), _ref(64, name))
    print(name, "device", worst(err, x, y, z))
    assert err.max() <= 1.0, worst(err, x, y, z)


def test_old_probe_and_new_probe_agree(gpu_mixed):
    """kidmp_diag.hip is built with the plain flags, kidmp_mathprobe.hip with the column objects': if a function differed,
    the accuracy figures taken through the old probe would describe other code than the kernel's."""
    c = fc.cases64()
    pick = {"log": "log@table", "log10": "log10@near1", "exp": "exp@ties", "exp10": "exp10@ties", "sqrt": "sqrt@edges",
            "cbrt": "cbrt@edges", "pow": "pow@table", "rcp_seed": "div@edges", "div": "div@edges", "ieee_div": "div@edges",
            "rcp": "div@edges"}
    assert tuple(pick) == gpu_mixed.MATH_FUNCS
    differing = {}
    for f, name in pick.items():
        x, y, z = c[name]
        old = gpu_mixed.math_probe(f, x, y)
        new = gpu_mixed.math_probe_ex(f, x, y, z)
        n = int((old.view(np.int64) != new.view(np.int64)).sum())
        if n:
            differing[f] = n
    assert not differing, differing
    x, y, z = c["div@edges"]
    assert np.array_equal(gpu_mixed.math_probe_ex("ieee_div", x, y, z), x / y)            # it is IEEE division


@pytest.mark.parametrize("name", [n for n in fc.cases32() if fc.fn_of(n) in ULP32 or fc.fn_of(n) in EXP_FAMILY])
def test_binary32_on_the_device(name, gpu_mixed):
    x, y, z = fc.cases32()[name]
    got = gpu_mixed.math_probe_ex(fc.fn_of(name), x, y, z, binary32=True)
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got)
    fig = binary32_figures(name, got, x, y, z)
    print(name, "binary32 device", fig)
    if "C" in fig:
        assert fig["C"] <= 2.0, fig
    else:
        assert fig["ulp"] <= DEVICE_ULP32[fc.fn_of(name)], fig
        assert fig.get("abs_near_1", 0.0) <= 1e-7, fig


def test_binary32_division_as_the_column_objects_compile_it(gpu_mixed):
    """x / y and 1 / y on REAL operands.  The operands are kept where neither the reciprocal nor the quotient leaves the
    binary32 normal range (|log2 y| <= 61, quotients within 2**+-121): a denormal reciprocal is another question."""
    x, y, z = fc.cases32()["plain_div@edges"]
    q = x.astype(fc.LD) / y.astype(fc.LD)
    assert (np.abs(np.log2(y)) <= 61).all() and (np.abs(np.log2(q.astype(np.float64))) <= 121).all()
    fig = {}
    for f, want in (("plain_div", q), ("plain_rcp", 1 / y.astype(fc.LD)), ("rcp_seed", 1 / y.astype(fc.LD))):
        got = gpu_mixed.math_probe_ex(f, x, y, z, binary32=True)
        fig[f] = float(fc.ulp_err(got, want, np.float32).max())
    print("binary32 division on the device, max ulp:", fig)
    assert fig["plain_div"] <= DIV_ULP32["plain_div"] and fig["plain_rcp"] <= DIV_ULP32["plain_rcp"], fig
    # binary64 operands through the same flags (the compiler's reciprocal + Newton expansion): printed for the record
    x, y, z = fc.cases64()["plain_div@edges"]
    for f in ("plain_div", "plain_rcp"):
        err = fc.ulp_err(gpu_mixed.math_probe_ex(f, x, y, z), _ref(64, f + "@edges"))
        print("binary64", f, "under the column flags:", worst(err, x, y, z))


def test_below_flt_min_is_on_record(gpu_mixed):
    """Characterisation only: the stated domain is "positive, finite, normal".  What each binary32 function returns at
    FLT_MIN and at the largest denormal is printed and copied to DESIGN.md; asserted: the call returns."""
    x = fc.subnormal_rows32()
    one = np.ones_like(x)
    rows = [("log", x, one, one), ("log10", x, one, one), ("sqrt", x, one, one), ("cbrt", x, one, one),
            ("pow", x, 0.5 * one, one), ("pow", x, -one, one), ("pow10_times_pow", 30 * one, x, one),
            ("plain_rcp", one, x, one), ("plain_div", x, one * 0.5, one), ("rcp_seed", one, x, one),
            ("exp", -87.5 * one, one, one), ("exp", -88.0 * one, one, one), ("exp10", -38.0 * one, one, one)]
    for f, a, b, c in rows:
        got = gpu_mixed.math_probe_ex(f, a, b, c, binary32=True)
        want = fc.reference(f, a, b, c)
        print("sub-FLT_MIN %-16s x=%s y=%s z=%s -> %s (exact %s)" % (f, a, b, c, got, want.astype(np.float64)))
        assert got.shape == x.shape


def test_refusals_write_nothing(gpu_mixed):
    from kid_amd.thompson import load_library
    L = load_library()
    dp = C.POINTER(C.c_double)
    x = np.full(8, 2.0)
    out = np.full(8, -77.0)
    px, po = x.ctypes.data_as(dp), out.ctypes.data_as(dp)
    h = gpu_mixed._h
    bad = [(h, 16, 0, 8, px, px, px, po), (h, -1, 0, 8, px, px, px, po), (h, 0, 0, -1, px, px, px, po),
           (h, 0, 0, 8, None, px, px, po), (h, 0, 0, 8, px, None, px, po), (h, 0, 0, 8, px, px, None, po),
           (h, 8, 1, 8, px, px, px, po), (h, 10, 1, 8, px, px, px, po), (h, 9, 1, 8, px, px, px, po),
           (h, 14, 1, 8, px, px, px, po), (h, 15, 1, 8, px, px, px, po)]
    for args in bad:
        assert L.kidmp_math_probe_ex(*args) == -1, args[1:4]
        assert (out == -77.0).all()
    assert L.kidmp_math_probe_ex(h, 0, 0, 8, px, px, px, None) == -1
    assert L.kidmp_math_probe_ex(None, 0, 0, 8, px, px, px, po) == -5
    assert (out == -77.0).all()
    assert L.kidmp_math_probe_ex(h, 0, 0, 0, px, px, px, po) == 0 and (out == -77.0).all()       # n == 0 succeeds
    with pytest.raises(ValueError):
        gpu_mixed.math_probe_ex("log", np.array([0.1]), binary32=True)                           # 0.1 is not a binary32 value
    with pytest.raises(ValueError):
        gpu_mixed.math_probe_ex("pow_df", np.array([2.0]), np.array([0.1]))
    assert gpu_mixed.math_probe_ex("log", np.array([1.0]), binary32=True)[0] == 0.0
