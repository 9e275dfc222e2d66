"""The HIP entries that have a counterpart in the reference Fortran, against what that Fortran itself computed
(tests/golden/reference_*.npz, recorded from the reference built from source; see tests/test_reference_goldens.py for
how the CPU oracle stands against the same records).  -m gpu; reads nothing but tests/golden/.

What `got` is compared with is the RECORD.  The oracle supplies only what a record cannot: its own sensitivity at each
level, a value at the U1 entries the reference leaves undefined (output qc and nc at level kts, NaN in the record), and
the two admissible outcomes of the residue-decided tests (M:3587, M:3596): at a level on one of them the HIP result must
equal the record or the other outcome, and the record itself must be one of the two (parity.branch_aware_compare).  Bounds are those the same entries are held
to against the oracle today (tests/parity.py, tests/rates_parity.py, test_gpu_parity, test_gpu_reflectivity,
test_gpu_precision, test_gpu_kid_adapter), unchanged.
"""
import numpy as np
import pytest

import reference_record as rr
from parity import OUT, against_record, assert_parity
from rates_parity import assert_rates
from test_reference_goldens import (DT, _inputs, _outputs, _records, adapter_case, adapter_error, adapter_logged_rates,
                                    p32n_errors)

pytestmark = pytest.mark.gpu
BOUND_DB = 3e-13                     # test_gpu_reflectivity.BOUND_DB
BOUND_RADII = 1e-12                  # test_gpu_parity.test_effective_radii_match_oracle
_cache = {}


def _rec(tree):
    if tree not in _cache:
        _cache[tree] = _records(tree)
    return _cache[tree]


def _pair(request, rec, b):
    kind = "warm" if rec[b + ".iiwarm"] else ("mixed_aero" if rec[b + ".aero"] else "mixed")
    return request.getfixturevalue("gpu_" + kind), request.getfixturevalue("oracle_" + kind)


# nz = 33, 120 and 200: each level-group count of the kernel meets a recorded answer; aero120 is the aerosol-aware branch
@pytest.mark.parametrize("b", ["warm120", "mixed33", "mixed120", "seeded120", "mixed200", "aero120"])
def test_column_step_matches_the_reference(request, b):
    rec = _rec("p64")
    m, o = _pair(request, rec, b)
    st = _inputs(rec, b)
    got = {k: v.copy() for k, v in st.items()}
    has_rates = b + ".rates" in rec
    gppt, rates = m.batch_step_host(got, DT, want_rates=has_rates)
    v = assert_parity(o, st, DT, got, gppt, record=_outputs(rec, b), record_ppt=rec[b + ".ppt"])
    print(b, "column step vs reference:", v)
    assert all(np.isfinite(got[k]).all() for k in OUT)
    if has_rates:
        cols = rec[b + ".rate_cols"]
        sub = {k: np.ascontiguousarray(x[cols]) for k, x in st.items()}
        rv = assert_rates(o.column_step, sub, DT, rates[cols], record=rec[b + ".rates"])
        rv.pop("cmp")
        print(b, "rates vs reference:", rv)


@pytest.mark.parametrize("b", ["warm120", "mixed33", "mixed120", "seeded120", "mixed200", "aero120"])
def test_diagnostics_match_the_reference(request, b):
    """reflectivity, effective_radii_host and column_outputs on the input state and on the state the reference stepped to
    (its U1 entries filled with the oracle's values; re_qc, NaN at kts there, is not compared at that level)."""
    import torch
    rec = _rec("p64")
    m, o = _pair(request, rec, b)
    st = _inputs(rec, b)
    stepped = {k: v.copy() for k, v in st.items()}
    o.batch_step(stepped, DT)
    stepped.update({k: np.ascontiguousarray(v) for k, v in against_record(_outputs(rec, b), stepped).items()})
    for state, sfx in ((st, "_in"), (stepped, "")):
        dev = {k: torch.from_numpy(np.ascontiguousarray(state[k])).cuda() for k in m.OUTPUT_NAMES}
        want_dbz = rec["%s.dbz%s" % (b, sfx)]
        want_re = [rec["%s.%s%s" % (b, n, sfx)] for n in ("re_qc", "re_qi", "re_qs")]
        dbz = m.reflectivity({k: dev[k] for k in m.REFL_NAMES}).cpu().numpy()
        both_dbz, both_re = m.column_outputs(dev)
        torch.cuda.synchronize()
        host_re = m.effective_radii_host({k: state[k] for k in m.RADII_NAMES})
        for g in (dbz, both_dbz.cpu().numpy()):
            assert np.abs(g - want_dbz).max() <= BOUND_DB, (b, sfx, float(np.abs(g - want_dbz).max()))
        for radii in (host_re, [r.cpu().numpy() for r in both_re]):
            for g, r, n in zip(radii, want_re, ("re_qc", "re_qi", "re_qs")):
                e = np.abs(g - r) / r
                assert np.isnan(e).sum() == (r.shape[0] if (n, sfx) == ("re_qc", "") else 0), (b, n, sfx)
                assert np.nanmax(e) < BOUND_RADII, (b, n, sfx, float(np.nanmax(e)))


@pytest.mark.parametrize("name", rr.TABLES)
def test_table_matches_the_reference(gpu_mixed, name):
    """The sampled elements at the bound and metric of test_gpu_parity.test_table_matches_oracle; the sum and the sum of
    absolute values at that bound times the square root of the element count, relative to the sum of absolute values."""
    T = _cache.setdefault("tables", rr.load("reference_tables.npz"))
    flat, v = gpu_mixed.table(name), T[name + ".val"]
    assert flat.size == int(np.prod(T[name + ".shape"]))
    e = np.abs(flat[T[name + ".idx"]] - v) / np.maximum(np.abs(v), 1e-30 + 1e-13 * np.max(np.abs(flat)))
    assert e.max() < 1e-11, (name, float(e.max()))
    sumabs = max(float(T[name + ".sumabs"]), 1e-300)
    for got, ref in ((flat.sum(), T[name + ".sum"]), (np.abs(flat).sum(), T[name + ".sumabs"])):
        assert abs(got - float(ref)) / sumabs < 1e-11 * np.sqrt(flat.size), (name, got, float(ref))


def test_public_constants_match_the_reference(gpu_mixed):
    T = _cache.setdefault("tables", rr.load("reference_tables.npz"))
    for n in rr.CONSTS:                                      # the bound of test_gpu_parity.test_constants_match_oracle
        np.testing.assert_allclose(gpu_mixed.const(n), float(T["const." + n]), rtol=1e-15, atol=0, err_msg=n)


@pytest.mark.parametrize("b", ["warm120", "mixed33", "mixed120", "seeded120", "mixed200", "aero120"])
def test_p32n_step_matches_the_native_reference(request, b):
    """batch_step32_host(arith="p32n") against the record of the native (4-byte REAL) tree, at the statistic and bounds
    of test_gpu_precision.test_p32n_kernel_against_the_p32n_oracle."""
    rec = _rec("native")
    m, _ = _pair(request, rec, b)
    got = _inputs(rec, b, np.float32)
    gppt, _, _ = m.batch_step32_host(got, DT, arith="p32n")
    e = p32n_errors(got, rec, b)
    rp = rec[b + ".ppt"].astype(np.float64)
    pe = float((np.abs(gppt.astype(np.float64) - rp) / np.maximum(np.abs(rp), 1e-8)).max())
    med, q99 = float(np.median(e)), float(np.quantile(e, 0.99))
    print("%-9s p32n kernel vs native reference: median %.1e q99 %.1e max %.1e ppt %.1e" % (b, med, q99, e.max(), pe))
    assert all(np.isfinite(got[k]).all() for k in OUT)
    assert med < 3e-7 and q99 < 1e-4, (med, q99)
    assert pe < 1e-4, pe


@pytest.mark.parametrize("tag", ["warm", "mixed"])
def test_kid_adapter_matches_the_reference(gpu_warm, gpu_mixed, oracle_warm, oracle_mixed, tag):
    """kid_interface_host against the tendencies mphys_thompson09_interfacen itself backed out (nx = 3), at the metric
    and bound of test_gpu_kid_adapter.test_warm_tendencies_match_the_oracle_adapter, and its rate buffer against the
    rates that call logged through save_dg, at the bounds of rates_parity.assert_rates."""
    A = _cache.setdefault("adapter", rr.load("reference_adapter.npz"))
    m = gpu_warm if tag == "warm" else gpu_mixed
    nz, nx, dt, p0, r_on_cp, F, want = adapter_case(A, tag)
    keys = ("theta", "qv", "qc", "qr", "nr") + (() if tag == "warm" else ("qi", "ni", "qs", "qg"))
    state = {k: np.ascontiguousarray(F[k]) for k in keys}
    exner = np.ascontiguousarray(A[tag + ".in.exner"].reshape(nx, nz))
    dz = np.ascontiguousarray(A[tag + ".in.dz"])
    got = m.kid_interface_host(state, dt, p0, r_on_cp, exner, dz, want_rates=True)
    worst, nan = adapter_error(F, got, want, keys)
    print(tag, "adapter vs reference:", worst)
    assert nan == nx
    for k in keys:
        assert worst[k] < 1e-9, (k, worst)
    assert np.isfinite(got["qc"][:, 0]).all()                # U1: the record has no tendency of qc at kts
    # the rates: the oracle, stepped from the state the adapter gathers (W:60-94, U2 defaults), supplies the sensitivity only
    o = oracle_warm if tag == "warm" else oracle_mixed
    st = {k: np.ascontiguousarray(F[k]) for k in ("qv", "qc", "qi", "qr", "qs", "qg", "ni", "nr")}
    st["t"], st["p"] = np.ascontiguousarray(F["theta"] * exner), np.ascontiguousarray(p0 * exner ** (1.0 / r_on_cp))
    st["nc"], st["nwfa"], st["nifa"] = (np.ascontiguousarray(a) for a in o.default_aerosols(st["qv"], st["t"], st["p"]))
    st["w"], st["dz"] = np.zeros((nx, nz)), np.ascontiguousarray(np.broadcast_to(dz, (nx, nz)))
    logged = adapter_logged_rates(A, tag, nz, nx)
    rv = assert_rates(o.column_step, st, dt, got["rates"], record=logged)
    rv.pop("cmp")
    print(tag, "adapter rates vs the logged ones:", rv)
    assert np.array_equal(np.any(got["rates"] != 0, axis=(0, 2)), np.any(logged != 0, axis=(0, 2)))   # the same rows reached
    assert np.any(logged != 0, axis=(0, 2)).sum() >= 4
