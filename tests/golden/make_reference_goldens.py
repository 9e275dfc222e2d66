"""Records tests/golden/reference_{p64,native}{,_seeded,_more}.npz, reference_tables.npz and reference_adapter.npz
from the reference Fortran built from source (`make -C oracle ref` -> oracle/_ref/{p64,native}/ref_driver); the step
records of a tree take three files so that each stays under 256 KB.  Run by hand, from the repository root:

    python tests/golden/make_reference_goldens.py

The first run of a tree builds the reference's own racg / racs tables (about a minute and a half), later ones reuse
them (l_reuse_thompson_lookup).  The files hold inputs and what the Fortran computed from them, nothing else.

What is NOT recorded, and why:
  U1  output qc and nc at level kts: the reference reads the never-assigned vtck / vtnck there (M:3415-3424 with
      ksed1(5) = 1), so the value is whatever the compiler left in those arrays.  Written as NaN, and with it the one
      figure derived from it: re_qc at kts of calc_effectRad on the stepped state.  The inputs keep T(kts) >= HGFR, so
      that block Q cannot carry that qc into qi, ni or t.
  U4  a column in which the oracle had to clamp the second index of t_Efrw / t_Efsw is one in which the reference reads
      out of bounds: it is replaced by the next candidate, never masked.
Every driver run is made twice and must give the same bits outside the U1 entries.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases                                                 # noqa: E402
import kat_cases as kc                                       # noqa: E402
import reference_record as rr                                # noqa: E402
from oracle.oracle import Oracle, u4_count                   # noqa: E402
from parity import MAX_SENSITIVE_FRAC, OUT, branch_aware_compare        # noqa: E402
from test_gpu_variants import _resample                      # noqa: E402

DT = 10.0
HGFR = 235.16
NSEEDED = 6
RATE_COLS = dict(warm120=(0, 1), mixed120=(0, 6), seeded120=(0, 6))     # KAT-A warm, KAT-B; KAT-A mixed, riming, config3, config5
# one file holds at most 256 KB, so the batches of a tree go to three files: reference_<tree><suffix>.npz
FILES = {"": ("warm120", "mixed120"), "_seeded": ("seeded120",), "_more": ("mixed33", "mixed200", "aero120")}
MAX_BYTES = 256 * 1024
f32 = np.float32


def _stack(cols):
    return {k: np.ascontiguousarray(np.stack([np.asarray(c[k], dtype=np.float64) for c in cols])) for k in cases.KEYS}


def _rows(st, idx):
    return [{k: st[k][i] for k in cases.KEYS} for i in idx]


def _reaches_u4(oracle, col):
    st = {k: np.ascontiguousarray(np.asarray(col[k], dtype=np.float64)[None].copy()) for k in cases.KEYS}
    n0 = u4_count()
    oracle.batch_step(st, DT, nthreads=1)
    return u4_count() != n0


def _admissible(oracle, pool, want):
    """The first `want` columns of `pool` that stay clear of U4 and keep T(kts) >= HGFR."""
    out = []
    for col in pool:
        if col["t"][0] >= HGFR and not _reaches_u4(oracle, col):
            out.append(col)
        if len(out) == want:
            return out
    raise SystemExit("not enough admissible columns")


def batches(o_warm, o_mixed):
    """{name: (iiwarm, aerosol_aware, inputs)} in binary64."""
    c3 = _admissible(o_mixed, _rows(cases.config3(4 * NSEEDED), range(4 * NSEEDED)), NSEEDED)
    c5 = _admissible(o_mixed, _rows(cases.config5(4 * NSEEDED), range(4 * NSEEDED)), NSEEDED)
    edge = _rows(cases.edge_cases(), range(9))               # 0 is KAT-A mixed, 4 is KAT-C, 5 is KAT-A warm in a mixed tree
    assert all(np.array_equal(edge[0][k], kc.kat_a(True)[k]) and np.array_equal(edge[4][k], kc.kat_c()[k]) for k in cases.KEYS)
    warm = [kc.kat_a(False), cases.warm_column_t0(), cases.warm_column_t900()]      # KAT-A warm, KAT-B step 1, config 2
    for col in warm:
        assert col["t"][0] >= HGFR and not _reaches_u4(o_warm, col)
    for col in edge:
        assert col["t"][0] >= HGFR and not _reaches_u4(o_mixed, col), "an edge case reaches U4 or freezes at kts"
    out = dict(warm120=(True, False, _stack(warm)), mixed120=(False, False, _stack(edge)),
               seeded120=(False, False, _stack(c3 + c5)))
    pick = [kc.kat_a(True), kc.kat_c(), c3[0]]
    for nz in (33, 200):
        cols = [_resample(c, nz) for c in pick]
        assert not any(_reaches_u4(o_mixed, c) for c in cols)
        out["mixed%d" % nz] = (False, False, _stack(cols))
    aero = _stack([edge[0], edge[6], edge[7], c3[0], c3[1], c5[0]])
    aero["w"][:] = 2.0                                       # an updraft, so that activation has something to do
    out["aero120"] = (False, True, aero)
    return out


def native_inputs(b64):
    """The same selection in binary32; KAT-A and KAT-B as a default-REAL driver forms them (kat_native_inputs.npz)."""
    out = {}
    for name, (iiwarm, aero, st) in b64.items():
        out[name] = (iiwarm, aero, {k: np.ascontiguousarray(v.astype(f32)) for k, v in st.items()})
    a_w, a_m, b = kc.kat_a_native_formed(False), kc.kat_a_native_formed(True), kc.kat_b_native_formed()
    g = np.load(os.path.join(HERE, "kat_native_inputs.npz"))
    for k in ("t", "p", "qv", "nc"):
        assert np.array_equal(a_m[k], g["a_" + k]), "this host's powf / expf do not form the committed native inputs"
    for k in cases.KEYS:
        out["warm120"][2][k][0] = a_w[k]
        out["mixed120"][2][k][0] = a_m[k]
        out["aero120"][2][k][0] = a_m[k]
    out["aero120"][2]["w"][0] = f32(2.0)
    # KAT-B step 1 as the adapter forms it in binary32: t = theta*exner, p = p0*exner**(1/r_on_cp) (W:60-61)
    m = kc._libm32()
    ex = float(f32(1.0) / f32(b["r_on_cp"]))
    w = out["warm120"][2]
    w["t"][1] = (b["theta"] * b["exner"]).astype(f32)
    w["p"][1] = (f32(b["p0"]) * np.array([m.powf(float(e), ex) for e in b["exner"]], dtype=f32)).astype(f32)
    w["qv"][1] = b["qv"]
    w["qc"][1], w["qr"][1], w["nr"][1] = b["hydro"][0, 0, 0], b["hydro"][0, 1, 0], b["hydro"][1, 1, 0]
    rho = (f32(0.622) * w["p"][1] / (f32(287.04) * w["t"][1] * (w["qv"][1] + f32(0.622)))).astype(f32)
    w["nc"][1], w["nwfa"][1], w["nifa"][1] = f32(1e8) / rho, f32(11.1e6) / rho, f32(5e3) / rho
    return out


def check_native_u4(o_warm, o_mixed, o_aero, b32):
    """U4 again for the binary32 inputs in the native arithmetic (the P32n oracle's own count of clamped reads): the
    selection is the binary64 one, so a batch that reaches U4 here stops the generator instead of being replaced."""
    for name, (iiwarm, aero, st) in sorted(b32.items()):
        o = o_warm if iiwarm else (o_aero if aero else o_mixed)
        n0 = u4_count(p32n=True)
        o.batch_step_p32n({k: v.copy() for k, v in st.items()}, DT)
        assert u4_count(p32n=True) == n0, "%s reaches U4 in the native arithmetic" % name


def _mask_u1(res):
    res["qc"][:, 0] = np.nan
    res["nc"][:, 0] = np.nan
    res["re_qc"][:, 0] = np.nan                              # calc_effectRad of that qc and nc (the stepped state only)


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in a)


def record_steps(tree, b):
    """One warm and one mixed process per pass, two passes; {"<batch>.<field>": array}."""
    out = {}
    for iiwarm in (True, False):
        names = [n for n in sorted(b) if b[n][0] == iiwarm]
        blocks = [(b[n][2], b[n][1]) for n in names]
        first, second = (rr.run_step(tree, iiwarm, blocks, DT) for _ in range(2))
        for n, r1, r2 in zip(names, first, second):
            _mask_u1(r1)
            _mask_u1(r2)
            if not _same_bits(r1, r2):
                raise SystemExit("%s %s: two runs of the reference differ outside U1, nothing written" % (tree, n))
            nan = {k: int(np.isnan(v).sum()) for k, v in r1.items() if np.isnan(v).any()}
            assert set(nan) <= {"qc", "nc", "re_qc"} and all(v == r1["qc"].shape[0] for v in nan.values()), (n, nan)
            st = b[n][2]
            out[n + ".iiwarm"], out[n + ".aero"] = np.bool_(iiwarm), np.bool_(b[n][1])
            for k in cases.KEYS:
                out["%s.in.%s" % (n, k)] = st[k]
            real = rr.TREES[tree]
            for k in OUT:                                    # what the Fortran returned, in the tree's own REAL
                assert np.array_equal(r1[k].astype(real).astype(np.float64), r1[k], equal_nan=True)
                out["%s.out.%s" % (n, k)] = r1[k].astype(real)
            out[n + ".ppt"] = r1["ppt"].astype(real)
            for k in rr.DIAG:
                out["%s.%s" % (n, k)] = r1[k].astype(real)
                out["%s.%s_in" % (n, k)] = r1[k + "_in"].astype(real)
            if n in RATE_COLS:
                out[n + ".rate_cols"] = np.array(RATE_COLS[n])
                out[n + ".rates"] = r1["rates"][list(RATE_COLS[n])]
    return out


def check_conditioning(o_warm, o_mixed, o_aero, b):
    """The oracle alone: each batch leaves at most parity.MAX_SENSITIVE_FRAC of its levels to the sensitivity allowance."""
    for name, (iiwarm, aero, st) in sorted(b.items()):
        o = o_warm if iiwarm else (o_aero if aero else o_mixed)
        ref = {k: v.copy() for k, v in st.items()}
        o.batch_step(ref, DT)
        cmp = branch_aware_compare(o, st, DT, ref)
        n = int((cmp["sens"] > 1e-11).sum())
        print("%-9s sensitive levels %d of %d, branch levels %d" % (name, n, cmp["sens"].size, int((cmp["flags"] != 0).sum())))
        assert n <= int(np.ceil(MAX_SENSITIVE_FRAC * cmp["sens"].size)), (name, n)


def record_tables():
    rng = np.random.Generator(np.random.PCG64(cases.SEED + 9))
    (t1, c1), (t2, c2) = rr.run_tables("p64"), rr.run_tables("p64")
    out = {}
    for name in rr.TABLES:
        assert np.array_equal(t1[name].view(np.uint64), t2[name].view(np.uint64)), name
        flat = t1[name].ravel(order="F")
        idx = np.sort(rng.choice(flat.size, size=min(512, flat.size), replace=False))
        out[name + ".shape"] = np.array(t1[name].shape)
        out[name + ".idx"] = idx.astype(np.int64)
        out[name + ".val"] = flat[idx]
        out[name + ".sum"] = np.float64(flat.sum())
        out[name + ".sumabs"] = np.float64(np.abs(flat).sum())
    assert c1 == c2
    for k, v in c1.items():
        out["const." + k] = np.float64(v)
    return out


def adapter_inputs(nx, native):
    """KAT-B's forcing on nx columns (rain scaled by 1 + 0.2 i); the mixed tree adds KAT-A's frozen species at KAT-B's
    levels.  Flattened Fortran order, as Oracle.kid_interface takes them."""
    c = kc.kat_b_native() if native else kc.kat_b()
    real = f32 if native else np.float64
    nz = c["nz"]
    rep = lambda a: np.ascontiguousarray(np.tile(np.asarray(a, dtype=real), nx))                 # noqa: E731
    hy = np.zeros((2, 5, nx, nz), dtype=real)
    for i in range(nx):
        hy[:, :, i, :] = c["hydro"][:, :, 0, :]
        hy[0, 1, i, :] *= real(1.0 + 0.2 * i)
    return dict(nz=nz, nx=nx, dt=c["dt"], p0=c["p0"], r_on_cp=c["r_on_cp"], theta=rep(c["theta"]), exner=rep(c["exner"]),
                dz=np.asarray(c["dz"], dtype=real), qv=rep(c["qv"]), hydro=hy.ravel())


def record_adapter(tree):
    out = {}
    for iiwarm in (True, False):
        c = adapter_inputs(3, tree == "native")
        if not iiwarm:                                       # something frozen for the mixed tree to act on
            hy = c["hydro"].reshape(2, 5, 3, c["nz"])
            live = hy[0, 0, 0] > 0
            hy[0, 3, :, live] = 2e-4
            hy[0, 4, :, live] = 1e-4
            c["theta"] = c["theta"] - c["theta"].dtype.type(30.0)          # 30 K colder, and dry enough to stay subsaturated
            c["qv"] = c["qv"] * c["qv"].dtype.type(0.1)
        o, z, zh, n0 = Oracle(iiwarm=iiwarm), np.zeros(3 * c["nz"]), np.zeros(30 * c["nz"]), u4_count()
        o.kid_interface(c["nz"], 3, c["dt"], c["p0"], c["r_on_cp"], c["theta"], z, z, c["exner"], c["dz"], c["qv"], z, z,
                        c["hydro"], zh, zh)
        assert u4_count() == n0 and (c["theta"] * c["exner"])[0] >= HGFR, "the adapter columns reach U4 or freeze at kts"
        a, b = rr.run_adapter(tree, iiwarm, c), rr.run_adapter(tree, iiwarm, c)
        # total_ppt_level is written from a local array nothing assigns (W:32, W:307): not a result
        log = [[e for e in r[3] if e[1] != "total_ppt_level"] for r in (a, b)]
        assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[:3], b[:3])) and log[0] == log[1]
        tag = "warm" if iiwarm else "mixed"
        for k in ("theta", "exner", "dz", "qv", "hydro"):
            out["%s.in.%s" % (tag, k)] = c[k]
        for k in ("nz", "nx", "dt", "p0", "r_on_cp"):
            out["%s.%s" % (tag, k)] = np.float64(c[k])
        dhy = a[2].reshape(2, 5, 3, c["nz"]).copy()
        dhy[0, 0, :, 0] = np.nan                             # U1: the tendency of qc at kts is backed out of an undefined qc
        assert not np.isnan(a[0]).any() and not np.isnan(a[1]).any() and np.isnan(dhy).sum() == 3
        out[tag + ".dth"], out[tag + ".dqv"], out[tag + ".dhy"] = a[0], a[1], dhy.ravel()
        # the save_dg log in call order: the name and the form of an entry as indices into the lists of distinct ones
        names, forms = sorted({e[1] for e in log[0]}), sorted({e[0] for e in log[0]})
        out[tag + ".log_names"], out[tag + ".log_forms"] = np.array(names), np.array(forms)
        out[tag + ".log_name"] = np.array([names.index(e[1]) for e in log[0]], dtype=np.uint8)
        out[tag + ".log_form"] = np.array([forms.index(e[0]) for e in log[0]], dtype=np.uint8)
        out[tag + ".log_k"] = np.array([e[2] for e in log[0]], dtype=np.int16)
        out[tag + ".log_i"] = np.array([e[3] for e in log[0]], dtype=np.int16)
        out[tag + ".log_v"] = np.array([e[4] for e in log[0]])
    return out


def save(name, arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (name, size))
    assert size < MAX_BYTES, (name, size)


def main():
    for tree in rr.TREES:
        if not rr.have_driver(tree):
            raise SystemExit("oracle/_ref/%s/ref_driver is missing: make -C oracle ref" % tree)
    o_warm, o_mixed, o_aero = Oracle(iiwarm=True), Oracle(iiwarm=False), Oracle(iiwarm=False, aerosol_aware=True)
    b64 = batches(o_warm, o_mixed)
    check_conditioning(o_warm, o_mixed, o_aero, b64)
    b32 = native_inputs(b64)
    check_native_u4(o_warm, o_mixed, o_aero, b32)
    for tree, b in (("p64", b64), ("native", b32)):
        rec = record_steps(tree, b)
        for suffix, names in FILES.items():
            part = {k: v for k, v in rec.items() if k.split(".")[0] in names}
            part["dt"], part["batches"] = np.float64(DT), np.array(names)
            save("reference_%s%s.npz" % (tree, suffix), part)
    save("reference_tables.npz", record_tables())
    save("reference_adapter.npz", record_adapter("p64"))


if __name__ == "__main__":
    main()
