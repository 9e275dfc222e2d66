#!/usr/bin/env python
"""tools/bench_kid_aerosol.py -- time the aerosol entries (include/kidmp_aerosol.h) on one MI355X beside the nine-field
entries they extend, on the same state and in the same aerosol-aware context.

Workloads: 10^5 and 10^4 mixed-phase columns x 120 levels (BASELINE config 3) in KiD's theta form with the aerosol loads of
the tests, fp64, state in HBM; for the slab variants the same columns as --nx (1000) cells per slab.  All variants run in
ONE process, warmed up, taking turns launch by launch; every launch is timed with device events of its own and the median
of --reps (30) launches is reported with the minimum and maximum beside it.  Pairs (new / parent's entry):
  kid_interface_aero / kid_interface      the adapter with adv = sum; the new one also reads w and a surface source
  advect_aero_sum / advect_sum            three members without courant / nine members with courant
  update_aero / update
  run_aero_step / run_step                advect(+aero), the centre updraft, the adapter, update(+aero), the ppt accumulation
  advect_slab_aero_sum / advect_slab_sum, run_slab_aero_step / run_slab_step      the same on periodic slabs
The state is put back before every launch that changes it (outside the timed span).  Algorithmic bytes per column (profiles
read + written, x nz x 8) and their share of 8 TB/s are printed for the streaming entries; the adapter pair has none (the
column step is not a streaming kernel), its line gives the extra bytes of the aerosol gather and back-out instead.
Prints one line per variant and workload and ONE JSON line at the end; the lines also go to --out
(profiles/r18_kid_aerosol.txt) under a header with the date and the library's fingerprint."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NZ = 120
HBM_PEAK = 8.0e12
P0, R_ON_CP, DT = 1.0e5, 287.058 / 1005.0, 10.0


def measure(a, ncol, lines):
    import numpy as np
    import torch
    import cases
    from kid_amd import AEROSOL_FIELDS, KID_FIELDS, ThompsonMP, streamfunction_flow
    from kid_amd.aerosol import centre_updraft

    def say(s):
        print(s)
        lines.append(s)

    nx = a.nx
    assert ncol % nx == 0, (ncol, nx)
    nslab = ncol // nx
    m = ThompsonMP(iiwarm=False, device=0, aerosol_aware=True)
    st = cases.config3(ncol)
    rng = np.random.default_rng(5)
    st["nwfa"] = st["nwfa"] * rng.uniform(0.3, 30.0, size=(ncol, 1))
    st["nifa"] = st["nifa"] * rng.uniform(0.5, 200.0, size=(ncol, 1))
    st["nc"] = st["nc"] * rng.uniform(0.2, 3.0, size=st["nc"].shape)
    exner = (st["p"] / P0) ** R_ON_CP
    F = {k: st[k] for k in KID_FIELDS[1:] + AEROSOL_FIELDS}
    F["theta"] = st["t"] / exner
    rho = 0.622 * st["p"][0] / (287.04 * st["t"][0] * (st["qv"][0] + 0.622))
    dz = st["dz"][0]
    dx = 4.0 * float(dz.mean())
    x = (np.arange(nx) / float(nx))[None, :, None]
    f = (np.arange(NZ + 1) / float(NZ))[None, None, :]
    rng = np.random.Generator(np.random.PCG64(18))
    psi = rng.uniform(0.3, 1.0, (nslab, 1, 1)) * np.sin(2.0 * np.pi * rng.integers(1, 4, (nslab, 1, 1)) * x
                                                          + rng.uniform(0.0, 6.0, (nslab, 1, 1))) * np.sin(np.pi * f)
    cu = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0")   # noqa: E731
    first = {k: cu(F[k]) for k in F}
    state = {k: v.clone() for k, v in first.items()}
    nine, aer = {k: state[k] for k in KID_FIELDS}, {k: state[k] for k in AEROSOL_FIELDS}
    drho, ddz, dex = cu(rho), cu(dz), cu(exner)
    du, dw = streamfunction_flow(cu(psi.reshape(ncol, NZ + 1)), drho, ddz, dx, nx=nx)
    one = float(m.kid_advect_slab(nine, du, dw, drho, ddz, dx, DT, nx, want=(), courant=True)["courant"].max())
    du, dw = du * (0.5 / one), dw * (0.5 / one)
    src = cu(np.full(ncol, 5.0e4))

    def restore():
        for k in state:
            state[k].copy_(first[k])

    o9 = m.kid_advect(nine, dw, drho, ddz, DT, want="sum", courant=True)
    o3 = m.kid_advect_aero(aer, dw, drho, ddz, DT, want="sum")
    s9 = m.kid_advect_slab(nine, du, dw, drho, ddz, dx, DT, nx, want="sum", courant=True)
    s3 = m.kid_advect_slab_aero(aer, du, dw, drho, ddz, dx, DT, nx, want="sum")
    both, sboth = dict(o9["sum"], **o3["sum"]), dict(s9["sum"], **s3["sum"])
    wc = centre_updraft(dw).contiguous()
    work = m.kid_workspace(ncol, NZ, torch.float64)
    mp9 = m.kid_interface(nine, DT, P0, R_ON_CP, dex, ddz, adv=o9["sum"], work=work)
    mp12 = m.kid_interface_aero(state, DT, P0, R_ON_CP, dex, ddz, adv=both, w=wc, nwfa_source=src, work=work)
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")

    def step9(slab):
        if slab:
            m.kid_advect_slab(nine, du, dw, drho, ddz, dx, DT, nx, want="sum", courant=True, out=s9)
        else:
            m.kid_advect(nine, dw, drho, ddz, DT, want="sum", courant=True, out=o9)
        adv = s9 if slab else o9
        m.kid_interface(nine, DT, P0, R_ON_CP, dex, ddz, adv=adv["sum"], work=work, out=mp9)
        m.kid_update(nine, DT, adv["sum"], mp9)
        ppt.add_(mp9["ppt"])

    def step12(slab):
        if slab:
            m.kid_advect_slab(nine, du, dw, drho, ddz, dx, DT, nx, want="sum", courant=True, out=s9)
            m.kid_advect_slab_aero(aer, du, dw, drho, ddz, dx, DT, nx, want="sum", out=s3)
        else:
            m.kid_advect(nine, dw, drho, ddz, DT, want="sum", courant=True, out=o9)
            m.kid_advect_aero(aer, dw, drho, ddz, DT, want="sum", out=o3)
        a9, a3 = (s9, s3) if slab else (o9, o3)
        centre_updraft(dw, out=wc)
        m.kid_interface_aero(state, DT, P0, R_ON_CP, dex, ddz, adv=sboth if slab else both, w=wc, nwfa_source=src, work=work, out=mp12)
        m.kid_update(nine, DT, a9["sum"], mp12)
        m.kid_update_aero(aer, DT, a3["sum"], mp12)
        ppt.add_(mp12["ppt"])

    # name -> (call, algorithmic profiles per column or None, changes the state); pairs: new entry, then the parent's
    variants = {
        "kid_interface_aero": (lambda: m.kid_interface_aero(state, DT, P0, R_ON_CP, dex, ddz, adv=both, w=wc, nwfa_source=src, work=work,
                                                            out=mp12), None, False),
        "kid_interface": (lambda: m.kid_interface(nine, DT, P0, R_ON_CP, dex, ddz, adv=o9["sum"], work=work, out=mp9), None, False),
        "advect_aero_sum": (lambda: m.kid_advect_aero(aer, dw, drho, ddz, DT, want="sum", out=o3), 7, False),
        "advect_sum": (lambda: m.kid_advect(nine, dw, drho, ddz, DT, want="sum", courant=True, out=o9), 19, False),
        "update_aero": (lambda: m.kid_update_aero(aer, DT, o3["sum"], mp12), 12, True),
        "update": (lambda: m.kid_update(nine, DT, o9["sum"], mp9), 36, True),
        "run_aero_step": (lambda: step12(False), None, True),
        "run_step": (lambda: step9(False), None, True),
        "advect_slab_aero_sum": (lambda: m.kid_advect_slab_aero(aer, du, dw, drho, ddz, dx, DT, nx, want="sum", out=s3), 8, False),
        "advect_slab_sum": (lambda: m.kid_advect_slab(nine, du, dw, drho, ddz, dx, DT, nx, want="sum", courant=True, out=s9), 20, False),
        "run_slab_aero_step": (lambda: step12(True), None, True),
        "run_slab_step": (lambda: step9(True), None, True),
    }
    say("ncol=%-6d = %d slabs x %d cells x %d levels; courant max %.3f (slab), %.3f (1-D)"
        % (ncol, nslab, nx, NZ, float(s9["courant"].max()), float(o9["courant"].max())))
    for _ in range(a.warmup):
        for fn, _n, _c in variants.values():
            fn()
    restore()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, (fn, _n, changes) in variants.items():
            if changes:
                restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"ncol": ncol, "nslab": nslab, "nx": nx, "nz": NZ, "reps": a.reps}
    for k, t in times.items():
        res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
        nprof = variants[k][1]
        extra = ""
        if nprof is not None:
            res[k]["algo_bytes_per_column"] = nprof * NZ * 8
            res[k]["share_of_8TBs"] = res[k]["algo_bytes_per_column"] * ncol / (res[k]["ms_median"] * 1e-3) / HBM_PEAK
            extra = "   %6d B/column -> %5.1f %% of 8 TB/s" % (res[k]["algo_bytes_per_column"], 100.0 * res[k]["share_of_8TBs"])
        say("ncol=%-6d %-21s median %8.4f ms   min %8.4f   max %8.4f%s" % (ncol, k, res[k]["ms_median"], min(t), max(t), extra))
    ms = {k: res[k]["ms_median"] for k in variants}
    names = list(variants)
    res["ratios"] = {}
    for new, old in zip(names[0::2], names[1::2]):
        res["ratios"][new + "/" + old] = ms[new] / ms[old]
        say("ncol=%-6d %-21s is %.3fx %s (%+.4f ms)" % (ncol, new, ms[new] / ms[old], old, ms[new] - ms[old]))
    # the adapter's extra traffic: gather 3 x (state, adv) + w in, 4 profiles out instead of 4 written anyway; back-out 3 x
    # (state, adv, post) in, 3 out: 19 profiles more than the nine-field call moves
    res["kid_interface_aero"]["extra_algo_bytes_per_column"] = 19 * NZ * 8
    say("ncol=%-6d kid_interface_aero moves %d B/column more than kid_interface (19 profiles): %.4f ms at 8 TB/s, measured +%.4f ms"
        % (ncol, 19 * NZ * 8, 19 * NZ * 8 * ncol / HBM_PEAK * 1e3, ms["kid_interface_aero"] - ms["kid_interface"]))
    for new, old in (("advect_aero_sum", "advect_sum"), ("advect_slab_aero_sum", "advect_slab_sum")):
        say("ncol=%-6d %s costs %.3f of %s; a third would be 0.333 (the face setup is paid again)" % (ncol, new, ms[new] / ms[old], old))
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--nx", type=int, default=1000, help="cells per slab; every --ncols must be a multiple")
    ap.add_argument("--lib", default=None, help="another build of the library")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_kid_aerosol.txt"))
    a = ap.parse_args()
    import torch
    import kid_amd
    if not torch.cuda.is_available():
        sys.exit("bench_kid_aerosol: no GPU visible (this measurement has no CPU path)")
    if a.lib:
        kid_amd.load_library(a.lib)
    m = kid_amd.ThompsonMP(iiwarm=False, device=0, aerosol_aware=True)
    lines = ["# tools/bench_kid_aerosol.py  %s  %s%s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0),
                                                          "  --lib " + a.lib if a.lib else ""),
             "# fingerprint: %s" % m.kernel_fingerprint()]
    m.close()
    results = [measure(a, n, lines) for n in a.ncols]
    lines.append(json.dumps({"bench": "kid_aerosol", "device": torch.cuda.get_device_name(0), "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
